"""Read NDJSON rows back into a framed stream on the GPU (``ops/hip/telemetry_import.hip``): the device
path of ``python -m beholder_amd import --device gpu`` (:mod:`beholder_amd.import_rows` defines the
result).

The stages, which ``scripts/gpu_import_probe.py`` times one by one:

1. :func:`upload` — the text goes to the device as it lies in the file, plus one ``\\n`` where it
   does not end in one. :class:`TooLarge` where that reaches 2^31 bytes, before anything is uploaded.
   The frames are always shorter than their rows (``telemetry_import.hpp`` says why), so the output
   needs no size check of its own.
2. :func:`split` — the device finds the lines: a count of the ``\\n`` bytes per tile of 4096 bytes,
   the extract's scan over the tiles' counts, and a second pass that ranks every newline and writes
   the line starts, ``n + 1`` int32. They play the part ``gpu_fold.index`` plays for the other
   commands; the host does no pass over the bytes and reads back one word, the line count.
3. :func:`classify` — one lane per line reads the row and stores its plan (a kind, the topic byte,
   the text spans and decoded lengths, the numbers) and the exact length of its frame, 0 for a blank
   line. A line the device does not write (a byte >= 0x80, a status by name, an unknown key, anything
   its reader does not recognise) goes to the overflow list with length 0.
4. :func:`decide_on_host` — reads the counters; where the overflow list is not empty the host asks
   ``import_rows.frame_of_row`` about those lines in ascending order, raises at the first malformed
   one under ``fail``, keeps the frames and scatters their lengths into ``keep_len`` before the scan.
5. ``gpu_extract.scan`` and ``totals`` — the extract's prefix sum, as it is, over this module's
   ``keep_len``: every frame's offset, and the one word that sizes the output.
6. :func:`emit` — a wave per 64 lines writes the planned frames' bytes at their offsets. It writes
   nothing into the spans of host rows.
7. :func:`collect` — the output and the line positions come back, and the host splices its frames
   into their spans.

The tables, the scatter, the emit's front and :func:`collect` are the rewriting commands' own
(``ops/gpu_rewrite.py``), shared with the normalise, the anonymise and the export.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`import_rows`.
"""
from __future__ import annotations

from typing import NamedTuple

from . import gpu_extract, gpu_rewrite, hip_lib
from .gpu_rewrite import HostParts, Tables, collect  # noqa: F401  collect: stage 7, as it is, over the lines

C_EVENTS, C_CARRIED, C_BLANK, C_OVERFLOW, N_COUNTERS = 0, 1, 2, 3, 4  # counters[] of the kernels
IM_BLANK, IM_B64, IM_STATUS, IM_PROGRESS, IM_HOST = 0, 1, 2, 3, 4  # FramePlan::kind of telemetry_import.hpp
PLAN_FIELDS = ("kind", "topic", "id_off", "id_text", "id_len", "host_off", "host_text", "host_len", "status", "progress",
               "out_len", "reserved")
TILE_BYTES = 4096  # SPLIT_TILE_BYTES of telemetry_import.hpp
LIMIT = 2 ** 31    # the line starts are int32


class TooLarge(ValueError):
    """The text does not stay below 2^31 bytes."""


class Lines(NamedTuple):
    """What :func:`split` found."""
    n: int          # the lines
    starts: object  # n + 1 int32 on the device: line m is buf[starts[m], starts[m + 1] - 1)


def _check_policy(policy) -> None:
    from .. import import_rows as definition
    definition._check_policy(policy)


def text_size(data) -> int:
    """The bytes that go to the device: ``data`` and one ``\\n`` where it does not end in one."""
    view = memoryview(data)
    return view.nbytes + (1 if view.nbytes and view[view.nbytes - 1] != 0x0A else 0)


def checked_size(data) -> int:
    """:func:`text_size`, or :class:`TooLarge` where it reaches 2^31 bytes."""
    size = text_size(data)
    if size >= LIMIT:
        raise TooLarge(f"the text takes {size} bytes, past the 2^31 bytes that the device's offsets reach")
    return size


def upload(data, device="cuda"):
    """The text on ``device``, ending in a newline. :class:`TooLarge` for 2^31 bytes or more, before
    anything is uploaded."""
    import warnings

    import torch
    size = checked_size(data)
    raw = memoryview(data).nbytes
    buf = torch.empty(size, dtype=torch.uint8, device=device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # a read-only view is all the copy needs
        buf[:raw].copy_(torch.frombuffer(data, dtype=torch.uint8))
    if size > raw:
        buf[raw:].fill_(0x0A)
    return buf


def _check_text(buf_dev) -> None:
    import torch
    if buf_dev.dtype != torch.uint8 or not buf_dev.is_cuda or not buf_dev.is_contiguous() or buf_dev.dim() != 1:
        raise ValueError("the kernels need a contiguous uint8 buf on a GPU")
    if not 1 <= buf_dev.numel() < LIMIT:
        raise ValueError("the text is 1 to 2^31 - 1 bytes")
    if buf_dev.data_ptr() % 16:
        raise ValueError("the text starts at a multiple of 16 bytes, for the split's wide loads")


def split(buf_dev) -> Lines:
    """The lines of the text in ``buf_dev``, which ends in a newline (:func:`upload`): count, the
    extract's scan over the tiles' counts, one word read back, and the starts."""
    import torch
    _check_text(buf_dev)
    size = buf_dev.numel()
    tiles = (size + TILE_BYTES - 1) // TILE_BYTES
    counts = torch.empty(tiles, dtype=torch.int32, device=buf_dev.device)
    hip_lib.call("bh_import_count", buf_dev, buf_dev.data_ptr(), size, counts.data_ptr())
    s = gpu_extract.scan_tables(counts, tiles, buf_dev, None)
    gpu_extract.scan(s)
    n = gpu_extract.totals(s)[1]  # the low word sums the counts: the text's newlines
    starts = torch.empty(n + 1, dtype=torch.int32, device=buf_dev.device)
    hip_lib.call("bh_import_starts", buf_dev, buf_dev.data_ptr(), size, s.pos.data_ptr(), n, starts.data_ptr())
    return Lines(n, starts)


def allocate(buf_dev, starts_dev, n: int) -> Tables:
    """Tables for ``n`` lines next to ``buf_dev``, the line starts in the place of ``offs``, zeroed
    where the kernels need it. Checks the arguments on the host."""
    _check_text(buf_dev)
    return gpu_rewrite.allocate(buf_dev, starts_dev, n, len(PLAN_FIELDS), N_COUNTERS, "the import")


def classify(t: Tables) -> None:
    """The classify launch over ``t`` on the current torch stream. ``t.offs`` must come from
    :func:`split`: the kernel trusts it. ``t.counters`` must be zero."""
    hip_lib.call("bh_import_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, t.plans.data_ptr(),
                 t.keep_len.data_ptr(), t.counters.data_ptr(), t.overflow.data_ptr())


def decide_on_host(t: Tables, data, policy, base: int = 0) -> HostParts:
    """Reads the counters. Where the overflow list is not empty, asks ``import_rows.frame_of_row``
    about those lines in ascending order and writes the lengths of their frames into ``t.keep_len``.
    Under ``fail`` the first malformed line raises ``ValueError`` with its number, ``base`` plus its
    position: the device leaves every malformed row to the host, so it is the input's first."""
    import torch

    from .. import import_rows as definition
    _check_policy(policy)
    count = int(t.counters[C_OVERFLOW].item())
    if count == 0:
        return gpu_rewrite.NO_HOST_PARTS
    rows = torch.sort(t.overflow[:count].to(torch.int64)).values
    spans = torch.stack((t.offs[rows], t.offs[rows + 1])).cpu().numpy()  # only these lines' starts come back
    frame = definition.decided_frame_of_row(policy)
    view = memoryview(data)
    where, parts, skipped = [], [], []
    events = carried = 0
    for i, a, b in zip(rows.cpu().numpy().tolist(), spans[0].tolist(), spans[1].tolist()):
        line = bytes(view[a:b - 1]).strip(definition.BLANK)  # b - 1 is the newline, or the end of a text without one
        try:
            f, from_b64 = frame(line)
        except definition.MalformedRow as e:
            if policy.malformed == "fail":
                raise definition.malformed_line(base + i, e) from None
            skipped.append(i)
            continue
        where.append(i)
        parts.append(f)
        carried += from_b64
        events += not from_b64
    return HostParts(count, gpu_rewrite.scatter(t, where, parts), parts, events, carried=carried, skipped=skipped)


def emit(t: Tables, kept: int, kept_bytes: int):
    """The output in a new device buffer of exactly ``kept_bytes``, the host frames' spans left as
    they are. ``kept`` and ``kept_bytes`` must be the totals of the scan over ``t.keep_len``: the
    kernel trusts them. No frame in the output launches nothing."""
    out = gpu_rewrite.emit_out(t, kept, kept_bytes, t.buf.numel())  # the frames are shorter than their rows
    if kept:
        hip_lib.call("bh_import_emit", t.buf, t.buf.data_ptr(), t.n, t.plans.data_ptr(), t.select.pos.data_ptr(),
                     out.data_ptr())
    return out


def import_rows(data, policy, device="cuda", base: int = 0):
    """``(Imported, rows decided on the host)`` of NDJSON text through the device."""
    from .. import import_rows as definition
    _check_policy(policy)
    definition._check_base(base)
    hip_lib.require_gpu(device, "import")
    size = checked_size(data)
    if size == 0:
        return definition.Imported(base=base, malformed=policy.malformed), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf = upload(data, device)
    lines = split(buf)
    t = allocate(buf, lines.starts, lines.n)
    classify(t)
    host = decide_on_host(t, data, policy, base)
    gpu_extract.scan(t.select)
    kept, kept_bytes = gpu_extract.totals(t.select)
    out = emit(t, kept, kept_bytes)
    frames, positions = collect(t, out, kept, host)
    counters = t.counters.cpu().numpy().tolist()
    return definition.Imported(frames, [base + i for i in positions], lines.n, counters[C_EVENTS] + host.events,
                               counters[C_CARRIED] + host.carried, [base + i for i in host.skipped], base,
                               policy.malformed), host.count
