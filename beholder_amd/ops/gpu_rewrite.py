"""The stages that the rewriting commands share: ``ops/gpu_normalise.py``, ``ops/gpu_anonymise.py``,
``ops/gpu_export.py`` and ``ops/gpu_import.py`` are one pipeline, and what does not depend on the
command is here. The kernels stay each command's own.

1. :func:`allocate` — the :class:`Tables`: a plan and a ``keep_len`` per frame, the counters, the
   overflow list and the extract's scan tables over ``keep_len``. The command's classify fills them.
2. The overflow list is decided on the host, by the command's own loop or by :func:`decide_with`,
   and :func:`scatter` writes the lengths of the host's parts into ``keep_len`` before the scan.
3. ``gpu_extract.scan`` and ``totals`` — the extract's prefix sum, as it is.
4. :func:`emit_out` — checks the scan's totals and allocates the output; the command launches its
   own emit kernel where anything is kept.
5. :func:`collect` — the output and the indices come back, and :func:`splice` copies the host's
   parts into their spans.

``hip_lib`` and ``gpu_extract`` are reached through their modules, so a patched ``hip_lib.call`` or
``hip_lib.lib`` holds here as it does in the commands.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from . import gpu_extract, hip_lib

LIMIT = 2 ** 31  # the scan keeps bytes in 32 bits and out_offs in int32


class Tables(NamedTuple):
    """The device tensors of one rewriting command; ``select`` holds the extract's over ``keep_len``,
    for its scan."""
    n: int
    buf: object
    offs: object      # the frame starts; the import's line starts
    plans: object     # (n, width) int32: the command's PLAN_FIELDS
    keep_len: object  # n int32: the length of the frame's output, 0 where it has none
    counters: object  # the command's N_COUNTERS int32
    overflow: object  # n int32
    select: gpu_extract.ScanTables
    base: int = 0     # the export's: the index of frame 0 in the whole input


class HostParts(NamedTuple):
    """What a command's ``decide_on_host`` keeps for :func:`collect`, and the tallies of the overflow
    list that the command adds to the device's."""
    count: int = 0                   # the overflow list's length
    frames: np.ndarray = np.zeros(0, dtype=np.int64)  # the frames (lines) among them with a part, ascending
    parts: Sequence[bytes] = ()      # their output frames (rows)
    events: int = 0                  # the decoded events among the list
    rewritten: int = 0               # normalise: those whose bytes changed
    carried: int = 0                 # import: the frames from b64 rows
    skipped: Sequence[int] = ()      # import: the malformed lines, ascending, as positions in the chunk


NO_HOST_PARTS = HostParts()


def check_undecoded(policy) -> None:
    if policy.undecoded not in ("keep", "drop"):
        raise ValueError("undecoded is keep or drop")


def allocate(buf_dev, offs_dev, n: int, width: int, n_counters: int, what: str, check=None, base: int = 0) -> Tables:
    """Tables for ``n`` frames with plans of ``width`` words next to ``buf_dev``, zeroed where the
    kernels need it. ``hip_lib.check_stream`` under the command's name ``what``, then the command's
    own ``check()``, come before any allocation."""
    import torch
    hip_lib.check_stream(buf_dev, offs_dev, n, what)
    if check is not None:
        check()
    dev = buf_dev.device
    keep_len = torch.empty(n, dtype=torch.int32, device=dev)
    return Tables(n, buf_dev, offs_dev, torch.empty((n, width), dtype=torch.int32, device=dev), keep_len,
                  torch.zeros(n_counters, dtype=torch.int32, device=dev),
                  torch.empty(n, dtype=torch.int32, device=dev),
                  gpu_extract.scan_tables(keep_len, n, buf_dev, offs_dev), base)


def scatter(t: Tables, where: Sequence[int], parts: Sequence[bytes]) -> np.ndarray:
    """Writes the lengths of the host's ``parts`` into ``t.keep_len`` at the frames ``where``, before
    the scan; nothing for an empty list. Returns ``where`` as an array, for :class:`HostParts`."""
    frames = np.asarray(where, dtype=np.int64)
    if len(parts):
        import torch
        dev = t.buf.device
        lengths = np.fromiter(map(len, parts), dtype=np.int32, count=len(parts))
        t.keep_len[torch.from_numpy(frames).to(dev)] = torch.from_numpy(lengths).to(dev)
    return frames


def decide_with(t: Tables, c_overflow: int, data, offs: np.ndarray, make_canon, check) -> HostParts:
    """The normalise's and the anonymise's ``decide_on_host``: ``t.counters[c_overflow]`` is the
    overflow list's length in the command's layout, ``make_canon()`` gives the per-frame function,
    made only where the list is not empty, and ``check(size, n, extra)`` is the command's size check
    over what the host's frames grow by."""
    from .. import normalise
    from ..coalesce import DROP, KEEP
    count = int(t.counters[c_overflow].item())
    if count == 0:
        return NO_HOST_PARTS
    canon = make_canon()
    where, parts = [], []
    events = rewritten = growth = 0
    for i, topic, body in hip_lib.overflow_frames(t.overflow, count, data, offs)[1]:
        c = canon(topic, body)
        if c is DROP:
            continue
        if c is not KEEP:
            events += 1
            rewritten += c != body
            body = c
        frame = normalise.frame_of(topic, body)
        growth += max(0, len(frame) - (int(offs[i + 1]) - int(offs[i])))
        where.append(i)
        parts.append(frame)
    check(t.buf.numel(), t.n, growth)
    return HostParts(count, scatter(t, where, parts), parts, events, rewritten)


def emit_out(t: Tables, kept: int, kept_bytes: int, limit: int = LIMIT):
    """A new device buffer of exactly ``kept_bytes`` for the command's emit, which it launches only
    where ``kept`` is not 0. ``ValueError``, before anything is allocated, where ``kept`` and
    ``kept_bytes`` cannot be the totals of the scan over ``t.keep_len``; ``limit`` is the bound that
    ``kept_bytes`` stays below."""
    if not (0 <= kept <= t.n and 0 <= kept_bytes < limit and (kept == 0) == (kept_bytes == 0)):
        raise ValueError("kept and kept_bytes are the scan's totals")
    import torch
    return torch.empty(kept_bytes, dtype=torch.uint8, device=t.buf.device)


def splice(stream: np.ndarray, at: Sequence[int], parts: Sequence[bytes]) -> None:
    """Copies ``parts[k]`` into the uint8 ``stream`` at byte ``at[k]``, for every k."""
    for start, part in zip(at, parts):
        stream[start:start + len(part)] = np.frombuffer(part, dtype=np.uint8)


def collect(t: Tables, out, kept: int, host: HostParts) -> Tuple[bytes, List[int]]:
    """The output stream and its frames' indices (``t.base`` added), on the host, with the host's
    parts spliced into their spans: ``pos``'s low word at the host's frames says where."""
    import torch
    stream = out.cpu().numpy()
    if len(host.parts):
        at = (t.select.pos[torch.from_numpy(host.frames).to(out.device)] & 0xFFFFFFFF).cpu().numpy()
        splice(stream, at.tolist(), host.parts)
    indices = t.select.indices[:kept].cpu().numpy().astype(np.int64)
    return stream.tobytes(), (indices + t.base).tolist()
