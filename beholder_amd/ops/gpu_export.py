"""Write a framed telemetry stream as NDJSON rows on the GPU (``ops/hip/telemetry_export.hip``): the
device path of ``python -m beholder_amd export --device gpu`` (:mod:`beholder_amd.export` defines the
result).

The stages, which ``scripts/gpu_export_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the host, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`classify` — one lane per frame reads the frame by its topic and stores its plan (spans,
   numbers, the strings' escaped lengths, a kind) and the exact length of its row, 0 for a dropped
   frame. A frame the device does not write (a decoded id or host with a byte >= 0x80 in either
   dialect; in the upb dialect also a start-group) goes to the overflow list with length 0.
3. :func:`decide_on_host` — reads the counters; where the overflow list is not empty the host asks
   ``export.decoded_row_of`` about those frames, keeps their rows and scatters their lengths into
   ``keep_len`` before the scan.
4. :func:`out_bytes` — the exact size of the output, a reduction over ``keep_len`` in 64 bits:
   :class:`TooLarge` where it reaches 2^31, before the scan and any emit.
5. ``gpu_extract.scan`` and ``totals`` — the extract's prefix sum, as it is, over this module's
   ``keep_len``: every row's offset, and the one word that sizes the output.
6. :func:`emit` — a wave per 64 frames writes the planned rows' bytes at their offsets. It writes
   nothing into the spans of host frames.
7. :func:`collect` — the output and the indices come back, and the host splices its rows into their
   spans.

The tables, the scatter, the emit's front and :func:`collect` are the rewriting commands' own
(``ops/gpu_rewrite.py``), shared with the normalise, the anonymise and the import.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`export`.
"""
from __future__ import annotations

import numpy as np

from . import gpu_extract, gpu_fold, gpu_rewrite, hip_lib
from .gpu_rewrite import LIMIT, HostParts, Tables, collect  # noqa: F401  collect: stage 7, as it is

C_EVENTS, C_ERRORS, C_OTHER, C_TOO_LONG, C_OVERFLOW, N_COUNTERS = 0, 1, 2, 3, 4, 5  # counters[] of the kernels
EX_B64, EX_DROP, EX_HOST, EX_STATUS, EX_PROGRESS, EX_TOO_LONG = 0, 1, 2, 3, 4, 5  # RowPlan::kind of telemetry_export.hpp
PLAN_FIELDS = ("id_off", "id_len", "status", "progress", "host_off", "host_len", "id_esc", "host_esc", "kind", "topic",
               "row_len", "reserved")


class TooLarge(ValueError):
    """The rows of the stream do not stay below 2^31 bytes."""


def _check_policy(policy) -> None:
    from .. import export
    if not isinstance(policy, export.Policy):
        raise TypeError(f"policy is an export.Policy, not {type(policy).__name__}")
    gpu_rewrite.check_undecoded(policy)


def _check_base(base) -> None:
    from .. import export
    export._check_base(base)


def _too_large(size: int) -> TooLarge:
    return TooLarge(f"the rows take {size} bytes or more, past the 2^31 bytes that the device's offsets reach")


def allocate(buf_dev, offs_dev, n: int, base: int = 0) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, zeroed where the kernels need it. Checks the
    arguments on the host."""
    return gpu_rewrite.allocate(buf_dev, offs_dev, n, len(PLAN_FIELDS), N_COUNTERS, "the export",
                                lambda: _check_base(base), base)


def classify(t: Tables, policy, dialect: str = "protobufjs") -> None:
    """The classify launch over ``t`` on the current torch stream. ``t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``t.counters`` must be zero."""
    _check_policy(policy)
    dialect_id = hip_lib.check_dialect(dialect)
    hip_lib.call("bh_export_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id,
                 int(policy.undecoded == "drop"), t.base, t.plans.data_ptr(), t.keep_len.data_ptr(),
                 t.counters.data_ptr(), t.overflow.data_ptr())


def decide_on_host(t: Tables, data, offs: np.ndarray, policy, dialect: str = "protobufjs") -> HostParts:
    """Reads the counters. :class:`TooLarge` where one row alone reaches 2^31 bytes. Where the
    overflow list is not empty, asks ``export.decoded_row_of`` about those frames and writes the
    lengths of their rows into ``t.keep_len``."""
    from .. import export
    from ..coalesce import DROP
    counters = t.counters.cpu().numpy().tolist()
    if counters[C_TOO_LONG]:
        raise _too_large(LIMIT)
    count = counters[C_OVERFLOW]
    if count == 0:
        return gpu_rewrite.NO_HOST_PARTS
    row = export.decoded_row_of(policy, dialect)
    where, parts = [], []
    events = 0
    for i, topic, body in hip_lib.overflow_frames(t.overflow, count, data, offs)[1]:
        r, decoded = row(t.base + i, topic, body)
        events += decoded
        if r is DROP:
            continue
        if len(r) >= LIMIT:
            raise _too_large(len(r))
        where.append(i)
        parts.append(r)
    return HostParts(count, gpu_rewrite.scatter(t, where, parts), parts, events)


def keep_len_sum(t: Tables) -> int:
    """The sum of ``t.keep_len`` in 64 bits: one reduction on the device, one word read back."""
    import torch
    return int(t.keep_len.sum(dtype=torch.int64).item())


def out_bytes(t: Tables) -> int:
    """The exact size of the output, host rows included; :class:`TooLarge` where it reaches 2^31
    bytes, which the scan's 32 bits do not hold. Comes after :func:`decide_on_host` and before the
    scan."""
    size = keep_len_sum(t)
    if size >= LIMIT:
        raise _too_large(size)
    return size


def emit(t: Tables, kept: int, kept_bytes: int):
    """The output in a new device buffer of exactly ``kept_bytes``, the host rows' spans left as they
    are. ``kept`` and ``kept_bytes`` must be the totals of the scan over ``t.keep_len``: the kernel
    trusts them. No row in the output launches nothing."""
    out = gpu_rewrite.emit_out(t, kept, kept_bytes)
    if kept:
        hip_lib.call("bh_export_emit", t.buf, t.buf.data_ptr(), t.n, t.base, t.plans.data_ptr(),
                     t.select.pos.data_ptr(), out.data_ptr())
    return out


def export(data, policy, device="cuda", dialect: str = "protobufjs", base: int = 0):
    """``(Exported, frames decided on the host)`` of a framed stream through the device."""
    from .. import export as definition
    _check_policy(policy)
    hip_lib.check_dialect(dialect)
    _check_base(base)
    hip_lib.require_gpu(device, "export")
    n, offs = gpu_fold.index(data)  # raises for a stream of 2^31 bytes or more
    if n == 0:
        return definition.Exported(base=base, dialect=dialect, undecoded=policy.undecoded), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    t = allocate(buf, offs_dev, n, base)
    classify(t, policy, dialect)
    host = decide_on_host(t, data, offs, policy, dialect)
    size = out_bytes(t)
    gpu_extract.scan(t.select)
    kept, kept_bytes = gpu_extract.totals(t.select)
    if kept_bytes != size:
        raise RuntimeError(f"the scan places {kept_bytes} bytes where keep_len sums to {size}")
    out = emit(t, kept, kept_bytes)
    rows, indices = collect(t, out, kept, host)
    events = int(t.counters[C_EVENTS].item()) + host.events
    return definition.Exported(rows, indices, n, events, base, dialect, policy.undecoded), host.count
