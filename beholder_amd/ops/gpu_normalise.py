"""Rewrite a framed telemetry stream's events in canonical form on the GPU
(``ops/hip/telemetry_normalise.hip``): the device path of ``python -m beholder_amd normalise --device
gpu`` (:mod:`beholder_amd.normalise` defines the result).

The stages, which ``scripts/gpu_normalise_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the host, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`classify` — one lane per frame reads the frame by its topic and stores its plan (spans,
   numbers, a kind) and the length of its output frame: the canonical length of a decoded event, the
   input length of a frame that stays, 0 for a dropped one. A frame the device does not write (a
   decoded id or host with a byte >= 0x80 in either dialect; in the upb dialect also a start-group)
   goes to the overflow list with length 0.
3. :func:`decide_on_host` — reads the counters; where the overflow list is not empty the host asks
   ``normalise.canon_of`` about those frames, keeps their output bytes and scatters their lengths
   into ``keep_len`` before the scan.
4. ``gpu_extract.scan`` and ``totals`` — the extract's prefix sum, as it is, over this module's
   ``keep_len``: every output frame's offset, and the one word that sizes the output.
5. :func:`emit` — a wave per 64 frames writes the planned frames' bytes at their offsets, and counts
   the events whose bytes changed. It writes nothing into the spans of host frames.
6. :func:`collect` — the output and the indices come back, and the host splices its frames' bytes
   into their spans.

The tables, the scatter, the emit's front and the splice are the rewriting commands' own
(``ops/gpu_rewrite.py``), shared with the anonymise, the export and the import.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`normalise`.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from . import gpu_extract, gpu_fold, gpu_rewrite, hip_lib
from .gpu_rewrite import LIMIT, HostParts, Tables  # noqa: F401  the shared shapes, under the names the callers know

C_EVENTS, C_ERRORS, C_OTHER, C_OVERFLOW, C_REWRITTEN, N_COUNTERS = 0, 1, 2, 3, 4, 5  # counters[] of the kernels
NM_COPY, NM_DROP, NM_HOST, NM_STATUS, NM_PROGRESS = 0, 1, 2, 3, 4  # Plan::kind of telemetry_normalise.hpp
PLAN_FIELDS = ("id_off", "id_len", "status", "progress", "host_off", "host_len", "kind", "out_len")
NM_GROWTH_MAX = 10  # telemetry_normalise.hpp, with its derivation


class TooLarge(ValueError):
    """The stream, grown by what normalising can add, does not stay below 2^31 bytes."""


def _check_policy(policy) -> None:
    from .. import normalise
    if not isinstance(policy, normalise.Policy):
        raise TypeError(f"policy is a normalise.Policy, not {type(policy).__name__}")
    gpu_rewrite.check_undecoded(policy)


def check_size(size: int, n: int, extra: int = 0) -> None:
    """:class:`TooLarge` where ``size`` bytes in ``n`` frames could normalise to 2^31 bytes or more;
    ``extra`` is what the host's frames add beyond the device's bound."""
    if size + NM_GROWTH_MAX * n + extra >= LIMIT:
        raise TooLarge(f"a stream of {size} bytes in {n} frames can grow past the 2^31 bytes that the device's "
                       "offsets reach")


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, zeroed where the kernels need it. Checks the
    arguments on the host."""
    return gpu_rewrite.allocate(buf_dev, offs_dev, n, len(PLAN_FIELDS), N_COUNTERS, "the normalise",
                                lambda: check_size(buf_dev.numel(), n))


def classify(t: Tables, policy, dialect: str = "protobufjs") -> None:
    """The classify launch over ``t`` on the current torch stream. ``t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``t.counters`` must be zero."""
    _check_policy(policy)
    dialect_id = hip_lib.check_dialect(dialect)
    hip_lib.call("bh_normalise_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id,
                 int(policy.undecoded == "drop"), t.plans.data_ptr(), t.keep_len.data_ptr(), t.counters.data_ptr(),
                 t.overflow.data_ptr())


def decide_on_host(t: Tables, data, offs: np.ndarray, policy, dialect: str = "protobufjs") -> HostParts:
    """Reads the overflow list's length; where it is not 0, asks ``normalise.canon_of`` about those
    frames and writes the lengths of their output frames into ``t.keep_len``. Raises
    :class:`TooLarge` where they grow the output past what the scan's 32 bits hold."""
    from .. import normalise
    return gpu_rewrite.decide_with(t, C_OVERFLOW, data, offs, lambda: normalise.canon_of(policy, dialect), check_size)


def emit(t: Tables, kept: int, kept_bytes: int):
    """The output in a new device buffer of exactly ``kept_bytes``, the host frames' spans left as
    they are. ``kept`` and ``kept_bytes`` must be the totals of the scan over ``t.keep_len``: the
    kernel trusts them. No frame in the output launches nothing."""
    out = gpu_rewrite.emit_out(t, kept, kept_bytes)
    if kept:
        hip_lib.call("bh_normalise_emit", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, t.plans.data_ptr(),
                     t.select.pos.data_ptr(), out.data_ptr(), t.counters.data_ptr())
    return out


def collect(t: Tables, out, kept: int, host: HostParts) -> Tuple[bytes, List[int]]:
    """The output stream and its frames' input indices, on the host, with the host's frames spliced
    into their spans: ``gpu_extract.collect`` where there are none."""
    if not host.parts:
        return gpu_extract.collect(t.select, out, kept)
    return gpu_rewrite.collect(t, out, kept, host)


def normalise(data, policy, device="cuda", dialect: str = "protobufjs"):
    """``(Normalised, frames decided on the host)`` of a framed stream through the device."""
    from .. import normalise as definition
    _check_policy(policy)
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "normalise")
    n, offs = gpu_fold.index(data)  # raises for a stream of 2^31 bytes or more
    if n == 0:
        return definition.Normalised(dialect=dialect, undecoded=policy.undecoded), 0
    check_size(len(data), n)
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    t = allocate(buf, offs_dev, n)
    classify(t, policy, dialect)
    host = decide_on_host(t, data, offs, policy, dialect)
    gpu_extract.scan(t.select)
    kept, kept_bytes = gpu_extract.totals(t.select)
    out = emit(t, kept, kept_bytes)
    out_bytes, indices = collect(t, out, kept, host)
    counters = t.counters.cpu().numpy().tolist()
    result = definition.Normalised(out_bytes, indices, n, counters[C_EVENTS] + host.events,
                                   counters[C_REWRITTEN] + host.rewritten, dialect, policy.undecoded)
    return result, host.count
