"""Replace a framed telemetry stream's media ids and host names by keyed pseudonyms on the GPU
(``ops/hip/telemetry_anonymise.hip``): the device path of ``python -m beholder_amd anonymise --device
gpu`` (:mod:`beholder_amd.anonymise` defines the result).

The stages are the normalise's (``ops/gpu_normalise.py``), over the tables and host stages that the
rewriting commands share (``ops/gpu_rewrite.py``); ``scripts/gpu_anonymise_probe.py`` times them one
by one next to the normalise's:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold.
2. :func:`classify` — one lane per frame reads the frame as the normalise does, hashes the chosen
   strings (keyed BLAKE2s, from the two states after the key block, which the launcher computes on
   the host: the key does not go to the device) and stores its plan and the length of its output
   frame. A frame the device does not write (the normalise's rule, or a chosen string above 4,096
   bytes) goes to the overflow list with length 0.
3. :func:`decide_on_host` — ``gpu_rewrite.decide_with``, as the normalise's, with ``anonymise.anon_of``
   in place of ``canon_of``.
4. ``gpu_extract.scan`` and ``totals`` — the extract's prefix sum, as it is, over ``keep_len``.
5. :func:`emit` — a wave per 64 frames writes the planned frames' bytes at their offsets; a digit of
   a pseudonym comes from the plan's digest words. It writes nothing into the spans of host frames.
6. :func:`collect` — the normalise's: the output and the indices come back, and the host splices its
   frames' bytes into their spans.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`anonymise`.
"""
from __future__ import annotations

import numpy as np

from . import gpu_extract, gpu_fold, gpu_normalise, gpu_rewrite, hip_lib
from .gpu_normalise import TooLarge, collect  # noqa: F401  collect: stage 6, as it is
from .gpu_rewrite import LIMIT, HostParts, Tables  # noqa: F401  the shared shapes, under the names the callers know

C_EVENTS, C_ERRORS, C_OTHER, C_OVERFLOW, N_COUNTERS = 0, 1, 2, 3, 4  # counters[] of the kernels
PLAN_FIELDS = gpu_normalise.PLAN_FIELDS + tuple(f"{s}_digest{k}" for s in ("id", "host") for k in range(4))
FIELD_BITS = {"mediaId": 1, "host": 2}  # AN_MEDIA, AN_HOST of telemetry_anonymise.hpp
AN_GROWTH_MAX = 72    # telemetry_anonymise.hpp, with its derivation
AN_STRING_MAX = 4096  # a longer chosen string goes to the host


def _check_policy(policy) -> None:
    from .. import anonymise
    if not isinstance(policy, anonymise.Policy):
        raise TypeError(f"policy is an anonymise.Policy, not {type(policy).__name__}")
    gpu_rewrite.check_undecoded(policy)
    if not policy.fields or not set(policy.fields) <= set(FIELD_BITS):
        raise ValueError("fields is a non-empty subset of mediaId and host")
    if not isinstance(policy.key, bytes) or not 16 <= len(policy.key) <= 32:
        raise ValueError("key has 16 to 32 bytes")


def check_size(size: int, n: int, extra: int = 0) -> None:
    """:class:`TooLarge` where ``size`` bytes in ``n`` frames could anonymise to 2^31 bytes or more;
    ``extra`` is what the host's frames add beyond the device's bound."""
    if size + AN_GROWTH_MAX * n + extra >= LIMIT:
        raise TooLarge(f"a stream of {size} bytes in {n} frames can grow past the 2^31 bytes that the device's "
                       "offsets reach")


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, zeroed where the kernels need it. Checks the
    arguments on the host."""
    return gpu_rewrite.allocate(buf_dev, offs_dev, n, len(PLAN_FIELDS), N_COUNTERS, "the anonymise",
                                lambda: check_size(buf_dev.numel(), n))


def classify(t: Tables, policy, dialect: str = "protobufjs") -> None:
    """The classify launch over ``t`` on the current torch stream. ``t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``t.counters`` must be zero. The key is read on the
    host, by the launcher."""
    _check_policy(policy)
    dialect_id = hip_lib.check_dialect(dialect)
    fields = sum(FIELD_BITS[f] for f in policy.fields)
    hip_lib.call("bh_anonymise_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id,
                 int(policy.undecoded == "drop"), fields, policy.key, len(policy.key), t.plans.data_ptr(),
                 t.keep_len.data_ptr(), t.counters.data_ptr(), t.overflow.data_ptr())


def decide_on_host(t: Tables, data, offs: np.ndarray, policy, dialect: str = "protobufjs") -> HostParts:
    """Reads the overflow list's length; where it is not 0, asks ``anonymise.anon_of`` about those
    frames and writes the lengths of their output frames into ``t.keep_len``. Raises
    :class:`TooLarge` where they grow the output past what the scan's 32 bits hold."""
    from .. import anonymise
    return gpu_rewrite.decide_with(t, C_OVERFLOW, data, offs, lambda: anonymise.anon_of(policy, dialect), check_size)


def emit(t: Tables, kept: int, kept_bytes: int):
    """The output in a new device buffer of exactly ``kept_bytes``, the host frames' spans left as
    they are. ``kept`` and ``kept_bytes`` must be the totals of the scan over ``t.keep_len``: the
    kernel trusts them. No frame in the output launches nothing."""
    out = gpu_rewrite.emit_out(t, kept, kept_bytes)
    if kept:
        hip_lib.call("bh_anonymise_emit", t.buf, t.buf.data_ptr(), t.n, t.plans.data_ptr(), t.select.pos.data_ptr(),
                     out.data_ptr())
    return out


def anonymise(data, policy, device="cuda", dialect: str = "protobufjs"):
    """``(Anonymised, frames decided on the host)`` of a framed stream through the device."""
    from .. import anonymise as definition
    _check_policy(policy)
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "anonymise")
    n, offs = gpu_fold.index(data)  # raises for a stream of 2^31 bytes or more
    if n == 0:
        return definition.result_for(policy, dialect), 0
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
    events = int(t.counters[C_EVENTS].item()) + host.events
    return definition.result_for(policy, dialect, out_bytes, indices, n, events), host.count
