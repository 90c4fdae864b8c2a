"""Drop the progress events that repeat their media's step on the GPU
(``ops/hip/telemetry_thin.hip``): the device path of ``python -m beholder_amd thin --device gpu``
(:mod:`beholder_amd.thin` defines the result).

The stages, which ``scripts/gpu_thin_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the host, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`classify` — one lane per frame sets the frame's kept length to its whole length and reads
   a topic-2 frame: a decode error is counted, a frame the device does not decide (the coalesce's
   rule for a progress frame: an id with a byte >= 0x80; in the upb dialect also a non-ASCII host and
   a start-group) goes to the overflow list, a progress event gets its row and its mark word,
   ``uint32(status) << 32 | uint32(progress // step)``. Other topics are not read.
3. ``gpu_transitions.claim``, ``rank``, ``counts``, ``compact`` and ``sort`` — the transitions'
   stages as they are: every event learns its media's dense number, and the events end up sorted
   stably by it, so a media's events are neighbours in stream order. A stream with no progress event
   that the device decides stops before ``compact``.
4. :func:`mark` — one lane per sorted position compares its mark word with its neighbour's, the
   next one under ``last`` and the previous one under ``first``, and stores a kept length of 0 where
   they are one media's and equal.
5. :func:`decide_on_host` — reads the counters; where the overflow list is not empty the host
   decodes those frames with ``thin.mark_of``. A media of host frames only is decided on the host
   alone. Where a media has host frames and device events (upb only: an ASCII id inside a frame with
   a group or a non-ASCII host), that media's run of the sorted events is read back, interleaved
   with the host's by frame index, the rule is applied to the whole run and the kept length of
   every frame in it is written again.
6. ``gpu_extract.scan``, ``totals`` and ``gather`` — the extract's prefix sum and copy, as they are,
   over this module's ``keep_len``; :func:`gpu_extract.collect` brings the bytes and indices back.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`thin`.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import gpu_extract, gpu_fold, gpu_transitions, hip_lib

C_PROGRESS_ERR, C_OVERFLOW, C_DROPPED, N_COUNTERS = 0, 1, 2, 3  # counters[] of telemetry_thin.hip
STEP_MAX = 2 ** 31 - 1
assert C_OVERFLOW == gpu_transitions.C_OVERFLOW


class Tables(NamedTuple):
    """The device tensors of one thin. ``t`` holds the transitions' tensors, for its claim, rank,
    compact and sort (``t.rows`` are progress events here, ``t.counters`` has ``N_COUNTERS`` words);
    ``select`` the extract's over ``keep_len``, for its scan and gather."""
    t: gpu_transitions.Tables
    marks: object     # n int64: the mark word of a progress event, else 0
    keep_len: object  # n int32: the frame's length where it is kept, else 0
    select: gpu_extract.ScanTables


def _check_policy(policy) -> None:
    from .. import thin
    if not isinstance(policy, thin.Policy):
        raise TypeError(f"policy is a thin.Policy, not {type(policy).__name__}")
    if isinstance(policy.step, bool) or not isinstance(policy.step, int) or not 1 <= policy.step <= STEP_MAX:
        raise ValueError(f"step is an int in 1..{STEP_MAX}")


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, zeroed where the kernels need it. Checks the
    arguments on the host."""
    import torch
    t = gpu_transitions.allocate(buf_dev, offs_dev, n)  # checks the tensors, n and the stream's size
    dev = buf_dev.device
    t = t._replace(counters=torch.zeros(N_COUNTERS, dtype=torch.int32, device=dev))
    keep_len = torch.empty(n, dtype=torch.int32, device=dev)
    return Tables(t, torch.empty(n, dtype=torch.int64, device=dev), keep_len,
                  gpu_extract.scan_tables(keep_len, n, buf_dev, offs_dev))


def classify(tb: Tables, policy, dialect: str = "protobufjs") -> None:
    """The classify launch over ``tb`` on the current torch stream. ``tb.t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``tb.t.counters`` must be zero."""
    _check_policy(policy)
    dialect_id = hip_lib.check_dialect(dialect)
    t = tb.t
    hip_lib.call("bh_thin_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id, policy.step,
                 t.rows.data_ptr(), t.is_event.data_ptr(), tb.marks.data_ptr(), tb.keep_len.data_ptr(),
                 t.counters.data_ptr(), t.overflow.data_ptr())


def mark(tb: Tables, s: gpu_transitions.Sorted, policy) -> None:
    """The mark launch over the sorted ``s``: stores 0 into ``tb.keep_len`` for every dropped event."""
    _check_policy(policy)
    if not 1 <= s.events <= tb.t.n:
        raise ValueError("the events are the scan's total, and there is at least one")
    hip_lib.call("bh_thin_mark", s.keys, s.keys.data_ptr(), s.vals.data_ptr(), s.events, tb.t.n,
                 int(policy.keep == "first"), tb.marks.data_ptr(), tb.keep_len.data_ptr(), tb.t.counters.data_ptr())


def _word(m: tuple) -> int:
    """The device's mark word of ``mark_of``'s ``(mediaId, status, bucket)``, as the int64 it is read back as."""
    w = ((m[1] & 0xFFFFFFFF) << 32) | (m[2] & 0xFFFFFFFF)
    return w - (1 << 64) if w >= 1 << 63 else w


def decide_on_host(tb: Tables, s: Optional[gpu_transitions.Sorted], data, offs: np.ndarray, policy,
                   dialect: str = "protobufjs") -> Tuple[int, int]:
    """Reads the counters; where the overflow list is not empty, decodes those frames with
    ``thin.mark_of``, decides every media that has one (with the device's events of that media,
    where it has any) and writes those frames' kept lengths into ``tb.keep_len``. ``s`` is None
    where the device sorted nothing. Returns ``(the list's length, the progress events among them)``."""
    import torch

    from .. import thin
    t = tb.t
    count = int(t.counters.cpu().numpy()[C_OVERFLOW])
    if count == 0:
        return 0, 0
    mark_of = thin.mark_of(policy, dialect)
    view = memoryview(data)
    per_media = {}  # id -> its (frame, mark word) pairs from the host's frames, in stream order
    for i, topic, body in hip_lib.overflow_frames(t.overflow, count, data, offs)[1]:
        m = mark_of(topic, body)
        if m is not None:
            per_media.setdefault(m[0], []).append((i, _word(m)))
    host_events = sum(map(len, per_media.values()))
    shared = {}  # id -> the device's (frame, mark word) pairs of that media
    if s is not None and any(mid.isascii() for mid in per_media):  # the device keeps ASCII ids only
        used = t.slot_scan.indices[:s.groups].long()  # the claimed slots by rank
        ids = t.rows[t.claim[used] - 1, 2:4].cpu().numpy().tolist()
        number = {bytes(view[off:off + length]): k for k, (off, length) in enumerate(ids)}
        keys = None
        for mid in per_media:
            k = number.get(mid.encode("ascii")) if mid.isascii() else None
            if k is None:
                continue
            if keys is None:
                keys = s.keys.cpu().numpy()
            start, end = int(np.searchsorted(keys, k, "left")), int(np.searchsorted(keys, k, "right"))
            theirs = (s.vals[start:end] >> 32).cpu().numpy()
            words = tb.marks[torch.from_numpy(theirs).to(tb.marks.device)].cpu().numpy()
            shared[mid] = list(zip(theirs.tolist(), words.tolist()))
    where, lengths = [], []
    for mid, mine in per_media.items():
        run = sorted(mine + shared.get(mid, []))
        for (i, _), gone in zip(run, thin.drops([w for _, w in run], policy.keep)):
            where.append(i)
            lengths.append(0 if gone else int(offs[i + 1]) - int(offs[i]))
    if where:
        dev = t.buf.device
        tb.keep_len[torch.tensor(where, dtype=torch.int64).to(dev)] = torch.tensor(lengths, dtype=torch.int32).to(dev)
    return count, host_events


def thin(data, policy, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None):
    """``(Thinned, frames decoded on the host)`` of a framed stream through the device."""
    from .. import thin as definition
    _check_policy(policy)
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "thin")
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    n, offs = gpu_fold.index(data)  # raises for a stream of 2^31 bytes or more
    if n == 0:
        return definition.Thinned(step=policy.step, keep=policy.keep, dialect=dialect), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    tb = allocate(buf, offs_dev, n)
    classify(tb, policy, dialect)
    gpu_transitions.claim(tb.t, hash_mask)
    gpu_transitions.rank(tb.t)
    groups, events = gpu_transitions.counts(tb.t)
    s = None
    if events:
        s = gpu_transitions.sort(gpu_transitions.compact(tb.t, groups, events))
        mark(tb, s, policy)
    host_frames, host_events = decide_on_host(tb, s, data, offs, policy, dialect)
    gpu_extract.scan(tb.select)
    kept, kept_bytes = gpu_extract.totals(tb.select)
    out = gpu_extract.gather(tb.select, kept, kept_bytes)
    out_bytes, indices = gpu_extract.collect(tb.select, out, kept)
    result = definition.Thinned(out_bytes, indices, n, policy.step, policy.keep, dialect, events + host_events)
    return result, host_frames
