"""Both topics of a framed telemetry stream joined per media, on the GPU
(``ops/hip/telemetry_stages.hip``): the device path of ``python -m beholder_amd stages --device gpu``
(:mod:`beholder_amd.stages` defines the result).

The stages, which ``scripts/gpu_stages_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the CPU, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`classify` — one lane per frame reads a topic-1 frame as the transitions do and a topic-2
   frame as the thin does: a decode error is counted under its topic, a frame the device does not
   decide (those two tools' rules) goes to the overflow list, an event of either topic gets its row
   and its ``aux`` word: the progress, and a bit for a status event. Other topics are not read.
3. ``gpu_transitions.claim``, ``rank``, ``counts``, ``compact`` and ``sort`` over the rows of both
   topics, unchanged: a media's events of both topics end up next to each other in stream order. A
   stream with no device event stops after ``counts``.
4. :func:`carry` — an inclusive scan with ``max`` over the sorted positions, of ``position + 1`` where
   the position holds a status event and of ``position + 1`` where it starts its media's run:
   ``stand[p]`` is the latest status position at or before ``p`` (``stood[p]`` its status) or -1,
   ``head[p]`` the first position of ``p``'s run. The scan runs over the whole array, not per media:
   a run is a contiguous range, so a status position at or after ``head[p]`` is the media's own, and
   one before it means that the media has none at or before ``p``. ``stand[p]`` is valid iff
   ``stand[p] >= head[p]``. The launch also gathers ``aux`` into sorted order.
5. :func:`settle` — one lane per sorted position adds to the three tables (summed per block in LDS),
   writes its media's row where it ends the lead or the run, and flags the lead events.
6. :func:`leads` — ``gpu_extract.scan`` over the lead flags, which sit where the kept lengths sit,
   compacts the lead positions; their ``(media number, status)`` come back and are counted on the
   CPU: O(lead events) there.
7. :func:`collect` and :func:`finish` — the tables, one row per media, the counters and the overflow
   list come back; strings come from the CPU's own copy of the stream. The CPU decodes the overflow
   frames with the service's codecs. A media that only the CPU holds goes through
   ``stages.course_of`` alone. Where one of their media is also the device's (upb: an ASCII id in a
   frame with a group or with a non-ASCII worker), that media's run of the sorted events is read
   back, its device contributions are taken out, and the whole run, interleaved by frame index, goes
   through ``stages.course_of`` and is added again.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`stages`.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import gpu_extract, gpu_fold, gpu_transitions, hip_lib
from .gpu_fold import ALL_ONES
from .gpu_transitions import CLASS_UNKNOWN, CLASSES

C_STATUS_ERR, C_OVERFLOW, C_PROGRESS_ERR, N_COUNTERS = 0, 1, 2, 3  # counters[] of telemetry_stages.hip
assert (C_STATUS_ERR, C_OVERFLOW) == (gpu_transitions.C_STATUS_ERR, gpu_transitions.C_OVERFLOW)
CARRY_BLOCK = 256  # BLOCK of telemetry_stages.hip: positions per block of the carry, totals per step of its totals scan
N_BUCKETS = 14     # telemetry_stages.hpp BUCKETS, in the order of stages.BUCKETS
T_MATRIX, T_ENTERED = 0, CLASSES * CLASSES  # the settle's tables, one after the other
T_CLOSED = T_ENTERED + CLASSES
T_WORDS = T_CLOSED + CLASSES * N_BUCKETS
M_START, M_END, M_LEAD, M_LEAD_LAST, M_OPEN, M_LAST, MEDIA_WORDS = 0, 1, 2, 3, 4, 5, 6  # telemetry_stages.hpp
AUX_STATUS = 1 << 32


class Tables(NamedTuple):
    """The device tensors of one run up to the sort: the transitions' (``t.rows`` are events of both
    topics here, ``t.counters`` has :data:`N_COUNTERS` words) and the per-frame ``aux`` words."""
    t: gpu_transitions.Tables
    aux: object  # n int64: the progress in the low half, AUX_STATUS for a status event


class Settled(NamedTuple):
    """What the launches after the sort write, next to a ``gpu_transitions.Sorted``."""
    saux: object        # events int64: aux in sorted order
    totals: object      # 2 * blocks int64, scratch of the carry
    base: object        # 2 * blocks int64, scratch of the carry
    stand: object       # events int32
    stood: object       # events int32
    head: object        # events int32
    tables: object      # T_WORDS int32: matrix, entered, closed
    media_rows: object  # (groups, MEDIA_WORDS) int32
    lead_scan: gpu_extract.ScanTables  # over the lead flags


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, zeroed where the kernels need it. Checks the
    arguments on the CPU."""
    import torch
    t = gpu_transitions.allocate(buf_dev, offs_dev, n)  # checks the tensors, n and the stream's size
    t = t._replace(counters=torch.zeros(N_COUNTERS, dtype=torch.int32, device=buf_dev.device))
    return Tables(t, torch.empty(n, dtype=torch.int64, device=buf_dev.device))


def classify(tb: Tables, dialect: str = "protobufjs") -> None:
    """The classify launch over ``tb`` on the current torch stream. ``tb.t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``tb.t.counters`` must be zero."""
    dialect_id = hip_lib.check_dialect(dialect)
    t = tb.t
    hip_lib.call("bh_stages_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id, t.rows.data_ptr(),
                 tb.aux.data_ptr(), t.is_event.data_ptr(), t.counters.data_ptr(), t.overflow.data_ptr())


def prepare(tb: Tables, s: gpu_transitions.Sorted) -> Settled:
    """The tensors of :func:`carry`, :func:`settle` and :func:`leads` next to the sorted ``s``, zeroed
    where the kernels need it."""
    import torch
    if not 1 <= s.groups <= s.events <= tb.t.n:
        raise ValueError("groups and events are the scans' totals, and there is at least one event")
    dev = s.keys.device
    blocks = (s.events + CARRY_BLOCK - 1) // CARRY_BLOCK

    def empty(size, dtype):
        return torch.empty(size, dtype=dtype, device=dev)
    lead_flag = empty(s.events, torch.int32)
    return Settled(empty(s.events, torch.int64), empty(2 * blocks, torch.int64), empty(2 * blocks, torch.int64),
                   empty(s.events, torch.int32), empty(s.events, torch.int32), empty(s.events, torch.int32),
                   torch.zeros(T_WORDS, dtype=torch.int32, device=dev),
                   torch.zeros((s.groups, MEDIA_WORDS), dtype=torch.int32, device=dev),
                   gpu_extract.scan_tables(lead_flag, s.events, tb.t.buf, tb.t.offs))


def carry(tb: Tables, s: gpu_transitions.Sorted, k: Settled) -> None:
    """The three carry launches over the sorted ``s``: ``k.saux``, ``k.stand``, ``k.stood`` and ``k.head``."""
    hip_lib.call("bh_stages_carry", s.keys, s.keys.data_ptr(), s.vals.data_ptr(), s.events, tb.t.n, tb.aux.data_ptr(),
                 k.saux.data_ptr(), k.totals.data_ptr(), k.base.data_ptr(), k.stand.data_ptr(), k.stood.data_ptr(),
                 k.head.data_ptr())


def settle(s: gpu_transitions.Sorted, k: Settled, mask: int) -> None:
    """The settle launch after :func:`carry`; ``mask`` is ``gpu_fold.known_mask`` of the enum.
    ``k.tables`` and ``k.media_rows`` must be zero."""
    if isinstance(mask, bool) or not isinstance(mask, int) or not 0 <= mask <= ALL_ONES:
        raise ValueError("the status mask is 64-bit")
    hip_lib.call("bh_stages_settle", s.keys, s.keys.data_ptr(), s.vals.data_ptr(), k.saux.data_ptr(),
                 k.stand.data_ptr(), k.stood.data_ptr(), k.head.data_ptr(), s.events, s.groups, mask,
                 k.tables.data_ptr(), k.media_rows.data_ptr(), k.lead_scan.keep_len.data_ptr())


def leads(s: gpu_transitions.Sorted, k: Settled) -> np.ndarray:
    """``(lead events, 2)`` int64 after :func:`settle`: the media number and the raw status of every
    lead event, from the extract's scan over the lead flags."""
    gpu_extract.scan(k.lead_scan)
    count = gpu_extract.totals(k.lead_scan)[0]
    if count == 0:
        return np.zeros((0, 2), dtype=np.int64)
    at = k.lead_scan.indices[:count].long()
    status = s.vals[at].cpu().numpy().astype(np.uint32).astype(np.int32)  # the low half, signed
    return np.stack((s.keys[at].cpu().numpy().astype(np.int64), status.astype(np.int64)), axis=-1)


class Collected(NamedTuple):
    """What crosses back to the CPU: O(classes^2 + media + lead events + overflow)."""
    counters: np.ndarray    # N_COUNTERS
    overflow: object        # the frame indices left to the CPU, as the device listed them
    tables: np.ndarray      # T_WORDS int64
    id_span: np.ndarray     # (groups, 2): offset and length of every media's id in the stream
    media_rows: np.ndarray  # (groups, MEDIA_WORDS)
    opened: np.ndarray      # groups int64: frame << 32 | status of the open stage's status event (0 where none)
    leads: np.ndarray       # (lead events, 2) int64: media number, raw status


def collect(tb: Tables, s: Optional[gpu_transitions.Sorted], k: Optional[Settled],
            lead_rows: Optional[np.ndarray] = None) -> Collected:
    """``s``, ``k`` and ``lead_rows`` (:func:`leads`) are None where the stream has no event that the
    device decided."""
    t = tb.t
    counters = t.counters.cpu().numpy()
    overflow = t.overflow[:int(counters[C_OVERFLOW])].cpu()
    if s is None:
        none = np.zeros((0, 2), dtype=np.int64)
        return Collected(counters, overflow, np.zeros(T_WORDS, dtype=np.int64), none,
                         np.zeros((0, MEDIA_WORDS), dtype=np.int64), none[:, 0], none)
    used = t.slot_scan.indices[:s.groups].long()  # the claimed slots by rank
    spans = t.rows[t.claim[used] - 1, 2:4].cpu().numpy()
    opened = s.vals[(k.media_rows[:, M_OPEN].long() - 1).clamp(min=0)]
    return Collected(counters, overflow, k.tables.cpu().numpy().astype(np.int64), spans, k.media_rows.cpu().numpy(),
                     opened.cpu().numpy(), lead_rows)


def _signed(word: int) -> int:
    status = word & 0xFFFFFFFF
    return status - (1 << 32) if status >= 1 << 31 else status


def _run(s: gpu_transitions.Sorted, k: Settled, start: int, end: int) -> list:
    """One media's ``(frame, kind, status, progress)`` events in stream order: a slice of the sorted events."""
    from ..stages import PROGRESS, STATUS
    words = s.vals[start:end].cpu().numpy().tolist()
    aux = k.saux[start:end].cpu().numpy().tolist()
    return [(v >> 32, STATUS if a & AUX_STATUS else PROGRESS, _signed(v), _signed(a)) for v, a in zip(words, aux)]


def _class(cls: int):
    from ..stages import UNKNOWN
    return UNKNOWN if cls == CLASS_UNKNOWN else cls


def finish(data, offs: np.ndarray, n: int, c: Collected, s: Optional[gpu_transitions.Sorted], k: Optional[Settled],
           dialect: str = "protobufjs"):
    """The :class:`~beholder_amd.stages.StageReport` from the device's columns and the CPU's own copy
    of the stream; the frames in ``c.overflow`` are decoded here with the service's codecs."""
    from .. import replay, stages as definition
    names = replay.status_names()
    report = definition.StageReport(frames=n, status_decode_errors=int(c.counters[C_STATUS_ERR]),
                                    progress_decode_errors=int(c.counters[C_PROGRESS_ERR]))
    matrix = c.tables[T_MATRIX:T_ENTERED].reshape(CLASSES, CLASSES)
    for a, b in zip(*np.nonzero(matrix)):
        report.matrix[(_class(int(a)), _class(int(b)))] = int(matrix[a, b])
    entered = c.tables[T_ENTERED:T_CLOSED]
    for a in np.nonzero(entered)[0]:
        report.entered[_class(int(a))] = int(entered[a])
    closed = c.tables[T_CLOSED:T_WORDS].reshape(CLASSES, N_BUCKETS)
    for a, b in zip(*np.nonzero(closed)):
        report.closed[(_class(int(a)), definition.BUCKETS[b])] = int(closed[a, b])
    report.status_events = int(entered.sum())
    view = memoryview(data)
    ids = [str(view[int(off):int(off) + int(length)], "ascii") for off, length in c.id_span]  # ASCII ids only
    lead_of = [{} for _ in ids]
    if len(c.leads):  # O(lead events) on the CPU
        cells, counts_of = np.unique(c.leads, axis=0, return_counts=True)
        for (media, status), count in zip(cells.tolist(), counts_of.tolist()):
            cls = definition.class_of(status, names)
            lead_of[media][cls] = lead_of[media].get(cls, 0) + count
    for mid, row, opened, lead in zip(ids, c.media_rows.tolist(), c.opened.tolist(), lead_of):
        events = row[M_END] - row[M_START]
        stage = None
        if row[M_OPEN]:
            count = row[M_END] - row[M_OPEN]  # the positions after the status event at M_OPEN - 1
            stage = (opened >> 32, _signed(opened), count, row[M_LAST] if count else None)
        report.media[mid] = definition.MediaStand(lead, row[M_LEAD_LAST] if row[M_LEAD] else None, events, stage)
        report.progress_events += events
    report.progress_events -= report.status_events
    if len(c.overflow):
        frames = hip_lib.overflow_frames(c.overflow, len(c.overflow), data, offs)[1]
        per_media, status_errors, progress_errors = definition.events_of(frames, dialect)
        report.status_decode_errors += status_errors
        report.progress_decode_errors += progress_errors
        number = {mid: i for i, mid in enumerate(ids)}
        for mid, mine in per_media.items():
            i = number.get(mid)
            if i is not None:  # the device holds events of this media too
                theirs = _run(s, k, int(c.media_rows[i, M_START]), int(c.media_rows[i, M_END]))
                report.add_course(mid, definition.course_of(theirs, names), sign=-1)
                mine = sorted(theirs + mine)
            report.add_course(mid, definition.course_of(mine, names))
    return report


def stages(data, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None):
    """``(StageReport, frames decoded on the CPU)`` of a framed stream through the device."""
    from .. import replay, stages as definition
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "stages")
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    n, offs = gpu_fold.index(data)  # raises for a stream of 2^31 bytes or more
    if n == 0:
        return definition.StageReport(), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    tb = allocate(buf, offs_dev, n)
    classify(tb, dialect)
    gpu_transitions.claim(tb.t, hash_mask)
    gpu_transitions.rank(tb.t)
    groups, events = gpu_transitions.counts(tb.t)
    s = k = lead_rows = None
    if events:
        s = gpu_transitions.sort(gpu_transitions.compact(tb.t, groups, events))
        k = prepare(tb, s)
        carry(tb, s, k)
        settle(s, k, gpu_fold.known_mask(replay.status_names()))
        lead_rows = leads(s, k)
    c = collect(tb, s, k, lead_rows)
    return finish(data, offs, n, c, s, k, dialect), len(c.overflow)
