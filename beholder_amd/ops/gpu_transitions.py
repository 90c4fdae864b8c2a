"""The status moves of every media of a framed telemetry stream on the GPU
(``ops/hip/telemetry_transitions.hip``): the device path of ``python -m beholder_amd transitions
--device gpu`` (:mod:`beholder_amd.transitions` defines the result).

The stages, which ``scripts/gpu_transitions_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the host, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`classify` — one lane per frame reads a topic-1 frame: a decode error is counted, a frame the
   device does not decide (the fold's rule: an id with a byte >= 0x80; in the upb dialect a
   start-group) goes to the overflow list, a status event gets its row. Other topics are not read.
3. :func:`claim` — the fold's open-addressing table: every status event learns its media's slot.
4. :func:`rank` — the extract's scan over the table (``gpu_extract.scan``, as it is): a claimed slot's
   rank is its dense media number. The same scan over the events gives their frames in stream
   order. :func:`counts` reads back the two words ``(groups, events)``; ``groups`` decides the
   number of sort passes.
5. :func:`compact` — per status event, in stream order: its media number and ``frame << 32 | status``.
6. :func:`sort` — a stable radix sort by media number, 8 bits per pass, :func:`sort_passes` passes:
   none for one media, at most 4.
7. :func:`pairs` — one lane per sorted position counts the move from its predecessor where that is
   the same media, and writes the media's first and last event and its run's bounds.
8. :func:`collect` and :func:`finish` — the matrix, the counters, one row per media and the overflow
   list come back; id strings come from the host's own copy of the stream. The host decodes the
   overflow frames with the service's codec. Where one of their media is also the device's (upb
   only: an ASCII id inside a frame with a group), that media's run of the sorted events is read
   back, interleaved with the host's by frame index, and the media's row and cells are recomputed.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`transitions`.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import gpu_extract, gpu_fold, hip_lib
from .gpu_fold import ALL_ONES

SORT_TILE = 256    # BLOCK of telemetry_transitions.hip: elements a block of the sort ranks at a time
SORT_BLOCK = 2048  # BLOCK * TILES: elements per block of the sort and of pairs
RADIX_BITS = 8
CLASSES, CLASS_UNKNOWN = 65, 64  # telemetry_transitions.hpp
C_STATUS_ERR, C_OVERFLOW, N_COUNTERS = 0, 1, 2  # counters[] of telemetry_transitions.hip
STAGE_COUNT, STAGE_TOTALS, STAGE_APPLY, ALL_STAGES = 1, 2, 4, 7
MAX_SLOTS = 1 << 30  # the slot scan counts the slots in an int


def sort_passes(groups: int) -> int:
    """Passes that order media numbers below ``groups``: ``ceil(bit_length(groups - 1) / 8)``."""
    return (max(groups - 1, 0).bit_length() + RADIX_BITS - 1) // RADIX_BITS


class Tables(NamedTuple):
    """The device tensors of one run up to the two scans. ``slot_scan`` and ``event_scan`` hold the
    extract's tensors for ``gpu_extract.scan``: over ``slot_used`` and over ``is_event``."""
    n: int
    slots: int
    buf: object
    offs: object
    rows: object       # (n, 6) int32: hash lo, hash hi, id_off, id_len, status, kind
    is_event: object   # n int32
    counters: object   # N_COUNTERS int32
    overflow: object   # n int32
    claim: object      # slots int64: 0 or 1 + the frame that claimed the slot
    slot_used: object  # slots int32
    slot_of: object    # n int32
    slot_scan: gpu_extract.ScanTables
    event_scan: gpu_extract.ScanTables


class Sorted(NamedTuple):
    """The status events by media, and what :func:`pairs` makes of them."""
    events: int
    groups: int
    keys: object       # events int32: the media number
    vals: object       # events int64: frame << 32 | status
    matrix: object     # CLASSES * CLASSES int32
    first: object      # groups int64
    last: object       # groups int64
    run_start: object  # groups int32
    run_end: object    # groups int32
    changes: object    # groups int32


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, zeroed where the kernels need it. Checks the
    arguments on the host."""
    import torch
    hip_lib.check_stream(buf_dev, offs_dev, n, "transitions")
    slots = gpu_fold.table_slots(n)
    if slots > MAX_SLOTS:
        raise ValueError("the media table is too large for int32 indexing: cut the stream into chunks")
    dev = buf_dev.device
    is_event = torch.empty(n, dtype=torch.int32, device=dev)
    slot_used = torch.zeros(slots, dtype=torch.int32, device=dev)
    return Tables(n, slots, buf_dev, offs_dev,
                  torch.empty((n, 6), dtype=torch.int32, device=dev), is_event,
                  torch.zeros(N_COUNTERS, dtype=torch.int32, device=dev),
                  torch.empty(n, dtype=torch.int32, device=dev),
                  torch.zeros(slots, dtype=torch.int64, device=dev), slot_used,
                  torch.empty(n, dtype=torch.int32, device=dev),
                  gpu_extract.scan_tables(slot_used, slots, buf_dev, offs_dev),
                  gpu_extract.scan_tables(is_event, n, buf_dev, offs_dev))


def classify(t: Tables, dialect: str = "protobufjs") -> None:
    """The classify launch over ``t`` on the current torch stream. ``t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``t.counters`` must be zero."""
    dialect_id = hip_lib.check_dialect(dialect)
    hip_lib.call("bh_transitions_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id,
                 t.rows.data_ptr(), t.is_event.data_ptr(), t.counters.data_ptr(), t.overflow.data_ptr())


def claim(t: Tables, hash_mask: int = ALL_ONES) -> None:
    """The claim launch over the rows of :func:`classify`. ``t.claim`` and ``t.slot_used`` must be zero."""
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    hip_lib.call("bh_transitions_claim", t.buf, t.buf.data_ptr(), t.rows.data_ptr(), t.n, hash_mask,
                 t.claim.data_ptr(), t.slot_used.data_ptr(), t.slot_of.data_ptr(), t.slots)


def rank(t: Tables) -> None:
    """The two prefix sums, the extract's launches as they are: over the table's slots and over the
    frames' event flags."""
    gpu_extract.scan(t.slot_scan)
    gpu_extract.scan(t.event_scan)


def counts(t: Tables) -> Tuple[int, int]:
    """``(groups, events)`` after :func:`rank`: the two words the host reads before it sorts."""
    import torch
    words = torch.stack((t.slot_scan.base[-1], t.event_scan.base[-1])).cpu().numpy() >> 32
    return int(words[0]), int(words[1])


def compact(t: Tables, groups: int, events: int) -> Sorted:
    """The status events in stream order as ``(media number, frame << 32 | status)``, and the zeroed
    outputs of :func:`pairs`. ``groups`` and ``events`` must be :func:`counts`'s."""
    import torch
    if not (1 <= groups <= events <= t.n):
        raise ValueError("groups and events are the scans' totals, and there is at least one event")
    dev = t.buf.device

    def empty(size, dtype):
        return torch.empty(size, dtype=dtype, device=dev)
    s = Sorted(events, groups, empty(events, torch.int32), empty(events, torch.int64),
               torch.zeros(CLASSES * CLASSES, dtype=torch.int32, device=dev), empty(groups, torch.int64),
               empty(groups, torch.int64), empty(groups, torch.int32), empty(groups, torch.int32),
               torch.zeros(groups, dtype=torch.int32, device=dev))
    hip_lib.call("bh_transitions_compact", t.buf, t.rows.data_ptr(), t.event_scan.indices.data_ptr(),
                 t.slot_of.data_ptr(), t.slot_scan.pos.data_ptr(), events, s.keys.data_ptr(), s.vals.data_ptr())
    return s


def sort_scratch(s: Sorted):
    """``(keys, vals, totals, base)`` that :func:`sort_pass` needs next to ``s``."""
    import torch
    blocks = (s.events + SORT_BLOCK - 1) // SORT_BLOCK
    dev = s.keys.device
    return (torch.empty_like(s.keys), torch.empty_like(s.vals),
            torch.empty(256 * blocks, dtype=torch.int32, device=dev), torch.empty(256 * blocks, dtype=torch.int32, device=dev))


def sort_pass(keys, vals, events: int, shift: int, totals, base, keys_out, vals_out, stages: int = ALL_STAGES) -> None:
    """One stable pass over bits ``[shift, shift + 8)`` of ``keys``: count, totals and/or apply
    (``stages``, a sum of ``STAGE_*``) on the current torch stream."""
    if shift not in (0, 8, 16, 24):
        raise ValueError("shift is 0, 8, 16 or 24")
    if not isinstance(stages, int) or not 1 <= stages <= ALL_STAGES:
        raise ValueError("stages is a sum of STAGE_COUNT, STAGE_TOTALS and STAGE_APPLY")
    hip_lib.call("bh_transitions_sort_pass", keys, keys.data_ptr(), vals.data_ptr(), events, shift, totals.data_ptr(),
                 base.data_ptr(), keys_out.data_ptr(), vals_out.data_ptr(), stages)


def sort(s: Sorted, passes: Optional[int] = None) -> Sorted:
    """``s`` with its events sorted stably by media number, in ``sort_passes(s.groups)`` passes
    (``passes`` overrides it for the probe; more passes than needed change nothing)."""
    passes = sort_passes(s.groups) if passes is None else passes
    if not 0 <= passes <= 4:
        raise ValueError("passes is 0-4")
    if passes == 0:
        return s
    keys, vals = s.keys, s.vals
    keys_b, vals_b, totals, base = sort_scratch(s)
    for k in range(passes):
        sort_pass(keys, vals, s.events, RADIX_BITS * k, totals, base, keys_b, vals_b)
        keys, keys_b, vals, vals_b = keys_b, keys, vals_b, vals
    return s._replace(keys=keys, vals=vals)


def pairs(s: Sorted, mask: int) -> None:
    """The pairs launch over the sorted ``s``; ``mask`` is ``gpu_fold.known_mask`` of the enum.
    ``s.matrix`` and ``s.changes`` must be zero."""
    if not isinstance(mask, int) or not 0 <= mask <= ALL_ONES:
        raise ValueError("the status mask is 64-bit")
    hip_lib.call("bh_transitions_pairs", s.keys, s.keys.data_ptr(), s.vals.data_ptr(), s.events, s.groups, mask,
                 s.matrix.data_ptr(), s.first.data_ptr(), s.last.data_ptr(), s.run_start.data_ptr(),
                 s.run_end.data_ptr(), s.changes.data_ptr())


class Collected(NamedTuple):
    """What crosses back to the host: O(classes^2 + media + overflow)."""
    counters: np.ndarray   # N_COUNTERS
    overflow: object       # the frame indices left to the host, as the device listed them
    matrix: np.ndarray     # (CLASSES, CLASSES)
    id_off: np.ndarray     # per media number
    id_len: np.ndarray
    first: np.ndarray      # int64: frame << 32 | status
    last: np.ndarray
    run_start: np.ndarray
    run_end: np.ndarray
    changes: np.ndarray


def collect(t: Tables, s: Optional[Sorted]) -> Collected:
    """``s`` is None where the stream has no status event that the device decided."""
    counters = t.counters.cpu().numpy()
    overflow = t.overflow[:int(counters[C_OVERFLOW])].cpu()
    if s is None:
        none = np.zeros(0, dtype=np.int64)
        return Collected(counters, overflow, np.zeros((CLASSES, CLASSES), dtype=np.int64), none, none, none, none, none,
                         none, none)
    used = t.slot_scan.indices[:s.groups].long()  # the claimed slots by rank
    ids = t.rows[t.claim[used] - 1, 2:4].cpu().numpy()
    return Collected(counters, overflow, s.matrix.cpu().numpy().reshape(CLASSES, CLASSES).astype(np.int64),
                     ids[:, 0], ids[:, 1], s.first.cpu().numpy(), s.last.cpu().numpy(), s.run_start.cpu().numpy(),
                     s.run_end.cpu().numpy(), s.changes.cpu().numpy())


def _signed(word: int) -> int:
    status = word & 0xFFFFFFFF
    return status - (1 << 32) if status >= 1 << 31 else status


def _run(s: Sorted, start: int, end: int) -> List[Tuple[int, int]]:
    """One media's ``(frame, status)`` pairs in stream order: a slice of the sorted events."""
    words = s.vals[start:end].cpu().numpy().tolist()
    return [(w >> 32, _signed(w)) for w in words]


def finish(data, offs: np.ndarray, n: int, c: Collected, s: Optional[Sorted], dialect: str = "protobufjs"):
    """The :class:`~beholder_amd.transitions.Transitions` from the device's columns and the host's own
    copy of the stream; the frames in ``c.overflow`` are decoded here with the service's codec."""
    from .. import replay, transitions as definition
    names = replay.status_names()
    t = definition.Transitions(frames=n, status_decode_errors=int(c.counters[C_STATUS_ERR]))
    for a, b in zip(*np.nonzero(c.matrix)):
        cell = tuple(definition.UNKNOWN if x == CLASS_UNKNOWN else int(x) for x in (a, b))
        t.matrix[cell] = int(c.matrix[a, b])
    view = memoryview(data)
    number = {}  # id -> media number, for the media the host shares with the device
    columns = (c.id_off.tolist(), c.id_len.tolist(), c.first.tolist(), c.last.tolist(), c.run_start.tolist(),
               c.run_end.tolist(), c.changes.tolist())
    for k, (off, length, first, last, start, end, changes) in enumerate(zip(*columns)):
        mid = str(view[off:off + length], "ascii")  # the device keeps ASCII ids only
        t.media[mid] = definition.MediaFlow(end - start, changes, _signed(first), first >> 32, _signed(last), last >> 32)
        t.status_events += end - start
        number[mid] = k
    if len(c.overflow):
        events = hip_lib.overflow_frames(c.overflow, len(c.overflow), data, offs)[1]
        per_media, errors = definition.status_events_of(events, dialect)
        t.status_decode_errors += errors
        for mid, mine in per_media.items():
            k = number.get(mid)
            if k is not None:  # upb: the device holds events of this media too
                theirs = _run(s, int(c.run_start[k]), int(c.run_end[k]))
                t.add_cells(definition.flow_of(theirs, names)[1], -1)
                mine = sorted(theirs + mine)
            flow, cells = definition.flow_of(mine, names)
            t.status_events += flow.status_events - (t.media[mid].status_events if k is not None else 0)
            t.media[mid] = flow
            t.add_cells(cells)
    return t


def transitions(data, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None):
    """``(Transitions, frames decoded on the host)`` of a framed stream through the device."""
    from .. import replay, transitions as definition
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "transitions")
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    n, offs = gpu_fold.index(data)
    if n == 0:
        return definition.Transitions(), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    t = allocate(buf, offs_dev, n)
    classify(t, dialect)
    claim(t, hash_mask)
    rank(t)
    groups, events = counts(t)
    s = None
    if events:
        s = sort(compact(t, groups, events))
        pairs(s, gpu_fold.known_mask(replay.status_names()))
    c = collect(t, s)
    return finish(data, offs, n, c, s, dialect), len(c.overflow)
