"""What every worker host did in a framed telemetry stream, on the GPU
(``ops/hip/telemetry_hosts.hip``): the device path of ``python -m beholder_amd hosts --device gpu``
(:mod:`beholder_amd.hosts` defines the result).

"Host" in this package's names is the CPU side (``host_frames``, ``decide_on_host``); the value of
the proto's ``host`` field is called the *worker* here.

The stages, which ``scripts/gpu_hosts_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the CPU, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`classify` — one lane per frame reads a topic-2 frame: a decode error is counted, a frame
   the device does not decide (an id or a worker string with a byte >= 0x80, in both dialects; in
   the upb dialect also a start-group) goes to the overflow list, a progress event gets a row keyed
   by its id, a row keyed by its worker string, and its progress. Other topics are not read.
3. ``gpu_transitions.claim``, ``rank``, ``compact`` and ``sort`` over the id rows, as ``gpu_thin``
   calls them: the events end up sorted stably by their media's dense number. :func:`counts` reads
   back ``(groups, events, workers)``; a stream with no device event stops here.
4. The same ``claim`` and slot scan over the worker rows, in a second ``gpu_transitions.Tables``
   (:func:`worker_tables`): a claimed slot's rank is the worker's dense number.
5. :func:`number` — per sorted position, the worker number and the progress of its event.
6. :func:`pairs` — one more open-addressing table, keyed by ``media number << 32 | worker number``,
   counts the events per pair; ``gpu_extract.scan`` over its used slots compacts them.
7. :func:`walk` — one lane per sorted position decides stint start, handover or rewind against its
   predecessor and adds to its worker's row of :data:`WORKER_WORDS` counters; workers numbered below
   :data:`LDS_WORKERS` are summed in a per-block LDS table first.
8. :func:`collect` and :func:`finish` — one row per worker, per media and per pair, the counters and
   the overflow list come back; strings come from the CPU's own copy of the stream. The CPU decodes
   the overflow frames with the service's codec. Where one of their media is also the device's (an
   ASCII id in a frame with a non-ASCII worker, or under upb with a group), that media's run of the
   sorted events is read back, its device contributions are taken out, and the whole run,
   interleaved by frame index, goes through ``hosts.course_of`` and is added again.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`hosts`.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import gpu_extract, gpu_fold, gpu_transitions, hip_lib
from .gpu_fold import ALL_ONES
from .gpu_transitions import CLASS_UNKNOWN, CLASSES

C_PROGRESS_ERR, C_OVERFLOW, N_COUNTERS = 0, 1, 2  # counters[] of telemetry_hosts.hip
assert C_OVERFLOW == gpu_transitions.C_OVERFLOW
LDS_WORKERS = 64  # telemetry_hosts.hip: workers numbered below it are summed in the walk's LDS table
W_STARTS, W_TAKEN, W_LOST, W_REWINDS, W_CLASS = 0, 1, 2, 3, 4  # telemetry_hosts.hpp: a worker's row of counters
WORKER_WORDS = W_CLASS + CLASSES


class Tables(NamedTuple):
    """The device tensors of one run up to the sort. ``t`` holds the transitions' tensors over the id
    rows (``t.rows`` are progress events here); ``w`` the same over the worker rows: its rows, claim
    table and slot scan are its own, everything per frame is ``t``'s."""
    t: gpu_transitions.Tables
    w: gpu_transitions.Tables
    progress: object  # n int32: the progress of a progress event, else 0


class Walked(NamedTuple):
    """What the launches after the sort write, next to a ``gpu_transitions.Sorted``."""
    workers: int
    worker_of: object    # events int32: the worker number per sorted position
    prog: object         # events int32: the progress per sorted position
    pair_claim: object   # slots int64: 0 or 1 + the sorted position that claimed the slot
    pair_count: object   # slots int32
    pair_scan: gpu_extract.ScanTables  # over the used slots of the pair table
    worker_rows: object  # (workers, WORKER_WORDS) int32
    run_start: object    # groups int32
    run_end: object      # groups int32


def worker_tables(t: gpu_transitions.Tables) -> gpu_transitions.Tables:
    """A second table next to ``t`` for the worker strings: zeroed claims and its own rows."""
    import torch
    dev = t.buf.device
    slot_used = torch.zeros(t.slots, dtype=torch.int32, device=dev)
    return t._replace(rows=torch.empty((t.n, 6), dtype=torch.int32, device=dev),
                      claim=torch.zeros(t.slots, dtype=torch.int64, device=dev), slot_used=slot_used,
                      slot_of=torch.empty(t.n, dtype=torch.int32, device=dev),
                      slot_scan=gpu_extract.scan_tables(slot_used, t.slots, t.buf, t.offs))


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, zeroed where the kernels need it. Checks the
    arguments on the CPU."""
    import torch
    t = gpu_transitions.allocate(buf_dev, offs_dev, n)  # checks the tensors, n and the stream's size
    return Tables(t, worker_tables(t), torch.empty(n, dtype=torch.int32, device=buf_dev.device))


def classify(tb: Tables, dialect: str = "protobufjs") -> None:
    """The classify launch over ``tb`` on the current torch stream. ``tb.t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``tb.t.counters`` must be zero."""
    dialect_id = hip_lib.check_dialect(dialect)
    t = tb.t
    hip_lib.call("bh_hosts_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id, t.rows.data_ptr(),
                 tb.w.rows.data_ptr(), tb.progress.data_ptr(), t.is_event.data_ptr(), t.counters.data_ptr(),
                 t.overflow.data_ptr())


def claim(tb: Tables, hash_mask: int = ALL_ONES) -> None:
    """The transitions' claim over the id rows and over the worker rows."""
    gpu_transitions.claim(tb.t, hash_mask)
    gpu_transitions.claim(tb.w, hash_mask)


def rank(tb: Tables) -> None:
    """The transitions' rank over the id table, and the slot scan of the worker table."""
    gpu_transitions.rank(tb.t)
    gpu_extract.scan(tb.w.slot_scan)


def counts(tb: Tables) -> Tuple[int, int, int]:
    """``(groups, events, workers)`` after :func:`rank`: the three words the CPU reads before it sorts."""
    import torch
    totals = (tb.t.slot_scan.base[-1], tb.t.event_scan.base[-1], tb.w.slot_scan.base[-1])
    words = torch.stack(totals).cpu().numpy() >> 32
    return int(words[0]), int(words[1]), int(words[2])


def prepare(tb: Tables, s: gpu_transitions.Sorted, workers: int) -> Walked:
    """The zeroed tensors of :func:`number`, :func:`pairs` and :func:`walk` next to the sorted ``s``.
    ``workers`` must be :func:`counts`'s."""
    import torch
    if not 1 <= workers <= s.events:
        raise ValueError("workers is the worker scan's total, and there is at least one event")
    dev = s.keys.device
    slots = tb.t.slots
    pair_used = torch.zeros(slots, dtype=torch.int32, device=dev)
    return Walked(workers, torch.empty(s.events, dtype=torch.int32, device=dev),
                  torch.empty(s.events, dtype=torch.int32, device=dev),
                  torch.zeros(slots, dtype=torch.int64, device=dev), torch.zeros(slots, dtype=torch.int32, device=dev),
                  gpu_extract.scan_tables(pair_used, slots, tb.t.buf, tb.t.offs),
                  torch.zeros((workers, WORKER_WORDS), dtype=torch.int32, device=dev),
                  torch.empty(s.groups, dtype=torch.int32, device=dev),
                  torch.empty(s.groups, dtype=torch.int32, device=dev))


def number(tb: Tables, s: gpu_transitions.Sorted, k: Walked) -> None:
    """The number launch: ``k.worker_of`` and ``k.prog`` per position of the sorted ``s``."""
    w = tb.w
    hip_lib.call("bh_hosts_number", s.vals, s.vals.data_ptr(), s.events, w.n, w.slot_of.data_ptr(),
                 w.slot_scan.pos.data_ptr(), w.slots, tb.progress.data_ptr(), k.worker_of.data_ptr(), k.prog.data_ptr())


def pairs(tb: Tables, s: gpu_transitions.Sorted, k: Walked, hash_mask: int = ALL_ONES) -> None:
    """The pairs launch after :func:`number`, and the scan over the pair table's used slots.
    ``k.pair_claim``, ``k.pair_count`` and the scan's ``keep_len`` must be zero."""
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    hip_lib.call("bh_hosts_pairs", s.keys, s.keys.data_ptr(), k.worker_of.data_ptr(), s.events, hash_mask,
                 k.pair_claim.data_ptr(), k.pair_scan.keep_len.data_ptr(), k.pair_count.data_ptr(), tb.t.slots)
    gpu_extract.scan(k.pair_scan)


def walk(s: gpu_transitions.Sorted, k: Walked, mask: int) -> None:
    """The walk launch after :func:`number`; ``mask`` is ``gpu_fold.known_mask`` of the enum.
    ``k.worker_rows`` must be zero."""
    if not isinstance(mask, int) or not 0 <= mask <= ALL_ONES:
        raise ValueError("the status mask is 64-bit")
    hip_lib.call("bh_hosts_walk", s.keys, s.keys.data_ptr(), s.vals.data_ptr(), k.worker_of.data_ptr(),
                 k.prog.data_ptr(), s.events, s.groups, k.workers, mask, k.worker_rows.data_ptr(),
                 k.run_start.data_ptr(), k.run_end.data_ptr())


class Collected(NamedTuple):
    """What crosses back to the CPU: O(workers + media + pairs + overflow)."""
    counters: np.ndarray     # N_COUNTERS
    overflow: object         # the frame indices left to the CPU, as the device listed them
    worker_span: np.ndarray  # (workers, 2): offset and length of every worker's string in the stream
    worker_rows: np.ndarray  # (workers, WORKER_WORDS)
    id_span: np.ndarray      # (groups, 2)
    run_start: np.ndarray
    run_end: np.ndarray
    edges: np.ndarray        # (2, groups, 3) int64: every media's first and last event, as
                             # (frame << 32 | status, worker number, progress)
    triples: np.ndarray      # (pairs, 3) int64: media number, worker number, events


def _spans(t: gpu_transitions.Tables, count: int) -> np.ndarray:
    used = t.slot_scan.indices[:count].long()  # the claimed slots by rank
    return t.rows[t.claim[used] - 1, 2:4].cpu().numpy()


def collect(tb: Tables, s: Optional[gpu_transitions.Sorted], k: Optional[Walked]) -> Collected:
    """``s`` and ``k`` are None where the stream has no progress event that the device decided."""
    import torch
    counters = tb.t.counters.cpu().numpy()
    overflow = tb.t.overflow[:int(counters[C_OVERFLOW])].cpu()
    if s is None:
        none = np.zeros((0, 2), dtype=np.int64)
        return Collected(counters, overflow, none, np.zeros((0, WORKER_WORDS), dtype=np.int64), none, none[:, 0],
                         none[:, 0], np.zeros((2, 0, 3), dtype=np.int64), np.zeros((0, 3), dtype=np.int64))
    run_start, run_end = k.run_start.long(), k.run_end.long()
    at = torch.stack((run_start, run_end - 1))  # the positions of every media's two edge events
    edges = torch.stack((s.vals[at], k.worker_of[at].long(), k.prog[at].long()), dim=-1)
    pair_count = gpu_extract.totals(k.pair_scan)[0]
    slots = k.pair_scan.indices[:pair_count].long()  # the claimed slots of the pair table
    owners = k.pair_claim[slots] - 1
    triples = torch.stack((s.keys[owners].long(), k.worker_of[owners].long(), k.pair_count[slots].long()), dim=-1)
    return Collected(counters, overflow, _spans(tb.w, k.workers), k.worker_rows.cpu().numpy(),
                     _spans(tb.t, s.groups), run_start.cpu().numpy(), run_end.cpu().numpy(), edges.cpu().numpy(),
                     triples.cpu().numpy())


def _signed(word: int) -> int:
    status = word & 0xFFFFFFFF
    return status - (1 << 32) if status >= 1 << 31 else status


def _run(s: gpu_transitions.Sorted, k: Walked, start: int, end: int, names: List[str]) -> list:
    """One media's ``(frame, host, status, progress)`` events in stream order: a slice of the sorted events."""
    words = s.vals[start:end].cpu().numpy().tolist()
    workers = k.worker_of[start:end].cpu().numpy().tolist()
    progress = k.prog[start:end].cpu().numpy().tolist()
    return [(v >> 32, names[w], _signed(v), p) for v, w, p in zip(words, workers, progress)]


def finish(data, offs: np.ndarray, n: int, c: Collected, s: Optional[gpu_transitions.Sorted], k: Optional[Walked],
           dialect: str = "protobufjs"):
    """The :class:`~beholder_amd.hosts.HostReport` from the device's columns and the CPU's own copy of
    the stream; the frames in ``c.overflow`` are decoded here with the service's codec."""
    from .. import hosts as definition, replay
    status_names = replay.status_names()
    report = definition.HostReport(frames=n, progress_decode_errors=int(c.counters[C_PROGRESS_ERR]))
    view = memoryview(data)

    def text(span) -> str:
        return str(view[int(span[0]):int(span[0]) + int(span[1])], "ascii")  # the device keeps ASCII strings only
    workers = [text(span) for span in c.worker_span]
    ids = [text(span) for span in c.id_span]
    classes = c.worker_rows[:, W_CLASS:]
    by_class = [{} for _ in workers]
    where = np.nonzero(classes)  # a worker has events in a few classes: only those cells are walked
    for worker, cls, count in zip(where[0].tolist(), where[1].tolist(), classes[where].tolist()):
        by_class[worker][definition.UNKNOWN if cls == CLASS_UNKNOWN else cls] = count
    columns = (workers, classes.sum(axis=1).tolist(), by_class, c.worker_rows[:, :W_CLASS].tolist())
    for name, events, counts_of, head in zip(*columns):
        report.hosts[name] = definition.HostRow(events, counts_of, head[W_STARTS] + head[W_TAKEN], head[W_TAKEN],
                                                head[W_LOST], head[W_REWINDS])
    report.pairs = dict(zip(zip(map(ids.__getitem__, c.triples[:, 0].tolist()),
                                map(workers.__getitem__, c.triples[:, 1].tolist())), c.triples[:, 2].tolist()))

    def event(edge) -> tuple:
        return edge[0] >> 32, workers[edge[1]], _signed(edge[0]), edge[2]
    for mid, start, end, first, last in zip(ids, c.run_start.tolist(), c.run_end.tolist(), c.edges[0].tolist(),
                                            c.edges[1].tolist()):
        report.media[mid] = definition.MediaEdge(end - start, event(first), event(last))
        report.progress_events += end - start
    if len(c.overflow):
        events = hip_lib.overflow_frames(c.overflow, len(c.overflow), data, offs)[1]
        per_media, errors = definition.progress_events_of(events, dialect)
        report.progress_decode_errors += errors
        number = {mid: i for i, mid in enumerate(ids)}
        for mid, mine in per_media.items():
            i = number.get(mid)
            if i is not None:  # the device holds events of this media too
                theirs = _run(s, k, int(c.run_start[i]), int(c.run_end[i]), workers)
                report.add_course(mid, *definition.course_of(theirs, status_names), sign=-1)
                mine = sorted(theirs + mine)
            report.add_course(mid, *definition.course_of(mine, status_names))
    return report


def hosts(data, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None):
    """``(HostReport, frames decoded on the CPU)`` of a framed stream through the device."""
    from .. import hosts as definition, replay
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "hosts")
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    n, offs = gpu_fold.index(data)  # raises for a stream of 2^31 bytes or more
    if n == 0:
        return definition.HostReport(), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    tb = allocate(buf, offs_dev, n)
    classify(tb, dialect)
    claim(tb, hash_mask)
    rank(tb)
    groups, events, workers = counts(tb)
    s = k = None
    if events:
        s = gpu_transitions.sort(gpu_transitions.compact(tb.t, groups, events))
        k = prepare(tb, s, workers)
        number(tb, s, k)
        pairs(tb, s, k, hash_mask)
        walk(s, k, gpu_fold.known_mask(replay.status_names()))
    c = collect(tb, s, k)
    return finish(data, offs, n, c, s, k, dialect), len(c.overflow)
