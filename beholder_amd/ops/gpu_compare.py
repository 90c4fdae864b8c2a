"""Two framed telemetry streams matched frame for frame on the GPU
(``ops/hip/telemetry_compare.hip``): the device path of ``python -m beholder_amd compare --device gpu``
(:mod:`beholder_amd.compare` defines the result).

The stages, which ``scripts/gpu_compare_probe.py`` times one by one:

1. ``gpu_fold.index`` over each capture and :func:`upload` — the two captures go to the device as
   **one joined stream**, A's ``n_a`` frames first and then B's with their offsets shifted by A's
   size: two copies into one device tensor, no joined copy on the host. The side of frame ``m`` is
   ``m >= n_a``.
2. :func:`classify` — one lane per joined frame: skipped because its topic is not selected (counted
   per side), left to the host because its content is longer than ``DEDUPE_DEVICE_MAX``, or given
   its row in the transitions' layout, with the dedupe's content hash and the side where the
   transitions keep a status.
3. ``gpu_transitions.claim``, ``rank``, ``counts``, ``compact`` and ``sort`` — the transitions'
   stages as they are: equal contents of both captures meet in one slot (length, hash, then bytes),
   get a dense content number, and the frames end up sorted stably by it, so a content's run holds
   A's occurrences in stream order and then B's. A stream with no participating device frame stops
   before ``compact``.
4. :func:`bounds` and :func:`match` — per content the run's start, the start of its B half and its
   end; then per sorted position the pairing rule: the frame's rank on its side against the smaller
   side's count. Unmatched frames get their length in ``keep_a`` or ``keep_b``; matched frames of A
   get ``is_matched`` and ``partner``, the joined index of the B frame they are paired with.
5. :func:`pair_on_host` — the frames above the cap come back as a list and are paired by the same
   rule in a plain dict; their lengths, flags and partners are scattered into the same device
   arrays. A host frame is longer than the cap and a device frame is not, so the two never share a
   content.
6. ``gpu_extract.scan`` over ``is_matched`` and :func:`breaks` — A's matched frames in stream
   order, and the adjacent descents of their partners.
7. ``gpu_extract.scan``, ``totals``, ``gather`` and ``collect`` — the extract's prefix sum and copy,
   as they are, twice: over ``keep_a`` and over ``keep_b``. B's indices come back as joined indices
   and the host subtracts ``n_a``.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`compare`.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import gpu_dedupe, gpu_extract, gpu_fold, gpu_transitions, hip_lib
from .gpu_dedupe import DEDUPE_DEVICE_MAX  # noqa: F401  the cap above which the host pairs

# counters[] of telemetry_compare.hip
(C_SKIPPED_A, C_OVERFLOW, C_SKIPPED_B, C_MATCHED, C_DISTINCT_A, C_DISTINCT_B, C_COMMON, C_BREAKS,
 N_COUNTERS) = range(9)
assert C_OVERFLOW == gpu_transitions.C_OVERFLOW


class Tables(NamedTuple):
    """The device tensors of one comparison. ``t`` holds the transitions' tensors, for its claim,
    rank, compact and sort (``t.rows`` are contents here, ``t.counters`` has ``N_COUNTERS`` words);
    ``select_a`` and ``select_b`` the extract's over ``keep_a`` and ``keep_b``, ``matched_scan`` the
    extract's over the first ``n_a`` words of ``is_matched`` (None where A is empty)."""
    t: gpu_transitions.Tables
    n_a: int
    keep_a: object      # n int32: the frame's length where it is only in A, else 0
    keep_b: object      # n int32: the frame's length where it is only in B, else 0
    is_matched: object  # n int32: 1 for a matched frame of A
    partner: object     # n int32: a matched frame of A's partner, a joined index
    select_a: gpu_extract.ScanTables
    select_b: gpu_extract.ScanTables
    matched_scan: Optional[gpu_extract.ScanTables]


class Bounds(NamedTuple):
    """Per content number: its run of the sorted events and where the run's B half starts."""
    run_start: object
    side_start: object
    run_end: object


def _check_policy(policy) -> None:
    from .. import compare
    if not isinstance(policy, compare.Policy):
        raise TypeError(f"policy is a compare.Policy, not {type(policy).__name__}")


def params_of(policy, slots: int, hash_mask: int = gpu_fold.ALL_ONES) -> gpu_dedupe.DedupeParams:
    """``policy`` flattened for the classify kernel: the dedupe's params, whose topics it reads."""
    from .. import dedupe
    _check_policy(policy)
    return gpu_dedupe.dedupe_params(dedupe.Policy(topics=policy.topics), slots, hash_mask)


def join_offsets(offs_a: np.ndarray, offs_b: np.ndarray, bytes_a: int) -> np.ndarray:
    """The joined stream's ``n_a + n_b + 1`` frame starts: A's, then B's shifted by A's size."""
    if bytes_a + (int(offs_b[-1]) if len(offs_b) else 0) >= 2 ** 31:
        raise ValueError("stream too large for int32 offsets")
    return np.concatenate((offs_a, offs_b[1:] + np.int32(bytes_a))).astype(np.int32, copy=False)


def upload(a, b, offs: np.ndarray, device="cuda") -> Tuple[object, object]:
    """The joined stream and its offsets on ``device``: each capture is copied from where it lies
    on the host into its part of one device tensor."""
    import warnings

    import torch
    buf = torch.empty(len(a) + len(b), dtype=torch.uint8, device=device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # a read-only view is all the copy needs
        at = 0
        for part in (a, b):
            if len(part):
                buf[at:at + len(part)].copy_(torch.frombuffer(part, dtype=torch.uint8))
                at += len(part)
    return buf, torch.from_numpy(offs).to(device)


def allocate(buf_dev, offs_dev, n: int, n_a: int) -> Tables:
    """Tables for ``n`` joined frames, the first ``n_a`` of them A's, next to ``buf_dev``, zeroed
    where the kernels need it. Checks the arguments on the host."""
    import torch
    if isinstance(n_a, bool) or not isinstance(n_a, int) or not 0 <= n_a <= n:
        raise ValueError("n_a is A's frame count, 0..n")
    t = gpu_transitions.allocate(buf_dev, offs_dev, n)  # checks the tensors, n, the stream's and the table's size
    dev = buf_dev.device
    t = t._replace(counters=torch.zeros(N_COUNTERS, dtype=torch.int32, device=dev))

    def empty():
        return torch.empty(n, dtype=torch.int32, device=dev)
    keep_a, keep_b, is_matched = empty(), empty(), empty()
    return Tables(t, n_a, keep_a, keep_b, is_matched, empty(),
                  gpu_extract.scan_tables(keep_a, n, buf_dev, offs_dev),
                  gpu_extract.scan_tables(keep_b, n, buf_dev, offs_dev),
                  gpu_extract.scan_tables(is_matched, n_a, buf_dev, offs_dev) if n_a else None)


def classify(tb: Tables, params: gpu_dedupe.DedupeParams) -> None:
    """The classify launch over ``tb`` on the current torch stream. ``tb.t.offs`` must be
    :func:`join_offsets` of two ``gpu_fold.index`` results: the kernel trusts it. ``tb.t.counters``
    must be zero."""
    t = tb.t
    if params.slot_mask + 1 != t.slots:
        raise ValueError("params were made for another table")
    hip_lib.call("bh_compare_classify", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, tb.n_a,
                 ctypes.addressof(params), t.rows.data_ptr(), t.is_event.data_ptr(), tb.keep_a.data_ptr(),
                 tb.keep_b.data_ptr(), tb.is_matched.data_ptr(), t.counters.data_ptr(), t.overflow.data_ptr())


def bounds(s: gpu_transitions.Sorted) -> Bounds:
    """The bounds launch over the sorted ``s``: every content's run and the start of its B half."""
    import torch
    dev = s.keys.device
    b = Bounds(*(torch.empty(s.groups, dtype=torch.int32, device=dev) for _ in range(3)))
    hip_lib.call("bh_compare_bounds", s.keys, s.keys.data_ptr(), s.vals.data_ptr(), s.events, s.groups,
                 b.run_start.data_ptr(), b.side_start.data_ptr(), b.run_end.data_ptr())
    return b


def match(tb: Tables, s: gpu_transitions.Sorted, b: Bounds) -> None:
    """The match launch over the sorted ``s`` and its bounds: writes ``keep_a``, ``keep_b``,
    ``is_matched`` and ``partner`` for every frame in ``s`` and adds to the counters."""
    t = tb.t
    if not 1 <= s.events <= t.n:
        raise ValueError("the events are the scan's total, and there is at least one")
    hip_lib.call("bh_compare_match", s.keys, s.keys.data_ptr(), s.vals.data_ptr(), s.events, s.groups,
                 t.offs.data_ptr(), t.n, b.run_start.data_ptr(), b.side_start.data_ptr(), b.run_end.data_ptr(),
                 tb.keep_a.data_ptr(), tb.keep_b.data_ptr(), tb.is_matched.data_ptr(), tb.partner.data_ptr(),
                 t.counters.data_ptr())


class HostPairs(NamedTuple):
    """What :func:`pair_on_host` decided, to add to the device's counters."""
    frames: int = 0      # the overflow list's length
    matched: int = 0
    distinct_a: int = 0
    distinct_b: int = 0
    common: int = 0


def pair_on_host(tb: Tables, data_a, data_b, offs: np.ndarray) -> Tuple[np.ndarray, HostPairs]:
    """Reads the counters; where the overflow list is not empty, pairs those frames by content in a
    plain dict, the k-th occurrence in A with the k-th in B, and scatters the unmatched ones'
    lengths into ``keep_a`` and ``keep_b`` and the matched ones' flags and partners into
    ``is_matched`` and ``partner``. Returns ``(the counters, what the host added)``."""
    import torch
    t = tb.t
    counters = t.counters.cpu().numpy().astype(np.int64)
    count = int(counters[C_OVERFLOW])
    if count == 0:
        return counters, HostPairs()
    frames = np.sort(t.overflow[:count].cpu().numpy()).tolist()
    views = memoryview(data_a), memoryview(data_b)
    where = {}  # content -> (its frames of A, its frames of B), joined indices, ascending
    for m in frames:
        side = int(m >= tb.n_a)
        shift = int(offs[tb.n_a]) if side else 0
        content = bytes(views[side][int(offs[m]) + 4 - shift:int(offs[m + 1]) - shift])
        where.setdefault(content, ([], []))[side].append(m)
    pairs, only = [], ([], [])
    for mine, theirs in where.values():
        k = min(len(mine), len(theirs))
        pairs.extend(zip(mine[:k], theirs[:k]))
        only[0].extend(mine[k:])
        only[1].extend(theirs[k:])
    dev = t.buf.device

    def scatter(target, index, values):
        if index:
            target[torch.tensor(index, dtype=torch.int64).to(dev)] = torch.tensor(values, dtype=torch.int32).to(dev)
    for keep, side in ((tb.keep_a, only[0]), (tb.keep_b, only[1])):
        scatter(keep, side, [int(offs[m + 1]) - int(offs[m]) for m in side])
    scatter(tb.is_matched, [m for m, _ in pairs], [1] * len(pairs))
    scatter(tb.partner, [m for m, _ in pairs], [p for _, p in pairs])
    return counters, HostPairs(count, len(pairs), sum(1 for mine, _ in where.values() if mine),
                               sum(1 for _, theirs in where.values() if theirs),
                               sum(1 for mine, theirs in where.values() if mine and theirs))


def breaks(tb: Tables) -> Tuple[int, int]:
    """``(matched, order_breaks)``: the scan over ``is_matched`` lists A's matched frames in stream
    order, the breaks launch counts the adjacent descents of their partners, and the two words are
    read back. ``tb.t.counters[C_BREAKS]`` must be zero."""
    if tb.matched_scan is None:
        return 0, 0
    gpu_extract.scan(tb.matched_scan)
    matched = gpu_extract.totals(tb.matched_scan)[0]
    if matched < 2:
        return matched, 0
    t = tb.t
    hip_lib.call("bh_compare_breaks", tb.partner, tb.matched_scan.indices.data_ptr(), matched, tb.partner.data_ptr(),
                 t.n, t.counters.data_ptr())
    return matched, int(t.counters[C_BREAKS].item())


def only(select: gpu_extract.ScanTables):
    """``(bytes, indices)`` of the frames with a length in ``select.keep_len``: the extract's scan,
    totals, gather and collect."""
    gpu_extract.scan(select)
    kept, kept_bytes = gpu_extract.totals(select)
    return gpu_extract.collect(select, gpu_extract.gather(select, kept, kept_bytes), kept)


def compare(a, b, policy, device="cuda", hash_mask: Optional[int] = None):
    """``(Comparison, frames paired on the host)`` of two framed streams through the device."""
    from .. import compare as definition
    _check_policy(policy)
    hip_lib.require_gpu(device, "compare")
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    error = definition.device_limit_error(len(a), len(b))
    if error:
        raise ValueError(error)
    indexed = []
    for side, data in (("A", a), ("B", b)):
        try:
            indexed.append(gpu_fold.index(data))
        except ValueError as e:
            raise ValueError(f"capture {side}: {e}") from None
    (n_a, offs_a), (n_b, offs_b) = indexed
    n = n_a + n_b
    if n == 0:
        return definition.Comparison(topics=policy.topics), 0
    error = definition.device_limit_error(len(a), len(b), n)
    if error:
        raise ValueError(error)
    hip_lib.lib()  # a missing library raises before anything is uploaded
    params = params_of(policy, gpu_fold.table_slots(n), hash_mask)
    offs = join_offsets(offs_a, offs_b, len(a))
    buf, offs_dev = upload(a, b, offs, device)
    tb = allocate(buf, offs_dev, n, n_a)
    classify(tb, params)
    gpu_transitions.claim(tb.t, hash_mask)
    gpu_transitions.rank(tb.t)
    groups, events = gpu_transitions.counts(tb.t)
    if events:
        s = gpu_transitions.sort(gpu_transitions.compact(tb.t, groups, events))
        match(tb, s, bounds(s))
    counters, host = pair_on_host(tb, a, b, offs)
    matched, order_breaks = breaks(tb)
    data_a, indices_a = only(tb.select_a)
    data_b, indices_b = only(tb.select_b)
    if matched != int(counters[C_MATCHED]) + host.matched:
        raise RuntimeError("the matched frames the scan lists are not the pairs the match counted")
    result = definition.Comparison(
        definition.Side(data_a, indices_a, n_a, int(counters[C_SKIPPED_A]),
                        int(counters[C_DISTINCT_A]) + host.distinct_a),
        definition.Side(data_b, [i - n_a for i in indices_b], n_b, int(counters[C_SKIPPED_B]),
                        int(counters[C_DISTINCT_B]) + host.distinct_b),
        matched, int(counters[C_COMMON]) + host.common, order_breaks, policy.topics)
    return result, host.frames
