"""Streams shared by the tests of ``transitions``: the definition (test_transitions.py), the per-frame
code compiled for the host (test_hip_transitions_host.py) and the device path
(test_gpu_transitions.py)."""
from __future__ import annotations

import functools
import random

from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from coalesce_cases import mixed_stream  # noqa: F401  re-exported: the small stream of every kind of frame
from dedupe_cases import three_statuses  # noqa: F401  re-exported
from extract_cases import collision_pairs
from telemetry_corpus import body, fold_corpus

UNKNOWN_NUMBERS = (6, 63, 64, -1, 2 ** 31 - 1)  # no TelemetryStatusEntry number: one class
GROUP_TAIL = b"\x2b\x2c"  # an empty unknown group (field 5): upb's STRICT reader leaves the frame to the host


@functools.lru_cache(maxsize=None)
def corpus() -> bytes:
    return fold_corpus()


def status_stream(ids, statuses=7, other_every=0) -> bytes:
    """One status event per entry of ``ids``, its status ``i % statuses``; with ``other_every`` every
    that many-th frame is followed by a progress frame of the same id, which takes no part."""
    events = []
    for i, mid in enumerate(ids):
        events.append((STATUS_ID, body(mid, i % statuses)))
        if other_every and i % other_every == 0:
            events.append((PROGRESS_ID, body(mid, 1)))
    return frames(events)


def boundary_ids(full: int, variant: str) -> list:
    """``full + 1`` ids: ``full`` status events fill a unit of the sort, the next unit holds one."""
    a, b = b"m-a", b"m-b"
    if variant == "one-media":
        return [a] * (full + 1)
    if variant == "two-media-alternating":
        return [a if i % 2 else b for i in range(full + 1)]
    assert variant == "last-alone-in-its-media"
    return [a] * full + [b]


MANY_EXTRA = 28  # frames of many_media_stream beyond one per media


def media_numbers(ids: list, n_frames: int) -> dict:
    """The dense media number the device gives an id, for the ids whose number does not depend on
    which lane claims first: the table's claimed slots are the same set in any order of insertion
    (linear probing), a media's number is its slot's rank among them, and an id whose home slot has
    no claimed neighbour sits in its home slot."""
    import numpy as np

    from beholder_amd.ops import gpu_extract, gpu_fold
    slots = gpu_fold.table_slots(n_frames)
    homes = (gpu_extract.hash64_many(ids) & np.uint64(slots - 1)).tolist()
    claimed = set()
    for s in homes:
        while s in claimed:
            s = (s + 1) & (slots - 1)
        claimed.add(s)
    rank = {s: k for k, s in enumerate(sorted(claimed))}
    return {mid: rank[s] for mid, s in zip(ids, homes)
            if (s - 1) & (slots - 1) not in claimed and (s + 1) & (slots - 1) not in claimed}


@functools.lru_cache(maxsize=None)
def many_media_stream(media: int) -> tuple:
    """``(stream, a, b)``: one status event for each of ``media`` ids; a second and a third one for
    eight of them, spread over the stream; and twelve more that alternate between the media ``a``
    and ``b``, spread over the stream too. The numbers of ``a`` and ``b`` differ only in the digit of
    the last sort pass, so every earlier pass sees the two as one digit and must keep their events
    in order. ``media + MANY_EXTRA`` frames."""
    from beholder_amd.ops import gpu_transitions
    rng = random.Random(media)
    low = (1 << 8 * (max(1, gpu_transitions.sort_passes(media)) - 1)) - 1  # the digits of the earlier passes
    for salt in range(64):
        ids = [b"media-%d-%06d" % (salt, k) for k in range(media)]
        by_number = {number: mid for mid, number in media_numbers(ids, media + MANY_EXTRA).items()}
        pair = next(((mid, by_number[number ^ high]) for number, mid in sorted(by_number.items())
                     for high in range(low + 1, media, low + 1) if number ^ high in by_number and number < number ^ high),
                    None) if media > 1 else (ids[0], ids[0])
        if pair is not None:
            break
    assert pair is not None, "no salt gives two media whose numbers differ in the high digit only"
    events = [body(mid, k % 6) for k, mid in enumerate(ids)]
    for k in range(8):
        mid = ids[k * (media - 1) // 7]
        for status in (k % 5, 5):
            events.insert(rng.randrange(len(events) + 1), body(mid, status))
    for k, at in enumerate(sorted((rng.randrange(len(events) + 1) for _ in range(12)), reverse=True)):
        events.insert(at, body(pair[k % 2], k % 7))
    assert len(events) == media + MANY_EXTRA
    return frames([(STATUS_ID, b) for b in events]), pair[0], pair[1]


def pairs_stream() -> bytes:
    """360 status events over 120 ids that differ from a neighbour in the last byte only, shuffled."""
    rng = random.Random(1)
    events = [(STATUS_ID, body(mid, rng.randrange(7))) for pair in collision_pairs() for mid in pair for _ in range(3)]
    rng.shuffle(events)
    return frames(events)


def shared_media_stream() -> bytes:
    """Two ASCII media whose status events alternate plain bodies and bodies with an empty group,
    shuffled into each other, and a third with plain bodies only. Both dialects decode every frame;
    upb's STRICT reader leaves the group frames to the host."""
    rng = random.Random(6)
    events = []
    for mid in (b"m", b"shared-2"):
        events += [(mid, i, body(mid, rng.randrange(7)) + (GROUP_TAIL if i % 2 else b"")) for i in range(12)]
    events += [(b"plain", i, body(b"plain", rng.randrange(7))) for i in range(9)]
    rng.shuffle(events)
    return frames([(STATUS_ID, b) for _, _, b in events])
