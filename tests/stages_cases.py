"""Streams shared by the tests of ``stages``: the definition (test_stages.py), the per-frame code
compiled for the host (test_hip_stages_host.py) and the device path (test_gpu_stages.py)."""
from __future__ import annotations

import functools
import random

from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from telemetry_corpus import body, fold_corpus
from thin_cases import PERCENTAGES, UNKNOWN_STATUSES, progress_body
from transitions_cases import GROUP_TAIL

S, P = "s", "p"  # the kind of an entry of joined_stream


@functools.lru_cache(maxsize=None)
def corpus() -> bytes:
    return fold_corpus()


def joined_stream(events) -> bytes:
    """One frame per entry: ``(S, mid, status)`` a status frame, ``(P, mid, status, progress)`` a
    progress frame, with an optional host after it."""
    out = []
    for kind, mid, status, *rest in events:
        if kind == S:
            out.append((STATUS_ID, body(mid, status)))
        else:
            out.append((PROGRESS_ID, progress_body(mid, status, *rest)))
    return frames(out)


@functools.lru_cache(maxsize=None)
def random_stream(seed: int, events: int = 200) -> bytes:
    """A seeded stream: status and progress events of a few media (one without an id, two that are
    not ASCII, two that are no UTF-8); a progress event reports its media's standing status more
    often than not; the percentage edges, unknown status numbers and hosts are mixed in; other topics
    and undecodable frames of both topics in between. ``late`` gets its first status event late and
    ``never`` none at all, so both have a lead."""
    rng = random.Random(seed)
    ids = [b"m-1", b"m-2", b"m-3", b"late", b"never", b"", "é".encode(), "メ".encode(), b"\xff", b"\xfe"]
    standing = {}
    out = []
    for k in range(events):
        roll = rng.random()
        mid = rng.choice(ids)
        if roll < 0.6:
            status = standing.get(mid, 2) if rng.random() < 0.7 else rng.choice((1, 2, 3) + UNKNOWN_STATUSES)
            progress = rng.choice(PERCENTAGES) if rng.random() < 0.25 else rng.choice((0, 3, 12, 50, 99, 100))
            host = rng.choice((None, b"node-a", "nœud".encode()))
            out.append((PROGRESS_ID, progress_body(mid, status, progress, host)))
        elif roll < 0.82:
            if mid == b"never" or (mid == b"late" and k < events // 2):
                continue
            standing[mid] = rng.choice((0, 1, 2, 3, 4, 5) + UNKNOWN_STATUSES[:1])
            out.append((STATUS_ID, body(mid, standing[mid])))
        elif roll < 0.88:
            out.append((rng.choice((0, 3, 9, 255)), progress_body(mid, 1, 5)))
        elif roll < 0.94:
            out.append((PROGRESS_ID, rng.choice((b"\x2e", b"\x2f\x00", b"\x0a\x05m", b"\x18\xff\xff\xff\xff\xff"))))
        else:
            out.append((STATUS_ID, rng.choice((b"\x2e", b"\x0a\x05m", b"\x10\xff\xff\xff\xff\xff"))))
    return frames(out)


def merge_stream() -> bytes:
    """About 60 frames in which media and stages cross every cut: ``a`` has stages with progress in
    them (a lead joins an open stage, a stage is closed by the later operand), ``lead`` only progress
    events until its late status event (a lead joins a lead), ``early`` only in the first third and
    ``tail`` only in the last (a media present in one operand only)."""
    events = []
    for k in range(20):
        events.append((P, b"a", 2, 5 * k))
        events.append((P, b"lead", 3, k) if k != 15 else (S, b"lead", 3))
        if k % 6 == 2:
            events.append((S, b"a", 1 + k // 6))
        if k < 6:
            events.append((S, b"early", 2) if k % 3 == 0 else (P, b"early", 2, 10 * k))
        if k > 14:
            events.append((S, b"tail", 4) if k % 2 else (P, b"tail", 4, 100))
    return joined_stream(events)


def bucket_edges() -> bytes:
    """One media whose stages end on every percentage edge, one stage with no progress event, under
    two statuses and the unknown ones on both topics; a second media's open stage ends on each edge
    in turn as the stream is cut."""
    events = []
    for status in (2, 3) + UNKNOWN_STATUSES:
        for p in PERCENTAGES:
            events += [(S, b"edge", status), (P, b"edge", status, 50), (P, b"edge", UNKNOWN_STATUSES[0], p)]
        events += [(S, b"edge", status)]  # closes the last and is closed with no progress event
    events += [(S, b"edge", 5)]
    return joined_stream(events)


def one_media(statuses_at, count: int, mid: bytes = b"m", status: int = 2) -> list:
    """``count`` events of one media: a status event at every index in ``statuses_at``, progress
    events (rising by one, under the standing status) everywhere else."""
    at = set(statuses_at)
    return [(S, mid, status + (k % 3)) if k in at else (P, mid, status, k % 101) for k in range(count)]


def stitch_stream() -> bytes:
    """Two ASCII media whose events of both topics alternate plain bodies and bodies with an empty
    group, shuffled into each other, a third with plain bodies only and a fourth with groups only.
    Both dialects decode every frame; upb's STRICT reader leaves the group frames to the CPU, so the
    status event a device progress event stands on is often the CPU's, and the other way round."""
    rng = random.Random(8)
    bodies = {}
    for mid, count, group in ((b"m", 24, "odd"), (b"shared-2", 24, "third"), (b"plain", 9, "none"), (b"host-only", 8, "all")):
        mine = []
        for i in range(count):
            is_status = i % 4 == (1 if mid == b"m" else 2)  # m: the CPU's frames are the status events
            b = (STATUS_ID, body(mid, 1 + i // 4)) if is_status else (PROGRESS_ID, progress_body(mid, 1 + i // 5, 7 * i % 120))
            tail = group == "all" or (group == "odd" and i % 2) or (group == "third" and i % 3 == 0)
            mine.append((b[0], b[1] + (GROUP_TAIL if tail else b"")))
        bodies[mid] = mine
    turns = [mid for mid, mine in bodies.items() for _ in mine]
    rng.shuffle(turns)  # every media's bodies stay in their own order
    return frames([bodies[mid].pop(0) for mid in turns])


def placed_stream(where: str) -> bytes:
    """One ASCII media of 12 events under upb: the CPU's frames (with a group) ``first``, in the
    ``middle`` or ``last`` in the run, with status events on both sides."""
    cpu = {"first": range(0, 4), "middle": range(4, 8), "last": range(8, 12)}[where]
    out = []
    for i in range(12):
        b = (STATUS_ID, body(b"m", i // 3)) if i % 3 == 1 else (PROGRESS_ID, progress_body(b"m", 2, 9 * i))
        out.append((b[0], b[1] + (GROUP_TAIL if i in cpu else b"")))
    out.append((PROGRESS_ID, progress_body(b"dev-only", 2, 5)))
    out.append((STATUS_ID, body(b"cpu-only", 2) + GROUP_TAIL))
    return frames(out)


def non_ascii_stream() -> bytes:
    """Events of both topics of media whose ids are not ASCII, ASCII ones in between: under protobufjs
    ``b"\\xff"`` and ``b"\\xfe"`` are one media (U+FFFD), under upb they do not decode."""
    rng = random.Random(4)
    ids = ["é".encode(), "メディア".encode(), b"\xff", b"\xfe", b"ok\x80", b"caf\xc3\xa9", b"ascii-1", b"ascii-2"]
    return joined_stream([(S, rng.choice(ids), rng.choice((1, 2, 3))) if rng.random() < 0.25 else
                          (P, rng.choice(ids), rng.choice((1, 2)), rng.choice((0, 5, 10, 100))) for _ in range(300)])
