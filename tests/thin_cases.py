"""Streams shared by the tests of ``thin``: the definition (test_thin.py), the per-frame code compiled
for the host (test_hip_thin_host.py) and the device path (test_gpu_thin.py)."""
from __future__ import annotations

import functools
import random

from beholder_amd.ops import frames
from beholder_amd.thin import Policy
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from coalesce_cases import mixed_stream  # noqa: F401  re-exported: the small stream of every kind of frame
from telemetry_corpus import body, fold_corpus, varint
from transitions_cases import GROUP_TAIL

STEPS = (1, 10, 25, 2 ** 31 - 1)
PERCENTAGES = (-2 ** 31, -11, -10, -1, 0, 9, 10, 99, 100, 101, 2 ** 31 - 1)
UNKNOWN_STATUSES = (6, 64, -1)  # no TelemetryStatusEntry number: each its own mark
KEEPS = ("last", "first")
POLICIES = [Policy(step, keep) for step in STEPS for keep in KEEPS]


def policy_id(policy: Policy) -> str:
    return f"{policy.step}-{policy.keep}"


def progress_body(mid: bytes, status: int, progress: int, host: bytes = None) -> bytes:
    """An ``api.TelemetryProgress``: mediaId, status, progress (any int32 each) and, where given, host."""
    out = body(mid, status) + b"\x18" + varint(progress)
    return out if host is None else out + b"\x22" + varint(len(host)) + host


@functools.lru_cache(maxsize=None)
def corpus() -> bytes:
    return fold_corpus()


def progress_stream(events) -> bytes:
    """One progress frame per ``(mid, status, progress)``."""
    return frames([(PROGRESS_ID, progress_body(mid, status, progress)) for mid, status, progress in events])


def course(ids, marks="alternate", status_every=0) -> bytes:
    """One progress event per entry of ``ids``. With ``alternate`` a media's neighbouring events never
    share a mark (its percentages go 0, 10, 20, ... 90, 0, ...), so nothing is dropped under step 10;
    with ``constant`` they all share one, so one event per media survives. With ``status_every`` every
    that many-th event is followed by a status frame of the same id, which takes no part."""
    seen, events = {}, []
    for i, mid in enumerate(ids):
        k = seen[mid] = seen.get(mid, -1) + 1
        events.append((PROGRESS_ID, progress_body(mid, 2, 10 * (k % 10) if marks == "alternate" else 42)))
        if status_every and i % status_every == 0:
            events.append((STATUS_ID, body(mid, 2)))
    return frames(events)


def boundary_ids(count: int, media: int) -> list:
    """``count`` ids over ``media`` media in turn."""
    return [b"m-%d" % (i % media) for i in range(count)]


@functools.lru_cache(maxsize=None)
def random_stream(seed: int, events: int = 160) -> bytes:
    """A seeded stream: progress events of a few media (one without an id, two that are not ASCII,
    two that are no UTF-8) whose statuses and percentages come from small sets, so that marks repeat,
    with the percentage edges, unknown status numbers and hosts mixed in; status frames, other
    topics and undecodable frames in between."""
    rng = random.Random(seed)
    ids = [b"m-1", b"m-2", b"m-3", b"", "é".encode(), "メ".encode(), b"\xff", b"\xfe"]
    out = []
    for _ in range(events):
        roll = rng.random()
        mid = rng.choice(ids)
        if roll < 0.7:
            status = rng.choice((1, 1, 2, 2, 3) + UNKNOWN_STATUSES)
            progress = rng.choice(PERCENTAGES) if rng.random() < 0.3 else rng.choice((0, 3, 7, 12, 24, 25, 26, 50))
            host = rng.choice((None, b"node-a", b"node-b", "nœud".encode()))
            out.append((PROGRESS_ID, progress_body(mid, status, progress, host)))
        elif roll < 0.85:
            out.append((STATUS_ID, body(mid, rng.randrange(6))))
        elif roll < 0.9:
            out.append((rng.choice((0, 3, 9, 255)), progress_body(mid, 1, 5)))
        else:
            out.append((PROGRESS_ID, rng.choice((b"\x2e", b"\x2f\x00", b"\x0a\x05m", b"\x18\xff\xff\xff\xff\xff"))))
    return frames(out)


def edge_stream() -> bytes:
    """One media walking through every percentage edge twice over, under two statuses and the
    unknown status numbers: which neighbours share a mark depends on the step."""
    events = []
    for status in (2, 3) + UNKNOWN_STATUSES:
        for p in PERCENTAGES + PERCENTAGES[::-1]:
            events.append((b"edge", status, p))
            events.append((b"edge", status, p))
    return progress_stream(events)


def stitch_stream() -> bytes:
    """Two ASCII media whose progress events alternate plain bodies and bodies with an empty group,
    shuffled into each other, a third with plain bodies only and a fourth with groups only. Both
    dialects decode every frame; upb's STRICT reader leaves the group frames to the host, so the
    neighbours of most events sit on the other side. Percentages repeat in stretches of three."""
    rng = random.Random(8)
    bodies = {mid: [progress_body(mid, 2, 10 * (i // 3)) + (GROUP_TAIL if i % 2 else b"") for i in range(18)]
              for mid in (b"m", b"shared-2")}
    bodies[b"plain"] = [progress_body(b"plain", 2, 10 * (i // 3)) for i in range(9)]
    bodies[b"host-only"] = [progress_body(b"host-only", 2, 10 * (i // 2)) + GROUP_TAIL for i in range(6)]
    turns = [mid for mid, mine in bodies.items() for _ in mine]
    rng.shuffle(turns)  # every media's bodies stay in their own order
    return frames([(PROGRESS_ID, bodies[mid].pop(0)) for mid in turns])


def non_ascii_stream() -> bytes:
    """Progress events of media whose ids are not ASCII, ASCII ones in between: under protobufjs
    ``b"\\xff"`` and ``b"\\xfe"`` are one media (U+FFFD), under upb they do not decode."""
    rng = random.Random(4)
    ids = ["é".encode(), "メディア".encode(), b"\xff", b"\xfe", b"ok\x80", b"caf\xc3\xa9", b"ascii-1", b"ascii-2"]
    return progress_stream([(rng.choice(ids), rng.choice((1, 2)), rng.choice((0, 5, 10, 15))) for _ in range(300)])
