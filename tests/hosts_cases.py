"""Streams shared by the tests of ``hosts``: the definition (test_hosts.py), the per-frame code
compiled for the host (test_hip_hosts_host.py) and the device path (test_gpu_hosts.py)."""
from __future__ import annotations

import functools
import random

from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from telemetry_corpus import body, fold_corpus
from thin_cases import PERCENTAGES, UNKNOWN_STATUSES, progress_body
from transitions_cases import GROUP_TAIL

# the empty host, a few ASCII workers, a non-ASCII one and two that are no UTF-8
WORKERS = (None, b"", b"node-a", b"node-b", b"node-c", "nœud".encode(), b"\xff", b"\xfe")
ASCII_WORKERS = (b"node-a", b"node-b", b"node-c")


@functools.lru_cache(maxsize=None)
def corpus() -> bytes:
    return fold_corpus()


def worker_stream(events) -> bytes:
    """One progress frame per ``(mid, host, status, progress)``; a host of None leaves field 4 out."""
    return frames([(PROGRESS_ID, progress_body(mid, status, progress, host)) for mid, host, status, progress in events])


@functools.lru_cache(maxsize=None)
def random_stream(seed: int, events: int = 200) -> bytes:
    """A seeded stream: progress events of a few media (one without an id, two that are not ASCII,
    two that are no UTF-8) from :data:`WORKERS`, who keep a media for a few events more often than
    not, with statuses and percentages from small sets so that rewinds happen, the percentage edges
    and unknown status numbers mixed in; status frames, other topics and undecodable frames in
    between."""
    rng = random.Random(seed)
    ids = [b"m-1", b"m-2", b"m-3", b"m-4", b"", "é".encode(), "メ".encode(), b"\xff", b"\xfe"]
    holder = {}
    out = []
    for _ in range(events):
        roll = rng.random()
        mid = rng.choice(ids)
        if roll < 0.75:
            if mid not in holder or rng.random() < 0.4:
                holder[mid] = rng.choice(WORKERS)
            status = rng.choice((1, 2, 2, 2, 3) + UNKNOWN_STATUSES)
            progress = rng.choice(PERCENTAGES) if rng.random() < 0.2 else rng.choice((0, 3, 7, 12, 24, 50))
            out.append((PROGRESS_ID, progress_body(mid, status, progress, holder[mid])))
        elif roll < 0.85:
            out.append((STATUS_ID, body(mid, rng.randrange(6))))
        elif roll < 0.9:
            out.append((rng.choice((0, 3, 9, 255)), progress_body(mid, 1, 5, b"node-a")))
        else:
            out.append((PROGRESS_ID, rng.choice((b"\x2e", b"\x2f\x00", b"\x0a\x05m", b"\x22\x05n"))))
    return frames(out)


def one_worker(data: bytes, worker: bytes = b"only") -> bytes:
    """``data`` with every progress event that protobufjs decodes written again from its decoded
    fields, with the host ``worker``: the decoded id keeps its identity (U+FFFD is valid UTF-8)."""
    from beholder_amd import ops
    from beholder_amd.models import proto
    from beholder_amd.transport.framing import iter_frames
    decode = ops.codec_for(proto.load("api.TelemetryProgress"), "protobufjs").decode
    out = []
    for topic, b in iter_frames(data):
        b = bytes(b)
        if topic == PROGRESS_ID:
            try:
                m = decode(b)
            except proto.DecodeError:
                pass
            else:
                b = progress_body(m.mediaId.encode("utf-8"), m.status, m.progress, worker)
        out.append((topic, b))
    return frames(out)


def relay(ids, workers, status: int = 2, rising: bool = True) -> bytes:
    """One progress event per entry of ``ids``, the k-th by ``workers[k % len(workers)]``. A media's
    progress rises by one per event, or with ``rising`` False falls, so that every neighbouring pair
    of one worker is a rewind."""
    seen, events = {}, []
    for k, mid in enumerate(ids):
        j = seen[mid] = seen.get(mid, -1) + 1
        events.append((mid, workers[k % len(workers)], status, j if rising else -j))
    return worker_stream(events)


def many_workers(count: int, per_worker: int = 2) -> bytes:
    """``count`` workers ``w-0000`` ... over three media: every worker sends ``per_worker`` events
    in a row for one media, the second a rewind, then the next worker takes the media over."""
    events = []
    for w in range(count):
        for j in range(per_worker):
            events.append((b"m-%d" % (w % 3), b"w-%04d" % w, 2 + w % 2, 50 - j))
    return worker_stream(events)


def stitch_stream() -> bytes:
    """``thin_cases.stitch_stream`` with workers: two ASCII media whose events alternate plain bodies
    and bodies with an empty group, a third with plain bodies only and a fourth with groups only,
    shuffled into each other; the worker changes every few events and the progress falls now and
    then. upb's STRICT reader leaves the group frames to the CPU, so most neighbours sit on the
    other side."""
    rng = random.Random(8)
    bodies = {}
    shapes = ((b"m", 18, "odd"), (b"shared-2", 18, "odd"), (b"plain", 9, "none"), (b"host-only", 6, "all"))
    for mid, count, group in shapes:
        bodies[mid] = [progress_body(mid, 2, (7 * i) % 20, ASCII_WORKERS[(i // 2) % 3])
                       + (GROUP_TAIL if group == "all" or (group == "odd" and i % 2) else b"") for i in range(count)]
    turns = [mid for mid, mine in bodies.items() for _ in mine]
    rng.shuffle(turns)  # every media's bodies stay in their own order
    return frames([(PROGRESS_ID, bodies[mid].pop(0)) for mid in turns])


def shared_by_worker_stream() -> bytes:
    """ASCII ids whose events come from ASCII workers and from workers that are not: the device
    holds the first kind and the CPU the second, in both dialects. In ``first`` the CPU's frames
    open the run, in ``last`` they close it, in ``middle`` they sit inside; ``cpu-only`` has no
    event with an ASCII worker, ``dev-only`` no other. The non-ASCII workers are valid UTF-8, so upb
    decodes them too."""
    far = "nœud".encode()
    other = "ノード".encode()
    events = []
    for k in range(6):
        events.append((b"first", far if k < 2 else b"node-a", 2, 10 * k))
        events.append((b"last", far if k >= 4 else b"node-b", 2, 50 - 10 * k))
        events.append((b"middle", other if k in (2, 3) else b"node-a", 3, 10 * (k % 3)))
        events.append((b"cpu-only", far if k % 2 else other, 2, 5))
        events.append((b"dev-only", b"node-b" if k % 3 else b"", 2, 7 - k))
    return worker_stream(events)


def non_ascii_stream() -> bytes:
    """Progress events of media whose ids are not ASCII, ASCII ones in between, from a few workers:
    under protobufjs ``b"\\xff"`` and ``b"\\xfe"`` are one media (U+FFFD), under upb they do not decode."""
    rng = random.Random(4)
    ids = ["é".encode(), "メディア".encode(), b"\xff", b"\xfe", b"ok\x80", b"caf\xc3\xa9", b"ascii-1", b"ascii-2"]
    return worker_stream([(rng.choice(ids), rng.choice(ASCII_WORKERS), rng.choice((1, 2)), rng.choice((0, 5, 10, 15)))
                          for _ in range(300)])
