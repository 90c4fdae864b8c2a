"""Policies and streams shared by the tests of ``dedupe``: the definition (test_dedupe.py), the
per-frame code compiled for the host (test_hip_dedupe_host.py) and the device path
(test_gpu_dedupe.py)."""
from __future__ import annotations

import functools
import itertools
import random

from beholder_amd.dedupe import KEEP_MODES, Policy
from beholder_amd.ops import frame, frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from coalesce_cases import mixed_events
from telemetry_corpus import body, fold_corpus

# all topics, each of the two the service reads, and one that no frame of the corpus carries
TOPIC_SETS = (None, frozenset({STATUS_ID}), frozenset({PROGRESS_ID}), frozenset({7}))
POLICIES = [Policy(k, t) for k, t in itertools.product(KEEP_MODES, TOPIC_SETS)]
assert POLICIES[0] == Policy() and len(POLICIES) == 8
WIDE_LENGTHS = (3, 4, 5, 7, 8, 9)  # content lengths around the wide forms' 8-byte step


def policy_id(policy: Policy) -> str:
    return f"{policy.keep}-" + ("all" if policy.topics is None else "+".join(map(str, sorted(policy.topics))))


@functools.lru_cache(maxsize=None)
def corpus() -> bytes:
    return fold_corpus()


# contents that differ in one place only, a strict prefix, and the shortest bodies there are
EDGE_EVENTS = [
    (STATUS_ID, b"abcdefghij"), (PROGRESS_ID, b"abcdefghij"),  # differ in the topic byte only
    (STATUS_ID, b"abcdefghik"),                                # ... in the last byte only
    (STATUS_ID, b"Xbcdefghij"),                                # ... in the first body byte only
    (STATUS_ID, b"abcdefghi"), (STATUS_ID, b"abcdefgh"),       # strict prefixes, one ending on the 8-byte step
    (STATUS_ID, b"a"), (STATUS_ID, b"b"), (PROGRESS_ID, b"a"),  # one-byte bodies
    (STATUS_ID, b""), (PROGRESS_ID, b""), (7, b""), (7, b"a"),  # no body at all; a third topic
]


def edge_stream() -> bytes:
    """Every edge event three times, shuffled."""
    events = EDGE_EVENTS * 3
    random.Random(3).shuffle(events)
    return frames(events)


def aligned_stream() -> bytes:
    """Contents of 3, 4, 5, 7, 8 and 9 bytes, each with a twin that differs in its last byte, each
    starting once at every offset mod 8 of the stream: a frame of its own content in front of each
    shifts it there. So every content occurs 8 times, and equal contents meet at every pair of
    alignments."""
    out = bytearray()
    pad = 0
    for length in WIDE_LENGTHS:
        base = bytes(range(0x41, 0x41 + length - 1))
        for content in (base, base[:-1] + bytes([base[-1] ^ 1])):
            for shift in range(8):
                filler = (shift - (len(out) + 4) - 5) % 8 + 8  # the pad frame is 5 + filler bytes
                out += frame(9, bytes([pad]) * filler)
                pad += 1
                assert (len(out) + 4) % 8 == shift
                out += frame(STATUS_ID, content)
    assert pad == 96
    return bytes(out)


def mixed_stream() -> bytes:
    """The coalesce's small stream of every kind of frame, a third of it again, and the edge events
    twice: some hundred frames with repeats on every topic, for the merge at every boundary."""
    events = mixed_events()
    return frames(events + EDGE_EVENTS + events[::3] + EDGE_EVENTS[::-1])


def three_statuses() -> bytes:
    """One media going QUEUED, ERRORED, QUEUED: two equal status frames around a different one."""
    from beholder_amd import replay
    numbers = {name: number for number, name in replay.status_names().items()}
    return frames([(STATUS_ID, body(b"m-1", numbers[name])) for name in ("QUEUED", "ERRORED", "QUEUED")])


def capped_stream(cap: int) -> bytes:
    """Contents of exactly ``cap`` and ``cap + 1`` bytes, each three times, and twins of them that
    differ in the last byte, among short frames."""
    rng = random.Random(8)
    at = rng.randbytes(cap - 1)
    over = rng.randbytes(cap)
    big = [(STATUS_ID, at), (STATUS_ID, over)] * 3 + [(STATUS_ID, at[:-1] + b"\x00"), (STATUS_ID, over[:-1] + b"\x00"),
                                                     (PROGRESS_ID, over), (PROGRESS_ID, at)]
    events = big + [(rng.choice((STATUS_ID, PROGRESS_ID)), body(b"m-%d" % rng.randrange(4), rng.randrange(3)))
                    for _ in range(40)]
    rng.shuffle(events)
    return frames(events)
