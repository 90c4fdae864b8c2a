"""Policies and streams shared by the tests of ``compare``: the definition (test_compare.py), the
per-frame and per-position code compiled for the host (test_hip_compare_host.py) and the device
path (test_gpu_compare.py)."""
from __future__ import annotations

import functools
import random

from beholder_amd.compare import Policy
from beholder_amd.ops import frame, frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames
from dedupe_cases import TOPIC_SETS, capped_stream, corpus, edge_stream, mixed_stream
from telemetry_corpus import body

POLICIES = [Policy(t) for t in TOPIC_SETS]
assert POLICIES[0] == Policy() and len(POLICIES) == 4


def policy_id(policy: Policy) -> str:
    return "all" if policy.topics is None else "+".join(map(str, sorted(policy.topics)))


def pieces(data: bytes) -> list:
    """The frames of a stream, each as its own bytes."""
    return [frame(t, b) for t, b in iter_frames(data)]


def contents(data: bytes, policy: Policy = Policy()) -> list:
    """The contents (topic byte and body) of the frames that take part, in stream order."""
    return [bytes([t]) + b for t, b in iter_frames(data) if policy.takes_part(t)]


def shuffled(data: bytes, seed: int = 5) -> bytes:
    parts = pieces(data)
    random.Random(seed).shuffle(parts)
    return b"".join(parts)


def copies(count: int, status: int = 5) -> bytes:
    """One content ``count`` times."""
    return frames([(STATUS_ID, body(b"m", status))] * count)


def distinct(count: int, start: int = 0) -> bytes:
    """``count`` frames of pairwise distinct contents, on both topics."""
    return frames([(STATUS_ID if k % 3 else PROGRESS_ID, body(b"media-%07d" % k, k % 5))
                   for k in range(start, start + count)])


@functools.lru_cache(maxsize=None)
def capped_pair(cap: int) -> tuple:
    """``(A, B)`` with contents of exactly ``cap`` and ``cap + 1`` bytes on both sides: B is A
    shuffled, without the first frame above the cap, and with one content above the cap that A does
    not have. So contents above the cap are matched across the captures and out of order, one is
    only in A and one only in B."""
    a = capped_stream(cap)
    parts = pieces(shuffled(a, 11))
    first_over = next(k for k, p in enumerate(parts) if len(p) - 4 > cap)
    del parts[first_over]
    parts.insert(3, frame(STATUS_ID, random.Random(12).randbytes(cap)))
    return a, b"".join(parts)


def over_cap(data: bytes, policy: Policy, cap: int) -> int:
    """The participating frames of ``data`` whose content is longer than ``cap``."""
    return sum(policy.takes_part(t) and 1 + len(b) > cap for t, b in iter_frames(data))


@functools.lru_cache(maxsize=None)
def small_pairs() -> dict:
    """Named ``(A, B)`` pairs of a few hundred frames at the most: repeats on both sides in unequal
    numbers, frames of one side only, every topic, bodies of every short length."""
    mixed, edge = mixed_stream(), edge_stream()
    parts = pieces(mixed)
    fewer = b"".join(parts[::2])
    return {
        "mixed-itself": (mixed, mixed),
        "mixed-shuffled": (mixed, shuffled(mixed)),
        "mixed-half": (mixed, fewer),
        "half-mixed": (fewer, mixed),
        "mixed-edge": (mixed, edge),
        "edge-twice": (edge, shuffled(edge + edge, 7)),
        "copies-3-5": (copies(3), copies(5)),
        "copies-and-others": (copies(4) + distinct(6) + copies(2, 4), distinct(9, 3) + copies(5) + copies(3, 4)),
        "disjoint": (distinct(20), distinct(20, 100)),
        "empty-a": (b"", mixed),
        "empty-b": (mixed, b""),
        "empty-both": (b"", b""),
    }


__all__ = ["POLICIES", "TOPIC_SETS", "policy_id", "pieces", "contents", "shuffled", "copies", "distinct",
           "capped_pair", "over_cap", "small_pairs", "corpus"]
