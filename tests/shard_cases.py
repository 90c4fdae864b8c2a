"""Policies and streams shared by the tests of ``shard``: the definition (test_shard.py), the decision
compiled for the host (test_hip_shard_host.py) and the device path (test_gpu_shard.py)."""
from __future__ import annotations

import functools
import itertools
import random

from beholder_amd.ops import frames
from beholder_amd.shard import UNDECODED_MODES, Policy
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from coalesce_cases import mixed_stream  # noqa: F401  re-exported: the small stream of every kind of frame
from extract_cases import collision_pairs
from telemetry_corpus import body, fold_corpus

# one shard, a few, a count that is no power of two, a prime, one wave's worth, and both ends of the top
SHARD_COUNTS = (1, 2, 3, 7, 64, 255, 256)
POLICIES = [Policy(n, u) for n, u in itertools.product(SHARD_COUNTS, UNDECODED_MODES)]
assert POLICIES[0] == Policy(1) and len(POLICIES) == 14


def policy_id(policy: Policy) -> str:
    return f"{policy.shards}-{policy.undecoded}"


@functools.lru_cache(maxsize=None)
def corpus() -> bytes:
    return fold_corpus()


def pairs_stream() -> bytes:
    """720 events over 120 ids that differ from a neighbour in the last byte only, on both topics,
    shuffled: the shard depends on the whole id."""
    rng = random.Random(1)
    events = [(topic, body(mid, rng.randrange(6))) for pair in collision_pairs() for mid in pair
              for topic in (STATUS_ID, PROGRESS_ID) for _ in range(3)]
    rng.shuffle(events)
    return frames(events)
