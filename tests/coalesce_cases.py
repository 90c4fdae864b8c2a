"""Policies and streams shared by the tests of ``coalesce``: the definition (test_coalesce.py), the
decision compiled for the host (test_hip_coalesce_host.py) and the device path (test_gpu_coalesce.py)."""
from __future__ import annotations

import itertools
import random

from beholder_amd.coalesce import PROGRESS_MODES, STATUS_MODES, UNDECODED_MODES, Policy
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from telemetry_corpus import body

# every policy there is, 16 of them; the default comes first
POLICIES = [Policy(s, p, u) for s, p, u in itertools.product(STATUS_MODES, PROGRESS_MODES, UNDECODED_MODES)]
assert POLICIES[0] == Policy() and len(POLICIES) == 16


def policy_id(policy: Policy) -> str:
    return f"{policy.status}-{policy.progress}-{policy.undecoded}"


def mixed_events() -> list:
    """60 events: five media (one with no id, one whose id is not ASCII) on both topics with
    statuses 0-3, 64 and -1, bodies that fail to decode on either topic, and other topic bytes."""
    rng = random.Random(21)
    ids = [b"m-1", b"m-2", b"", "é".encode(), b"m-10"]
    events = [(rng.choice((STATUS_ID, PROGRESS_ID)), body(rng.choice(ids), rng.choice((0, 1, 2, 3, 64, -1))))
              for _ in range(48)]
    events += [(STATUS_ID, b"\x2e"), (PROGRESS_ID, b"\x2e"), (STATUS_ID, b"\x0a\x05m"), (PROGRESS_ID, b"\x2f\x00"),
               (9, body(b"m-1", 1)), (0, b""), (255, body(b"m-2", 2)), (3, b"\x2e"),
               (STATUS_ID, b""), (PROGRESS_ID, b""), (STATUS_ID, body(b"m-1", 5)), (PROGRESS_ID, body(b"m-1", 5))]
    rng.shuffle(events)
    return events


def mixed_stream() -> bytes:
    return frames(mixed_events())
