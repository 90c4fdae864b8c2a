"""Byte strings for the tests of the telemetry readers (ops/hip/telemetry_readers.hpp): the batched
decode (test_gpu_decode.py), the stream fold (test_gpu_fold.py) and the readers compiled for the
host (test_hip_readers_host.py). Seeds and order are fixed: both corpora are the same bytes on
every run."""
from __future__ import annotations

import functools
import random

from beholder_amd import ops
from beholder_amd.bench.generator import Workload
from beholder_amd.models import proto
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

STATUS = ops.codec_for(proto.load("api.TelemetryStatus"))


def varint(v: int) -> bytes:
    v &= (1 << 64) - 1
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def body(mid: bytes, status: int) -> bytes:
    """mediaId and status, valid as either message type; status may be any int32."""
    return b"\x0a" + varint(len(mid)) + mid + b"\x10" + varint(status)


MALFORMED = [
    b"\x00\x05",                         # field 0 (varint): skipped by protobufjs, an error for upb
    b"\x02\x01x\x0a\x02ok",             # field 0 length-delimited, then mediaId
    b"\x08\x07",                         # mediaId tagged as a varint: read as a string of length 7
    b"\x10\x03abc",                      # ... status tagged fine
    b"\x15\x05\x00\x00\x00",           # status with wire type 5: read as a varint anyway
    b"\x1a\x2a",                         # progress with wire type 2: varint 42
    b"\x0a\x7fabc",                      # mediaId of 127 bytes in a 5-byte body: clamped
    b"\x22\xff\xff\xff\xff\x0fhost",  # host length 2^32-1: clamped
    b"\x18\xff\xff\xff\xff\xff\x01\x00\x00\x00\x00",  # 10-byte progress varint
    b"\x18\xff\xff\xff\xff\xff",       # ... truncated inside the unchecked tail
    b"\x80\x80\x80\x80\x80",           # 5-byte tag with continuation: tail past the end
    b"\x2b\x08\x01\x2c\x0a\x01z",     # a group (field 5) around a varint, then mediaId
    b"\x2b\x33\x08\x01\x34\x2c",      # nested groups
    b"\x2c",                              # end-group with nothing open
    b"\x2e", b"\x2f\x00",                # wire types 6 / 7
    b"\x0a\x03\xff\xfe\xfd",           # invalid UTF-8 (protobufjs: U+FFFD)
    b"\x0a\x02ab\x0a\x01c\x10\x01\x10\x02",  # repeated scalars: last wins
    b"\x39" + bytes(7),                   # unknown fixed64 one byte short
    b"\x3d\x01\x02\x03",                # unknown fixed32 one byte short
]

# what the fold adds: the two message types apart, and where upb's STRICT reader differs from the plain one
MALFORMED_FOLD = MALFORMED + [
    b"\x1a\x02\x10\x04", b"\x22\x01",    # fields 3 / 4: known to a progress, unknown to a status
    b"\x0a\x01m\x22\x02\xc3\x28",      # a host that is not UTF-8 (upb raises, for a progress only)
    b"\x8a\x80\x80\x80\x10\x01m",       # a 5-byte tag above 32 bits (upb: tag overflow)
    b"\x8a\x80\x80\x80\x80\x00\x01m",  # a 6-byte tag (upb: too long)
    b"\x0a\x01m\x10" + b"\xff" * 9 + b"\x01",  # a 10-byte status varint
    b"\x0a\x01m\x10" + b"\xff" * 10 + b"\x01",  # ... and an 11-byte one
]


def malformed(rng: random.Random, fixed=MALFORMED) -> list:
    """Where protobufjs and upb disagree: field 0, known fields with the wrong wire type, strings
    running past the end (clamped by protobufjs), 5-byte and overlong varints, groups, invalid
    UTF-8, and a tag varint truncated in its 5th byte; then 400 random bodies."""
    out = list(fixed)
    for _ in range(400):  # random bodies built from tags of every field number 0-6 and wire type
        b = bytearray()
        for _ in range(rng.randrange(1, 6)):
            b.append((rng.randrange(7) << 3) | rng.randrange(8))
            b += bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 6)))
        out.append(bytes(b))
    return out


def decode_corpus(rng: random.Random) -> list:
    """Message bodies for the batched decode: workload events, statuses, truncations, garbage,
    unknown fields, the malformed list, empty."""
    w = Workload(n_media=64, seed=5)
    bodies = [b for _, b in w.events(3000)]
    bodies += [STATUS.encode({"mediaId": f"m{i}", "status": i % 7}) for i in range(200)]
    for _ in range(500):  # truncations, garbage, unknown fields, empty
        b = rng.choice(bodies)
        bodies.append(b[:rng.randrange(len(b) + 1)])
        bodies.append(bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 30))))
        bodies.append(b + bytes([0x28, rng.randrange(128), 0x35, 1, 2, 3, 4, 0x39]) + bytes(8))
    bodies += malformed(rng)
    bodies.append(b"")
    return bodies


@functools.lru_cache(maxsize=None)
def fold_corpus() -> bytes:
    """About 3,000 workload events over 64 media on both topics, then every kind of malformed body
    on both topics, unknown topic bytes, and status numbers 6, 63, 64 and -1; shuffled."""
    rng = random.Random(11)
    w = Workload(n_media=64, seed=5, progress_fraction=0.7)
    events = w.events(3000)
    bodies = [b for _, b in events]
    odd = []
    for _ in range(300):  # truncations, garbage, unknown fields
        b = rng.choice(bodies)
        odd.append(b[:rng.randrange(len(b) + 1)])
        odd.append(bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 30))))
        odd.append(b + bytes([0x28, rng.randrange(128), 0x35, 1, 2, 3, 4, 0x39]) + bytes(8))
    odd += malformed(rng, MALFORMED_FOLD) + [b""]
    ids = [m.id.encode() for m in w.media]
    for status in (6, 63, 64, -1):
        odd += [body(rng.choice(ids), status) for _ in range(5)]
    for b in odd:
        events += [(STATUS_ID, b), (PROGRESS_ID, b)]
    events += [(t, rng.choice(bodies)) for t in (0, 3, 4, 127, 255) for _ in range(3)]
    rng.shuffle(events)
    return frames(events)
