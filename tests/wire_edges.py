"""A systematic wire-format corpus for the telemetry readers (ops/hip/telemetry_readers.hpp) and the
per-frame headers on top of them: the host programs (test_wire_edges.py, test_hip_*_host.py) and the
device (test_gpu_wire_edges.py) read the same bodies. Nothing here is random: varints of every
length in every role at every distance from the message end, tags whose field number does not fit
32 bits, strings around the end, and groups.

The expectation per frame is defined here and nowhere else: what the service's own codec decodes
(``ops.codec_for(type, dialect).decode``, the message type chosen by the topic), or that it raises."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

from beholder_amd import ops
from beholder_amd.models import proto
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from telemetry_corpus import varint

TYPES = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}
MAX_BODIES, MAX_BYTES = 60_000, 1_000_000

VALUES = (0, 1, 5, 127, 128, 300, 2 ** 14 - 1, 2 ** 14, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 31 - 1, 2 ** 31,
          2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 35, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1)
# The share of the compared frames that a per-frame read may leave to the host. Under protobufjs
# those are the frames that decode to a string that is not ASCII; upb's STRICT reader hands over every
# frame with a group as well, which is most of what decodes here.
HOST_CAP = {"protobufjs": 0.01, "upb": 0.25}
ID = b"\x0a\x01m"  # mediaId = "m"
TAILS = (b"", b"\x10\x03", ID + b"\x10\x02\x18\x07", b"\x00", b"\x80", b"abcdef")


def tag(field: int, wire_type: int) -> bytes:
    return varint(field << 3 | wire_type)


def overlong(encoding: bytes, extra: int) -> bytes:
    """The same value with ``extra`` redundant continuation bytes."""
    if not extra:
        return encoding
    return encoding[:-1] + bytes([encoding[-1] | 0x80]) + b"\x80" * (extra - 1) + b"\x00"


@functools.lru_cache(maxsize=None)
def encodings() -> tuple:
    out = [overlong(varint(v), extra) for v in VALUES for extra in (0, 1, 2)]
    for k in range(1, 12):
        out += [b"\xff" * k + b"\x01", b"\x80" * k + b"\x00"]
    out += [b"\xff" * k + b"\x7f" for k in (4, 9, 10)]
    return tuple(dict.fromkeys(e for e in out if len(e) <= 11))


def roles() -> tuple:
    """The bytes before a varint, per role the varint then plays."""
    out = [b"", ID]                                                              # a tag
    out += [tag(f, wt) for f in range(7) for wt in (0, 2)]                       # a value or a length
    out += [tag(f, wt) for f in (2, 3) for wt in (1, 3, 4, 5, 6, 7)]             # whatever follows that tag
    out += [b"\x2b", b"\x2b\x08", b"\x2b\x0a"]                                   # in a group: tag, value, length
    return tuple(out)


def _cuts(before: bytes, rest: bytes):
    return (before + rest[:k] for k in range(len(rest) + 1))


def _varint_family():
    for before in roles():
        for e in encodings():
            for tail in TAILS:
                yield from _cuts(before, e + tail)


def _wide_tag_family():
    """Field numbers past 32 bits (plain upb must not take 2^32 + k for field k) and past the 29
    bits a 32-bit key has (protobufjs does take 2^29 + k for field k)."""
    payload = {0: b"\x05", 2: b"\x01m"}
    for base in (2 ** 32, 2 ** 29):
        for k in range(6):
            for wt in (0, 2):
                for extra in (0, 1):
                    t = overlong(tag(base + k, wt), extra)
                    for before in (b"", ID):
                        for tail in (b"", b"\x10\x03"):
                            yield from _cuts(before, t + payload[wt] + tail)
    for field in (2 ** 29 - 1, 2 ** 29):
        for wt in range(8):
            yield tag(field, wt) + payload.get(wt, b"") + ID


def _tag_family():
    """Every tag of wire types 0..7 and fields 0..6 in front of each kind of payload."""
    for field in range(7):
        for wt in range(8):
            for payload in (b"", b"\x05", b"\x01m", b"\x01\x02\x03\x04", bytes(range(8))):
                yield tag(field, wt) + payload
                yield tag(field, wt) + payload + ID


def _string_family():
    text = b"abcdef"
    for field in (1, 4, 5):
        for present in range(7):
            for n in (0, 1, present - 1, present, present + 1, 127, 128, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1):
                if n < 0:
                    continue
                for extra in (0, 1):
                    b = tag(field, 2) + overlong(varint(n), extra) + text[:present]
                    yield b
                    yield ID + b
                    if n == present:
                        yield b + b"\x10\x03"
    for field in (1, 4):
        for s in (b"\x80", b"\xffab", b"ab\xff", b"\xc3\xa9", b"a\xc3\xa9", b"\xc3\xa9a", b"\xe3\x83\xa1", b"\xc3"):
            b = tag(field, 2) + varint(len(s)) + s
            yield b
            yield b + b"\x10\x03"
            yield b"\x10\x03" + b
            if field == 4:
                yield ID + b
    yield b"\x0a\x00"
    yield b"\x0a\x00\x10\x03\x18\x07"


def _group_family():
    inner_payloads = (b"", b"\x10\x03", b"\x0a\x01x", b"\x3d\x01\x02\x03\x04", b"\x39" + bytes(range(8)), b"\x3e")
    for depth in range(4):
        starts = b"".join(tag(5 + d, 3) for d in range(depth))
        for ends in range(depth + 2):
            # the tags that close what was opened, innermost first, and one more; field 9 closes nothing here
            matching = b"".join(tag(5 + d, 4) for d in list(reversed(range(depth))) + [0])
            variants = {matching[:ends], (b"\x4c" + matching[1:])[:ends], (matching[:-1] + b"\x4c")[:ends]}
            for close in sorted(variants):
                for inner in inner_payloads:
                    g = starts + inner + close
                    yield g
                    yield ID + g
                    yield g + ID


@functools.lru_cache(maxsize=None)
def bodies() -> tuple:
    """Every body of the corpus, sorted and without repeats."""
    out = set()
    for family in (_varint_family, _wide_tag_family, _tag_family, _string_family, _group_family):
        out.update(family())
    out = tuple(sorted(out))
    assert len(out) <= MAX_BODIES and sum(map(len, out)) <= MAX_BYTES, (len(out), sum(map(len, out)))
    return out


@functools.lru_cache(maxsize=None)
def picked(limit: Optional[int] = None) -> tuple:
    """Every k-th body of the sorted list, so that every family stays in, for at most ``limit`` frames."""
    all_bodies = bodies()
    if limit is None:
        return all_bodies
    k = max(1, -(-2 * len(all_bodies) // limit))
    return all_bodies[::k]


@functools.lru_cache(maxsize=None)
def events(limit: Optional[int] = None) -> tuple:
    """``(topic, body)`` per frame of ``stream(limit)``: every body as a status, then as a progress."""
    return tuple((topic, b) for b in picked(limit) for topic in (STATUS_ID, PROGRESS_ID))


@functools.lru_cache(maxsize=None)
def stream(limit: Optional[int] = None) -> bytes:
    return frames(list(events(limit)))


class Values(NamedTuple):
    """What the codec decoded; ``progress`` and ``host`` are 0 and "" for a TelemetryStatus."""
    media_id: str
    status: int
    progress: int
    host: str


def decode(topic: int, body: bytes, dialect: str) -> Optional[Values]:
    """The service codec's reading of one frame: its values, or None where it raises."""
    try:
        m = ops.codec_for(TYPES[topic], dialect).decode(body)
    except proto.DecodeError:
        return None
    return Values(m.mediaId, m.status, getattr(m, "progress", 0), getattr(m, "host", ""))


@functools.lru_cache(maxsize=None)
def expected(dialect: str, limit: Optional[int] = None) -> tuple:
    """``decode`` of every frame of ``stream(limit)``."""
    return tuple(decode(topic, b, dialect) for topic, b in events(limit))


def selector():
    """An extract selector that keeps by media and by status: a frame's fate hangs on both values."""
    from beholder_amd.extract import Selector
    return Selector(media={"m", "", "abcdef", "x", "é"}, statuses={0, 3, 5}, unknown_status=True)


def id_hash(values: Values) -> int:
    """The hash the device files the frame's media under (ids the device decides are ASCII)."""
    from beholder_amd.ops import gpu_fold
    return gpu_fold.hash64(values.media_id.encode("utf-8"))
