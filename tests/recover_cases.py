"""Streams and damages for the ``recover`` tests (tests/test_recover.py, tests/test_hip_recover_host.py,
tests/test_gpu_recover.py): small hand-made captures whose frames hold at most 64 bytes, so that they
can be walked under ``max_frame`` 64 as well as 1,024, and the two corpora, intact and damaged."""
from __future__ import annotations

import functools
import random
import struct
from typing import Dict, List, Tuple

from beholder_amd.capture_io import frame_spans
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

import wire_edges
from telemetry_corpus import fold_corpus, varint

CORPORA = ("fold_corpus", "wire_edges")
MAX_FRAMES = (64, 1024)
GROUP = b"\x2b\x08\x01\x2c"  # a start-group, a varint field inside, its end-group
JUNK = b"\xff" * 7           # no header fits in it: every length is above any max_frame


def frame(topic: int, body: bytes) -> bytes:
    return struct.pack("<IB", 1 + len(body), topic) + body


def _str(field: int, value: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(value)) + value


def status(mid: bytes = b"m-1", number: int = 2) -> bytes:
    return frame(STATUS_ID, _str(1, mid) + b"\x10" + varint(number))


def progress(mid: bytes = b"m-1", number: int = 2, percent: int = 50, host: bytes = b"h") -> bytes:
    return frame(PROGRESS_ID, _str(1, mid) + b"\x10" + varint(number) + b"\x18" + varint(percent) + _str(4, host))


MINIMAL = frame(9, b"")                    # 5 bytes: the shortest frame there is
EMPTY_ID = frame(STATUS_ID, b"\x10\x02")   # decodes, and its mediaId is empty
OTHER_TOPIC = frame(9, b"\x0a\x03m-1")     # would be an anchor under topic 1
UNDECODABLE = frame(PROGRESS_ID, b"\x0a\x05m")  # a string that runs past the end: an error under upb, clamped under protobufjs
BROKEN = frame(STATUS_ID, b"\x0a\x01m\x2e")     # wire type 6: an error in either dialect


def five() -> List[bytes]:
    return [status(b"m-%d" % k, k) if k % 2 else progress(b"m-%d" % k, k, 10 * k) for k in range(5)]


def starts(parts: List[bytes]) -> List[int]:
    out, at = [], 0
    for part in parts:
        out.append(at)
        at += len(part)
    return out


def damage_cases() -> Dict[str, bytes]:
    """Name -> buffer. Every frame in them holds at most 64 bytes."""
    f = five()
    whole = b"".join(f)
    rng = random.Random(11)
    noise = bytes(rng.randrange(256) for _ in range(900))
    cases = {
        "intact": whole,
        "one_frame": f[0],
        "minimal_frames": MINIMAL * 7,
        "torn_inside_the_last_body": whole[:-3],
        "torn_inside_the_last_header": whole[:len(whole) - len(f[4]) + 2],
        "ends_exactly_at_n": whole + frame(9, b"x" * 63),
        "would_end_at_n_plus_1": whole + frame(9, b"x" * 63)[:-1],
        "length_0": f[0] + struct.pack("<I", 0) + b"\x01" + f[1] + f[2],
        "length_max_frame_64": f[0] + frame(9, b"y" * 63) + f[1],
        "length_max_frame_64_plus_1": f[0] + frame(9, b"y" * 64) + f[1] + f[2],
        "zeros": f[0] + bytes(40) + f[1] + f[2],
        "garbage_at_0": JUNK + whole,
        "garbage_only": JUNK * 5,
        "noise_only": noise[:200],
        "two_gaps_one_frame_between": f[0] + JUNK + f[1] + f[2] + JUNK * 2 + f[3] + f[4],
        # the first candidate behind the gap is followed by damage again: not an anchor, the next one is taken
        "anchor_with_a_damaged_successor": f[0] + JUNK + f[1] + JUNK + f[2] + f[3],
        "in_sync_frames_that_are_no_anchor": f[0] + EMPTY_ID + OTHER_TOPIC + UNDECODABLE + BROKEN + f[1],
        "no_anchor_among_the_candidates": f[0] + JUNK + EMPTY_ID + OTHER_TOPIC + BROKEN + f[1] + f[2],
        "gap_longer_than_two_chunks": f[0] + f[1] + noise + f[2] + f[3] + f[4],
        "long_intact_run": whole * 40,
        "damage_in_a_long_run": whole * 12 + JUNK + whole * 12 + b"\x00" + whole * 12,
        "a_damaged_length_that_still_fits": f[0] + struct.pack("<IB", 20, STATUS_ID) + f[1][5:] + f[2] + f[3] + f[4],
        "non_ascii_id": f[0] + JUNK + status("é".encode()) + f[1] + JUNK + status(b"\xff\xfe") + f[2],
        "group_behind_a_gap": f[0] + JUNK + frame(STATUS_ID, _str(1, b"m") + GROUP) + f[1] + f[2],
        "non_ascii_host": f[0] + JUNK + progress(b"m", 1, 2, "hôte".encode()) + f[1] + JUNK + progress(b"m", 1, 2, b"\xff") + f[2],
    }
    return cases


@functools.lru_cache(maxsize=None)
def corpus(name: str) -> bytes:
    return fold_corpus() if name == "fold_corpus" else wire_edges.stream(6000)


@functools.lru_cache(maxsize=None)
def damaged(name: str) -> Tuple[bytes, int]:
    """``(buffer, k)``: the corpus of ``k`` frames with four damages, placed from its true spans: the
    first header byte of frame ``3k // 4`` XORed with 0x04, 300 bytes of ``random.Random(7)`` before
    frame ``k // 2``, the bytes from 3 into frame ``k // 4`` to 1 into frame ``k // 4 + 2`` deleted,
    and the last 3 bytes dropped."""
    data = bytearray(corpus(name))
    spans = list(frame_spans(bytes(data)))
    k = len(spans)
    data[spans[3 * k // 4][0]] ^= 0x04
    rng = random.Random(7)
    at = spans[k // 2][0]
    data[at:at] = bytes(rng.randrange(256) for _ in range(300))
    del data[spans[k // 4][0] + 3:spans[k // 4 + 2][0] + 1]
    del data[-3:]
    return bytes(data), k
