"""The gfx950 normalise kernels' per-frame code (ops/hip/telemetry_normalise.hpp: the plan, the
canonical length and every canonical byte) on a CPU, under ASan and UBSan.

tests/native/normalise_host.cpp compiles the header for the host and plans every frame of a stream
from a heap block of exactly the frame's size: a read past it is a sanitizer report here. Its output
frames, put together from ``canon_byte`` one byte at a time, are held to ``normalise.canon_of`` and
the service's codec on both topics, in both dialects and under both policies; the frames it leaves
to the host are exactly the rule's; and no frame grows by more than ``NM_GROWTH_MAX`` (the program
checks that itself). Nothing is loaded into Python under a sanitizer."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

from beholder_amd import normalise as nm, ops
from beholder_amd.coalesce import DROP, KEEP
from beholder_amd.models import proto
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus, varint  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
TYPES = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}
HOST_SHARE_MAX = 0.10  # of the fold corpus, in either dialect
POLICIES = ("keep", "drop")


def growth_max() -> int:
    with open(os.path.join(HIP, "telemetry_normalise.hpp"), encoding="utf-8") as f:
        return int(re.search(r"constexpr int NM_GROWTH_MAX = (\d+);", f.read()).group(1))


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_thin_host.py."""
    out = str(tmp_path_factory.mktemp("normalise_host") / "normalise_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "normalise_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _lines(program: str, dialect: str, stream: bytes, undecoded: str, tmp_path) -> list:
    """The program's line per frame of ``stream``; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, dialect, str(path), undecoded], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _high(b: bytes) -> bool:
    return any(c >= 0x80 for c in b)


def _rule_protobufjs(topic: int, body: bytes) -> bool:
    """A decoded frame with a string that is not ASCII. Every byte >= 0x80 of a span decodes to a
    character that is not ASCII (U+FFFD where it is no UTF-8), so the decoded string tells."""
    if topic not in TYPES:
        return False
    try:
        m = ops.codec_for(TYPES[topic], "protobufjs").decode(body)
    except proto.DecodeError:
        return False
    return not m.mediaId.isascii() or (topic == PROGRESS_ID and not m.host.isascii())


def _rule_upb(topic: int, body: bytes) -> bool:
    """The STRICT upb walk, written out on its own: the first start-group hands the frame over; so do
    the last id span and, in a progress message, the last host span of a message that is read to
    its end, where one holds a byte >= 0x80. An error on the way decides the frame on the device."""
    if topic not in TYPES:
        return False
    spans = {}
    i, end = 0, len(body)

    def read(limit):
        nonlocal i
        v = 0
        for k in range(limit):
            if i >= end:
                return None
            b = body[i]
            i += 1
            v |= (b & 0x7f) << (7 * k)
            if not b & 0x80:
                return v
        return None
    while i < end:
        key = read(5)
        if key is None or key > 0xFFFFFFFF or key >> 3 == 0:
            return False
        field, wt = key >> 3, key & 7
        if wt == 0:
            if read(10) is None:
                return False
        elif wt == 2:
            n = read(10)
            if n is None or n > end - i:
                return False
            if field == 1 or (topic == PROGRESS_ID and field == 4):
                spans[field] = body[i:i + n]
            i += n
        elif wt in (1, 5):
            if end - i < (8 if wt == 1 else 4):
                return False
            i += 8 if wt == 1 else 4
        else:
            return wt == 3
    return any(_high(s) for s in spans.values())


RULES = {"protobufjs": _rule_protobufjs, "upb": _rule_upb}


def _against_the_definition(stream: bytes, got: list, dialect: str, undecoded: str) -> dict:
    """Asserts every line; returns the frames per kind of line."""
    canon = nm.canon_of(nm.Policy(undecoded), dialect)
    events = list(iter_frames(stream))
    assert len(got) == len(events)
    kinds = {"copy": set(), "drop": set(), "host": set(), "status": set(), "progress": set()}
    bad = []
    cap = growth_max()
    for i, ((topic, body), line) in enumerate(zip(events, got)):
        word = line.split()
        kinds[word[0]].add(i)
        if word[0] == "host":
            continue
        c = canon(topic, body)
        if c is DROP:
            want = ["drop"]
        elif c is KEEP:
            want = ["copy", nm.frame_of(topic, body).hex(), "0"]
        else:
            want = [{STATUS_ID: "status", PROGRESS_ID: "progress"}[topic], nm.frame_of(topic, c).hex(),
                    str(len(c) - len(body))]
            assert len(c) - len(body) <= cap
        if word != want:
            bad.append((i, topic, body, line, want))
    assert not bad, (len(bad), bad[:5])
    rule = RULES[dialect]
    assert kinds["host"] == {i for i, (topic, body) in enumerate(events) if rule(topic, body)}
    return kinds


@pytest.mark.parametrize("undecoded", POLICIES)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_frame_of_the_fold_corpus(program, tmp_path, dialect, undecoded):
    stream = fold_corpus()
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, undecoded, tmp_path), dialect, undecoded)
    frames_ = sum(map(len, kinds.values()))
    assert frames_ > 5000 and kinds["status"] and kinds["progress"] and kinds["copy" if undecoded == "keep" else "drop"]
    assert not kinds["drop" if undecoded == "keep" else "copy"]
    print(f"{dialect}: {len(kinds['host'])} of {frames_} frames left to the host")
    assert 0 < len(kinds["host"]) <= HOST_SHARE_MAX * frames_


@pytest.mark.parametrize("undecoded", POLICIES)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_frame_of_the_wire_edges(program, tmp_path, dialect, undecoded):
    stream = wire_edges.stream(6000)
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, undecoded, tmp_path), dialect, undecoded)
    assert len(kinds["status"]) + len(kinds["progress"]) > 300
    print(f"{dialect}: {len(kinds['host'])} of {sum(map(len, kinds.values()))} frames left to the host")


def _int(field: int, value: int) -> bytes:
    return varint(field << 3) + varint(value & 0xFFFFFFFFFFFFFFFF)


def _str(field: int, value: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(value)) + value


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_frames_that_grow_and_the_lengths_where_a_varint_steps(program, tmp_path, dialect):
    """Both int32 fields negative from 5-byte varints is the frame that reaches NM_GROWTH_MAX; string
    lengths step the head at 128 and 16,384; INT_MIN, INT_MAX and -1 through both writers."""
    minus = b"\xff\xff\xff\xff\x0f"  # 0xffffffff in 5 bytes: -1 as an int32
    bodies = [b"\x10" + minus + b"\x18" + minus, b"\x10" + minus, b"\x18" + minus]
    bodies += [_int(2, v) + _int(3, w) for v in (-1, -2 ** 31, 2 ** 31 - 1, 127, 128) for w in (-1, -2 ** 31, 1, 2 ** 14)]
    bodies += [_str(1, b"i" * n) + _str(4, b"h" * k) for n in (0, 1, 127, 128, 16383, 16384) for k in (0, 127, 128)]
    bodies += [_str(4, b"h") + _int(3, 7) + _int(2, 0) + _str(1, b"m") + _int(2, 3), b""]
    stream = frames([(topic, body) for body in bodies for topic in (STATUS_ID, PROGRESS_ID)])
    got = _lines(program, dialect, stream, "keep", tmp_path)
    kinds = _against_the_definition(stream, got, dialect, "keep")
    assert not kinds["host"] and not kinds["copy"]
    assert got[2].split()[2] == "5" and got[1].split()[2] == str(growth_max()) == "10"  # status alone; both
    assert max(int(line.split()[2]) for line in got) == growth_max()


def test_a_group_goes_to_the_host_under_upb_only(program, tmp_path):
    body = _str(1, b"m") + b"\x2b\x08\x01\x2c" + _int(2, 3)
    stream = frames([(STATUS_ID, body), (PROGRESS_ID, body)])
    assert _lines(program, "upb", stream, "keep", tmp_path) == ["host", "host"]
    _against_the_definition(stream, _lines(program, "upb", stream, "keep", tmp_path), "upb", "keep")
    kinds = _against_the_definition(stream, _lines(program, "protobufjs", stream, "keep", tmp_path), "protobufjs", "keep")
    assert kinds["status"] == {0} and kinds["progress"] == {1}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_a_string_that_is_not_ascii_goes_to_the_host(program, tmp_path, dialect):
    """An id or a host, valid UTF-8 or not; the host field of a status message is an unknown field."""
    events = [(PROGRESS_ID, _str(1, "é".encode())), (PROGRESS_ID, _str(1, b"m") + _str(4, b"\xff")),
              (STATUS_ID, _str(1, b"\x80")), (STATUS_ID, _str(1, b"m") + _str(4, b"\xff")),
              (PROGRESS_ID, _str(1, b"\xc3\xa9") + _str(1, b"m"))]  # the last id wins, and it is ASCII
    stream = frames(events)
    got = _lines(program, dialect, stream, "keep", tmp_path)
    assert [line.split()[0] for line in got] == ["host", "host", "host", "status", "progress"]
    _against_the_definition(stream, got, dialect, "keep")
