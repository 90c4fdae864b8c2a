"""The gfx950 export kernels' per-frame code (ops/hip/telemetry_export.hpp: the plan, the row's
length, every byte of the row, the escapes in pieces of 64) on a CPU, under ASan and UBSan.

tests/native/export_host.cpp compiles the header for the host, plans every frame of a stream from a
heap block of exactly the frame's size and builds every row twice into heap blocks of exactly the
row's length: one byte after the other, and piecewise as the emit kernel does. The program itself
fails where the two differ or miss ``row_len``; here its rows are held to ``export.row_of`` on both
corpora, in both dialects and under both policies, and the frames it leaves to the host must be
exactly the rule's (tests/test_hip_normalise_host.py has it). Nothing is loaded into Python under a
sanitizer."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

from beholder_amd import export as ex, ops
from beholder_amd.coalesce import DROP
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus, varint  # noqa: E402
from test_hip_normalise_host import RULES  # noqa: E402  which frames go to the host

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
HOST_SHARE_MAX = 0.10  # of the fold corpus, in either dialect
POLICIES = ("keep", "drop")
KIND_OF = {STATUS_ID: "status", PROGRESS_ID: "progress"}


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_normalise_host.py."""
    out = str(tmp_path_factory.mktemp("export_host") / "export_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "export_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _lines(program: str, dialect: str, stream: bytes, undecoded: str, tmp_path, base: int = 0) -> list:
    """The program's line per frame of ``stream``; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, dialect, str(path), undecoded, str(base)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _against_the_definition(stream: bytes, got: list, dialect: str, undecoded: str, base: int = 0) -> dict:
    """Asserts every line; returns the frames per kind of line."""
    row = ex.row_of(ex.Policy(undecoded), dialect)
    events = list(iter_frames(stream))
    assert len(got) == len(events)
    kinds = {"b64": set(), "drop": set(), "host": set(), "status": set(), "progress": set()}
    bad = []
    for i, ((topic, body), line) in enumerate(zip(events, got)):
        word = line.split()
        kinds[word[0]].add(i)
        if word[0] == "host":
            continue
        r = row(base + i, topic, body)
        if r is DROP:
            want = ["drop"]
        else:
            want = ["b64" if b'"b64":' in r else KIND_OF[topic], r.hex()]
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
    assert frames_ > 5000 and kinds["status"] and kinds["progress"] and kinds["b64" if undecoded == "keep" else "drop"]
    assert not kinds["drop" if undecoded == "keep" else "b64"]
    print(f"{dialect}: {len(kinds['host'])} of {frames_} frames left to the host")
    assert len(kinds["host"]) <= HOST_SHARE_MAX * frames_
    if dialect == "protobufjs":
        assert len(kinds["host"]) > 0


@pytest.mark.parametrize("undecoded", POLICIES)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_frame_of_the_wire_edges(program, tmp_path, dialect, undecoded):
    stream = wire_edges.stream(6000)
    base = 2 ** 53 - 100  # the index steps to 16 digits on the way
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, undecoded, tmp_path, base), dialect,
                                    undecoded, base)
    assert len(kinds["status"]) + len(kinds["progress"]) > 300
    print(f"{dialect}: {len(kinds['host'])} of {sum(map(len, kinds.values()))} frames left to the host")


def _int(field: int, value: int) -> bytes:
    return varint(field << 3) + varint(value & 0xFFFFFFFFFFFFFFFF)


def _str(field: int, value: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(value)) + value


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_ascii_byte_as_an_id_and_as_a_host(program, tmp_path, dialect):
    """The escapes one by one, and json.loads gives the byte back."""
    events = [(PROGRESS_ID, _str(1, bytes([c]))) for c in range(0x80)]
    events += [(PROGRESS_ID, _str(1, b"m") + _str(4, bytes([c]))) for c in range(0x80)]
    events += [(STATUS_ID, _str(1, bytes([c]) * 3)) for c in range(0x80)]
    stream = frames(events)
    got = _lines(program, dialect, stream, "keep", tmp_path)
    kinds = _against_the_definition(stream, got, dialect, "keep")
    assert not kinds["host"] and not kinds["b64"]
    for c in range(0x80):
        assert json.loads(bytes.fromhex(got[c].split()[1]))["json"]["mediaId"] == chr(c)
        assert json.loads(bytes.fromhex(got[0x80 + c].split()[1]))["json"]["host"] == chr(c)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_escapes_across_the_pieces_of_64(program, tmp_path, dialect):
    """A two-byte and a six-byte escape at and around every piece boundary; all six-byte, all two-byte."""
    events = []
    for n in (1, 63, 64, 65, 127, 128, 129, 200):
        for fill in (b"\x01", b"\\", b"\n"):
            events.append((PROGRESS_ID, _str(1, fill * n) + _str(4, fill * n)))
        for at in sorted({0, 62, 63, 64, n - 1} & set(range(n))):
            for esc in (b'"', b"\x01", b"\x1f", b"\t"):
                s = b"a" * at + esc + b"b" * (n - at - 1)
                events += [(STATUS_ID, _str(1, s)), (PROGRESS_ID, _str(1, b"plain") + _str(4, s)),
                           (PROGRESS_ID, _str(1, s) + _str(4, s[::-1]))]
    stream = frames(events)
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, "keep", tmp_path), dialect, "keep")
    assert not kinds["host"] and not kinds["b64"]


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_numbers_names_indices_and_base64(program, tmp_path, dialect):
    values = (0, 5, 6, -1, -2 ** 31, 2 ** 31 - 1, 10, 99, 100, 9, -9, -10, 2 ** 31 - 2)
    events = [(PROGRESS_ID, _int(2, s) + _int(3, p)) for s in values for p in values]
    events += [(STATUS_ID, _int(2, s)) for s in values]
    events += [(t, b"\x2e" + bytes(range(n))) for t in (STATUS_ID, PROGRESS_ID, 0, 9, 10, 99, 100, 255)
               for n in (0, 1, 2, 3, 4, 5, 62, 63, 64, 65, 255)]  # 0x2e: field 5, wire type 6, in either dialect
    events += [(9, b""), (STATUS_ID, b""), (PROGRESS_ID, b"")]
    stream = frames(events)
    for base in (0, 9, 99, 10 ** 9 - 1, 2 ** 31, 2 ** 32 - 5, 2 ** 53, 2 ** 62 - len(events)):
        kinds = _against_the_definition(stream, _lines(program, dialect, stream, "keep", tmp_path, base), dialect,
                                        "keep", base)
        assert not kinds["host"] and len(kinds["b64"]) == 8 * 11 + 1
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, "drop", tmp_path), dialect, "drop")
    assert len(kinds["drop"]) == 8 * 11 + 1 and not kinds["b64"]


def test_a_group_goes_to_the_host_under_upb_only(program, tmp_path):
    body = _str(1, b"m") + b"\x2b\x08\x01\x2c" + _int(2, 3)
    stream = frames([(STATUS_ID, body), (PROGRESS_ID, body)])
    assert _lines(program, "upb", stream, "keep", tmp_path) == ["host", "host"]
    _against_the_definition(stream, _lines(program, "upb", stream, "keep", tmp_path), "upb", "keep")
    kinds = _against_the_definition(stream, _lines(program, "protobufjs", stream, "keep", tmp_path), "protobufjs", "keep")
    assert kinds["status"] == {0} and kinds["progress"] == {1}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_a_string_that_is_not_ascii_goes_to_the_host(program, tmp_path, dialect):
    events = [(PROGRESS_ID, _str(1, "é".encode())), (PROGRESS_ID, _str(1, b"m") + _str(4, b"\xff")),
              (STATUS_ID, _str(1, b"\x80")), (STATUS_ID, _str(1, b"m") + _str(4, b"\xff")),
              (PROGRESS_ID, _str(1, b"\xc3\xa9") + _str(1, b"m\x7f"))]  # the last id wins, and it is ASCII
    stream = frames(events)
    got = _lines(program, dialect, stream, "keep", tmp_path)
    assert [line.split()[0] for line in got] == ["host", "host", "host", "status", "progress"]
    _against_the_definition(stream, got, dialect, "keep")
