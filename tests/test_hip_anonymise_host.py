"""The gfx950 anonymise kernels' per-frame code (ops/hip/telemetry_anonymise.hpp: the keyed hash, the
plan, the output length and every output byte) on a CPU, under ASan and UBSan.

tests/native/anonymise_host.cpp compiles the header for the host. Its ``hash`` mode is held to
``hashlib.blake2s`` for every string length from 1 to 200 and for 4,096, under keys of 16, 17, 31 and
32 bytes and both ``person`` values, each string in a heap block of exactly its size. Its ``stream``
mode plans every frame from a heap block of exactly the frame's size and puts the output frame
together from ``anon_byte`` one byte at a time; the frames are held to ``anonymise.anon_of`` on both
corpora, in both dialects, under both policies and the three ``fields`` choices; the frames it leaves
to the host are exactly the rule's (the normalise's, plus a chosen string above 4,096 bytes); and no
frame grows by more than ``AN_GROWTH_MAX`` (the program checks that itself). Nothing is loaded into
Python under a sanitizer."""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess

import pytest

from beholder_amd import anonymise as an, ops
from beholder_amd.coalesce import DROP, KEEP
from beholder_amd.models import proto
from beholder_amd.normalise import frame_of
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus, varint  # noqa: E402
from test_hip_normalise_host import RULES, TYPES  # noqa: E402  the normalise's host rule, written out there

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
KEY = bytes(range(1, 33))
KEYS = [bytes(range(7, 7 + n)) for n in (16, 17, 31, 32)]
FIELDS = {1: frozenset({"mediaId"}), 2: frozenset({"host"}), 3: frozenset({"mediaId", "host"})}
STRING_MAX = 4096
HOST_SHARE_MAX = 0.10  # of the fold corpus, in either dialect: the normalise's


def growth_max() -> int:
    with open(os.path.join(HIP, "telemetry_anonymise.hpp"), encoding="utf-8") as f:
        return int(re.search(r"constexpr int AN_GROWTH_MAX = (\d+);", f.read()).group(1))


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_normalise_host.py."""
    out = str(tmp_path_factory.mktemp("anonymise_host") / "anonymise_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "anonymise_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _run(program: str, *args) -> list:
    """The program's lines; any sanitizer report fails."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _lines(program: str, dialect: str, stream: bytes, undecoded: str, fields: int, tmp_path, key: bytes = KEY) -> list:
    path = tmp_path / "stream"
    path.write_bytes(stream)
    return _run(program, "stream", dialect, str(path), undecoded, str(fields), key.hex())


def test_the_hash_is_blake2s(program, tmp_path):
    """Every length 1 to 200 and 4,096: the block edges at 64, 128 and 192 are full final blocks."""
    cases = [(key, field, bytes((7 * i + n) & 0xff for i in range(n))) for key in KEYS for field in an.PERSON
             for n in list(range(1, 201)) + [4096]]
    path = tmp_path / "lines"
    path.write_text("".join(f"{key.hex()} {field} {text.hex()}\n" for key, field, text in cases))
    got = _run(program, "hash", str(path))
    want = [hashlib.blake2s(text, key=key, digest_size=16, person=an.PERSON[field]).hexdigest()
            for key, field, text in cases]
    assert len(got) == len(want) == 4 * 2 * 201
    assert got == want


def test_the_hash_is_pseudonym_of(program, tmp_path):
    path = tmp_path / "lines"
    key = bytes(range(32))
    path.write_text(f"{key.hex()} mediaId {b'abc'.hex()}\n{key.hex()} host {b'abc'.hex()}\n")
    assert _run(program, "hash", str(path)) == ["b43e852137b0f85cd672ee1eeece559a", "1b6723a26a3859aff3dd67995e6eac73"]
    assert an.pseudonym_of(key, "mediaId", "abc") == "b43e852137b0f85cd672ee1eeece559a"


def test_a_bad_key_is_refused(program, tmp_path):
    path = tmp_path / "lines"
    for n in (0, 15, 33):
        path.write_text(f"{bytes(n).hex() or '-'} host 61\n")
        r = subprocess.run([program, "hash", str(path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "bad line" in r.stderr


def _long_rule(topic: int, body: bytes, dialect: str, chosen: frozenset) -> bool:
    """The anonymise's own addition: a decoded event with a chosen string above 4,096 bytes."""
    if topic not in TYPES:
        return False
    try:
        m = ops.codec_for(TYPES[topic], dialect).decode(body)
    except proto.DecodeError:
        return False
    return ("mediaId" in chosen and len(m.mediaId.encode()) > STRING_MAX) or \
        (topic == PROGRESS_ID and "host" in chosen and len(m.host.encode()) > STRING_MAX)


def _against_the_definition(stream: bytes, got: list, dialect: str, undecoded: str, fields: int,
                            key: bytes = KEY) -> dict:
    """Asserts every line; returns the frames per kind of line."""
    anon = an.anon_of(an.Policy(key, undecoded, FIELDS[fields]), dialect)
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
        c = anon(topic, body)
        if c is DROP:
            want = ["drop"]
        elif c is KEEP:
            want = ["copy", frame_of(topic, body).hex(), "0"]
        else:
            want = [{STATUS_ID: "status", PROGRESS_ID: "progress"}[topic], frame_of(topic, c).hex(),
                    str(len(c) - len(body))]
            assert len(c) - len(body) <= cap
        if word != want:
            bad.append((i, topic, body, line, want))
    assert not bad, (len(bad), bad[:5])
    rule = RULES[dialect]
    assert kinds["host"] == {i for i, (topic, body) in enumerate(events)
                             if rule(topic, body) or _long_rule(topic, body, dialect, FIELDS[fields])}
    return kinds


@pytest.mark.parametrize("fields", sorted(FIELDS))
@pytest.mark.parametrize("undecoded", ["keep", "drop"])
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_frame_of_the_fold_corpus(program, tmp_path, dialect, undecoded, fields):
    stream = fold_corpus()
    got = _lines(program, dialect, stream, undecoded, fields, tmp_path)
    kinds = _against_the_definition(stream, got, dialect, undecoded, fields)
    frames_ = sum(map(len, kinds.values()))
    assert frames_ > 5000 and kinds["status"] and kinds["progress"] and kinds["copy" if undecoded == "keep" else "drop"]
    assert not kinds["drop" if undecoded == "keep" else "copy"]
    assert 0 < len(kinds["host"]) <= HOST_SHARE_MAX * frames_


@pytest.mark.parametrize("fields", sorted(FIELDS))
@pytest.mark.parametrize("undecoded", ["keep", "drop"])
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_frame_of_the_wire_edges(program, tmp_path, dialect, undecoded, fields):
    stream = wire_edges.stream(6000)
    got = _lines(program, dialect, stream, undecoded, fields, tmp_path)
    kinds = _against_the_definition(stream, got, dialect, undecoded, fields)
    assert len(kinds["status"]) + len(kinds["progress"]) > 300


def _int(field: int, value: int) -> bytes:
    return varint(field << 3) + varint(value & 0xFFFFFFFFFFFFFFFF)


def _str(field: int, value: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(value)) + value


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_frame_that_grows_most_and_the_block_edges(program, tmp_path, dialect):
    """`0a 01 6d | 10 ff ff ff ff 0f | 18 ff ff ff ff 0f | 22 01 68` reaches AN_GROWTH_MAX; string
    lengths at the hash's block edges and at the host limit, under every key length."""
    minus = b"\xff\xff\xff\xff\x0f"
    most = b"\x0a\x01m\x10" + minus + b"\x18" + minus + b"\x22\x01h"
    lengths = (0, 1, 55, 56, 63, 64, 65, 127, 128, 129, 4095, 4096)
    bodies = [most, b"\x0a\x01m\x10" + minus]
    bodies += [_str(1, b"i" * n) + _str(4, b"h" * k) + _int(2, 3) for n in lengths for k in (0, 1, 64, 4096)]
    stream = frames([(topic, body) for body in bodies for topic in (STATUS_ID, PROGRESS_ID)])
    for key in KEYS:
        got = _lines(program, dialect, stream, "drop", 3, tmp_path, key)
        kinds = _against_the_definition(stream, got, dialect, "drop", 3, key)
        assert not kinds["host"] and not kinds["drop"]
        assert got[1].split()[2] == str(growth_max()) == "72"  # the progress event
        assert got[2].split()[2] == "36"  # a status event's most: one string, one int32
        assert max(int(line.split()[2]) for line in got) == growth_max()


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_a_chosen_string_above_the_limit_goes_to_the_host(program, tmp_path, dialect):
    long = b"x" * (STRING_MAX + 1)
    events = [(PROGRESS_ID, _str(1, long)), (PROGRESS_ID, _str(1, b"m") + _str(4, long)), (STATUS_ID, _str(1, long)),
              (STATUS_ID, _str(1, b"m") + _str(4, long)),  # field 4 of a status message is an unknown field
              (PROGRESS_ID, _str(1, long) + _str(1, b"m"))]  # the last id wins, and it is short
    stream = frames(events)
    for fields, want in ((3, ["host", "host", "host", "status", "progress"]),
                         (1, ["host", "progress", "host", "status", "progress"]),
                         (2, ["progress", "host", "status", "status", "progress"])):
        got = _lines(program, dialect, stream, "keep", fields, tmp_path)
        assert [line.split()[0] for line in got] == want
        _against_the_definition(stream, got, dialect, "keep", fields)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_normalise_rule_still_holds(program, tmp_path, dialect):
    """A string that is not ASCII goes to the host whether it is chosen or not; a group under upb."""
    group = _str(1, b"m") + b"\x2b\x08\x01\x2c" + _int(2, 3)
    events = [(PROGRESS_ID, _str(1, "é".encode())), (PROGRESS_ID, _str(1, b"m") + _str(4, b"\xff")),
              (STATUS_ID, _str(1, b"\x80")), (STATUS_ID, group)]
    stream = frames(events)
    for fields in FIELDS:
        got = _lines(program, dialect, stream, "keep", fields, tmp_path)
        assert [line.split()[0] for line in got] == ["host", "host", "host", "host" if dialect == "upb" else "status"]
        _against_the_definition(stream, got, dialect, "keep", fields)
