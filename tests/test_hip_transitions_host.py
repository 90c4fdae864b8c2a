"""The gfx950 transitions kernels' per-frame code (ops/hip/telemetry_transitions.hpp: classify and the
class mapping) on a CPU, under ASan and UBSan.

tests/native/transitions_host.cpp compiles the header for the host and decides every frame of a
stream from a heap block of exactly the frame's size: a read past it is a sanitizer report here. Its
lines are held to the service's codecs in both dialects: not read / error / event with id, status,
class and hash / host. Nothing is loaded into Python under a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from beholder_amd import ops, replay
from beholder_amd.models import proto
from beholder_amd.topics import STATUS_ID
from beholder_amd.transitions import UNKNOWN, class_of
from beholder_amd.transport.framing import iter_frames

np = pytest.importorskip("numpy")  # gpu_fold imports it
from beholder_amd.ops import gpu_fold  # noqa: E402
import wire_edges  # noqa: E402
from transitions_cases import UNKNOWN_NUMBERS, corpus, mixed_stream, shared_media_stream, status_stream  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
STATUS = proto.load("api.TelemetryStatus")


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_shard_host.py."""
    out = str(tmp_path_factory.mktemp("transitions_host") / "transitions_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "transitions_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _lines(program: str, dialect: str, stream: bytes, tmp_path) -> list:
    """The program's line per frame of ``stream``; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    mask = gpu_fold.known_mask(replay.status_names())
    r = subprocess.run([program, dialect, str(path), str(mask)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _against_the_codec(stream: bytes, got: list, dialect: str) -> dict:
    """Asserts every line; returns the frames per kind of line."""
    decode = ops.codec_for(STATUS, dialect).decode
    names = replay.status_names()
    events = list(iter_frames(stream))
    assert len(got) == len(events)
    kinds = {"skip": set(), "error": set(), "host": set(), "event": set()}
    bad = []
    for i, ((topic, body), line) in enumerate(zip(events, got)):
        word = line.split()
        kinds[word[0]].add(i)
        if topic != STATUS_ID:
            want = ["skip"]
        else:
            try:
                m = decode(body)
            except proto.DecodeError:
                m = None
            if word[0] == "host":  # the device does not decide: never an error of the codec under protobufjs
                if dialect == "protobufjs":
                    assert m is not None and not m.mediaId.isascii(), (i, body)
                continue
            if m is None:
                want = ["error"]
            else:
                mid = m.mediaId.encode("ascii")  # a frame the device decides has an ASCII id
                cls = class_of(m.status, names)
                want = ["event", mid.hex() or "-", str(m.status), str(64 if cls == UNKNOWN else cls),
                        str(gpu_fold.hash64(mid))]
        if word != want:
            bad.append((i, topic, body, line, want))
    assert not bad, (len(bad), bad[:5])
    return kinds


def _rule(stream: bytes) -> set:
    """The frames of a protobufjs stream that the rule hands to the host: topic 1, decodes, and the
    id is not ASCII."""
    decode = ops.codec_for(STATUS, "protobufjs").decode

    def high(body):
        try:
            return not decode(body).mediaId.isascii()
        except proto.DecodeError:
            return False
    return {i for i, (topic, body) in enumerate(iter_frames(stream)) if topic == STATUS_ID and high(body)}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_lines_agree_with_the_codec_on_the_fold_corpus(program, tmp_path, dialect):
    stream = corpus()
    kinds = _against_the_codec(stream, _lines(program, dialect, stream, tmp_path), dialect)
    assert all(kinds.values())
    frames = sum(map(len, kinds.values()))
    assert frames > 5000 and len(kinds["host"]) <= 0.05 * frames  # the comparison covers what the device decides itself
    assert kinds["skip"] == {i for i, (topic, _) in enumerate(iter_frames(stream)) if topic != STATUS_ID}
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_lines_agree_with_the_codec_on_the_wire_edges(program, tmp_path, dialect):
    stream = wire_edges.stream()
    kinds = _against_the_codec(stream, _lines(program, dialect, stream, tmp_path), dialect)
    compared = sum(map(len, kinds.values())) - len(kinds["skip"])
    print(f"{dialect}: {compared} status frames, {len(kinds['host'])} left to the host")
    assert compared == len(wire_edges.bodies()) and len(kinds["event"]) > 2000 and len(kinds["error"]) > 2000
    assert len(kinds["host"]) <= wire_edges.HOST_CAP[dialect] * compared
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_small_mixed_stream(program, tmp_path, dialect):
    stream = mixed_stream()
    kinds = _against_the_codec(stream, _lines(program, dialect, stream, tmp_path), dialect)
    assert all(kinds.values())
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


def test_the_unknown_numbers_are_one_class(program, tmp_path):
    stream = status_stream([b"m"] * 12, statuses=1)
    from beholder_amd.ops import frames
    from telemetry_corpus import body
    stream += frames([(STATUS_ID, body(b"m", s)) for s in UNKNOWN_NUMBERS])
    for dialect in ops.DIALECTS:
        got = _lines(program, dialect, stream, tmp_path)
        _against_the_codec(stream, got, dialect)
        assert [line.split()[3] for line in got[12:]] == ["64"] * len(UNKNOWN_NUMBERS)
        assert {line.split()[3] for line in got[:12]} == {"0"}


def test_a_group_goes_to_the_host_under_upb_only(program, tmp_path):
    stream = shared_media_stream()
    upb = _against_the_codec(stream, _lines(program, "upb", stream, tmp_path), "upb")
    assert len(upb["host"]) == 12 and len(upb["event"]) == 21
    pbjs = _against_the_codec(stream, _lines(program, "protobufjs", stream, tmp_path), "protobufjs")
    assert not pbjs["host"] and len(pbjs["event"]) == 33
