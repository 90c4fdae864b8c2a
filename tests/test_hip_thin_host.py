"""The gfx950 thin kernels' per-frame code (ops/hip/telemetry_thin.hpp: the classification, the floor
division and the mark word) on a CPU, under ASan and UBSan.

tests/native/thin_host.cpp compiles the header for the host and decides every frame of a stream from
a heap block of exactly the frame's size: a read past it is a sanitizer report here. Its lines are
held to ``thin.mark_of`` and the service's codec in both dialects: not read / error / event with id,
status, bucket and hash / host. Nothing is loaded into Python under a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from beholder_amd import ops, thin as th
from beholder_amd.models import proto
from beholder_amd.topics import PROGRESS_ID
from beholder_amd.transport.framing import iter_frames

np = pytest.importorskip("numpy")  # gpu_fold imports it
from beholder_amd.ops import gpu_fold  # noqa: E402
import wire_edges  # noqa: E402
from thin_cases import (STEPS, corpus, edge_stream, mixed_stream, non_ascii_stream, random_stream,  # noqa: E402
                        stitch_stream)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
PROGRESS = proto.load("api.TelemetryProgress")


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_shard_host.py."""
    out = str(tmp_path_factory.mktemp("thin_host") / "thin_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "thin_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _lines(program: str, dialect: str, stream: bytes, step: int, tmp_path) -> list:
    """The program's line per frame of ``stream``; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, dialect, str(path), str(step)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _against_the_definition(stream: bytes, got: list, dialect: str, step: int) -> dict:
    """Asserts every line; returns the frames per kind of line."""
    mark = th.mark_of(th.Policy(step), dialect)
    events = list(iter_frames(stream))
    assert len(got) == len(events)
    kinds = {"skip": set(), "error": set(), "host": set(), "event": set()}
    bad = []
    for i, ((topic, body), line) in enumerate(zip(events, got)):
        word = line.split()
        kinds[word[0]].add(i)
        if topic != PROGRESS_ID:
            want = ["skip"]
        else:
            m = mark(topic, body)
            if word[0] == "host":  # the device does not decide: never an error of the codec under protobufjs
                if dialect == "protobufjs":
                    assert m is not None and not m[0].isascii(), (i, body)
                continue
            if m is None:
                want = ["error"]
            else:
                mid = m[0].encode("ascii")  # a frame the device decides has an ASCII id
                want = ["event", mid.hex() or "-", str(m[1]), str(m[2]), str(gpu_fold.hash64(mid))]
        if word != want:
            bad.append((i, topic, body, line, want))
    assert not bad, (len(bad), bad[:5])
    return kinds


def _rule(stream: bytes) -> set:
    """The frames of a protobufjs stream that the rule hands to the host: topic 2, decodes, and the
    id is not ASCII."""
    decode = ops.codec_for(PROGRESS, "protobufjs").decode

    def high(body):
        try:
            return not decode(body).mediaId.isascii()
        except proto.DecodeError:
            return False
    return {i for i, (topic, body) in enumerate(iter_frames(stream)) if topic == PROGRESS_ID and high(body)}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_lines_agree_with_the_definition_on_the_fold_corpus(program, tmp_path, dialect):
    stream = corpus()
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, 10, tmp_path), dialect, 10)
    assert all(kinds.values())
    frames = sum(map(len, kinds.values()))
    assert frames > 5000 and len(kinds["host"]) <= 0.05 * frames  # the comparison covers what the device decides itself
    assert kinds["skip"] == {i for i, (topic, _) in enumerate(iter_frames(stream)) if topic != PROGRESS_ID}
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_lines_agree_with_the_definition_on_the_wire_edges(program, tmp_path, dialect):
    stream = wire_edges.stream()
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, 10, tmp_path), dialect, 10)
    compared = sum(map(len, kinds.values())) - len(kinds["skip"])
    print(f"{dialect}: {compared} progress frames, {len(kinds['host'])} left to the host")
    assert compared == len(wire_edges.bodies()) and len(kinds["event"]) > 2000 and len(kinds["error"]) > 2000
    assert len(kinds["host"]) <= wire_edges.HOST_CAP[dialect] * compared
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_small_mixed_stream(program, tmp_path, dialect):
    stream = mixed_stream()
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, 10, tmp_path), dialect, 10)
    assert all(kinds.values())
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("step", STEPS)
def test_the_step_and_percentage_edges(program, tmp_path, dialect, step):
    """INT_MIN, INT_MAX and the negatives through every step: the division is Python's, and UBSan sees
    no overflow in it."""
    stream = edge_stream() + random_stream(1) + random_stream(2)
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, step, tmp_path), dialect, step)
    assert len(kinds["event"]) > 200 and kinds["error"]
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


def test_a_group_or_a_non_ascii_host_goes_to_the_host_under_upb_only(program, tmp_path):
    stream = stitch_stream()
    upb = _against_the_definition(stream, _lines(program, "upb", stream, 10, tmp_path), "upb", 10)
    assert len(upb["host"]) == 9 + 9 + 6 and len(upb["event"]) == 9 + 9 + 9
    pbjs = _against_the_definition(stream, _lines(program, "protobufjs", stream, 10, tmp_path), "protobufjs", 10)
    assert not pbjs["host"] and len(pbjs["event"]) == 51
    stream = random_stream(3)  # a quarter of its hosts are not ASCII
    upb = _against_the_definition(stream, _lines(program, "upb", stream, 10, tmp_path), "upb", 10)
    pbjs = _against_the_definition(stream, _lines(program, "protobufjs", stream, 10, tmp_path), "protobufjs", 10)
    assert len(upb["host"]) > len(pbjs["host"]) > 0


def test_ids_that_are_not_ascii_go_to_the_host(program, tmp_path):
    stream = non_ascii_stream()
    for dialect in ops.DIALECTS:
        kinds = _against_the_definition(stream, _lines(program, dialect, stream, 10, tmp_path), dialect, 10)
        assert len(kinds["host"]) > 150 and len(kinds["event"]) > 40 and not kinds["error"]
