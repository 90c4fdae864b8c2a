"""The gfx950 stages kernels' per-frame code (ops/hip/telemetry_stages.hpp: the classification of both
topics, the row, the aux word, and the bucket function) on a CPU, under ASan and UBSan.

tests/native/stages_host.cpp compiles the header for the host and decides every frame of a stream from
a heap block of exactly the frame's size: a read past it is a sanitizer report here. Its lines are
held to the service's codecs in both dialects: not read / error / host / status or progress event
with id, status, progress and hash. Nothing is loaded into Python under a sanitizer."""
from __future__ import annotations

import os
import random
import shutil
import subprocess

import pytest

from beholder_amd import ops
from beholder_amd.models import proto
from beholder_amd.ops import frames
from beholder_amd.stages import BUCKETS, bucket_of
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

np = pytest.importorskip("numpy")  # gpu_fold imports it
from beholder_amd.ops import gpu_fold  # noqa: E402
import wire_edges  # noqa: E402
from stages_cases import bucket_edges, corpus, non_ascii_stream, random_stream, stitch_stream  # noqa: E402
from telemetry_corpus import MALFORMED_FOLD, malformed  # noqa: E402
from thin_cases import PERCENTAGES, mixed_stream  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
TYPES = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_hosts_host.py."""
    out = str(tmp_path_factory.mktemp("stages_host") / "stages_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "stages_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _run(program: str, args: list, stdin: str = None) -> list:
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, *args], input=stdin, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _lines(program: str, dialect: str, stream: bytes, tmp_path) -> list:
    """The program's line per frame of ``stream``; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    return _run(program, [dialect, str(path)])


def _against_the_definition(stream: bytes, got: list, dialect: str) -> dict:
    """Asserts every line; returns the frames per kind of line."""
    decode = {topic: ops.codec_for(t, dialect).decode for topic, t in TYPES.items()}
    events = list(iter_frames(stream))
    assert len(got) == len(events)
    kinds = {"skip": set(), "error": set(), "host": set(), "status": set(), "progress": set()}
    bad = []
    for i, ((topic, body), line) in enumerate(zip(events, got)):
        word = line.split()
        kinds[word[0]].add(i)
        if topic not in decode:
            want = ["skip"]
        else:
            try:
                m = decode[topic](body)
            except proto.DecodeError:
                m = None
            if word[0] == "host":  # the device does not decide: never an error of the codec under protobufjs
                if dialect == "protobufjs":
                    assert m is not None and not m.mediaId.isascii(), (i, body)
                continue
            if m is None:
                want = ["error"]
            else:  # a frame the device decides has an ASCII id
                mid = m.mediaId.encode("ascii")
                want = ["status", mid.hex() or "-", str(m.status)] if topic == STATUS_ID else \
                    ["progress", mid.hex() or "-", str(m.status), str(m.progress)]
                want.append(str(gpu_fold.hash64(mid)))
        if word != want:
            bad.append((i, topic, body, line, want))
    assert not bad, (len(bad), bad[:5])
    return kinds


def _rule(stream: bytes) -> set:
    """The frames of a protobufjs stream that the rule hands to the CPU: topic 1 or 2, decodes, and
    the id is not ASCII."""
    decode = {topic: ops.codec_for(t, "protobufjs").decode for topic, t in TYPES.items()}

    def high(topic, body):
        try:
            return not decode[topic](body).mediaId.isascii()
        except proto.DecodeError:
            return False
    return {i for i, (topic, body) in enumerate(iter_frames(stream)) if topic in decode and high(topic, body)}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_lines_agree_with_the_definition_on_the_fold_corpus(program, tmp_path, dialect):
    stream = corpus()
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
    assert all(kinds.values())
    total = sum(map(len, kinds.values()))
    assert total == 5711 and len(kinds["host"]) <= 0.05 * total  # the comparison covers what the device decides
    assert kinds["skip"] == {i for i, (topic, _) in enumerate(iter_frames(stream)) if topic not in TYPES}
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_lines_agree_with_the_definition_on_the_wire_edges(program, tmp_path, dialect):
    stream = wire_edges.stream()
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
    compared = sum(map(len, kinds.values()))
    print(f"{dialect}: {compared} frames, {len(kinds['host'])} left to the host")
    assert compared == 2 * len(wire_edges.bodies()) and not kinds["skip"] and len(kinds["error"]) > 4000
    assert len(kinds["status"]) > 2000 and len(kinds["progress"]) > 2000
    assert len(kinds["host"]) <= wire_edges.HOST_CAP[dialect] * compared
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_malformed_bodies_on_both_topics(program, tmp_path, dialect):
    bodies = malformed(random.Random(3), MALFORMED_FOLD) + [b""]
    stream = frames([(topic, b) for b in bodies for topic in (STATUS_ID, PROGRESS_ID, 7)])
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
    assert kinds["error"] and kinds["status"] and kinds["progress"] and len(kinds["skip"]) == len(bodies)
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_small_streams(program, tmp_path, dialect):
    for stream in (mixed_stream(), bucket_edges(), random_stream(1) + random_stream(2) + random_stream(3)):
        kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
        assert kinds["status"] and kinds["progress"]
        if dialect == "protobufjs":
            assert kinds["host"] == _rule(stream)


def test_a_group_goes_to_the_cpu_under_upb_only(program, tmp_path):
    stream = stitch_stream()
    upb = _against_the_definition(stream, _lines(program, "upb", stream, tmp_path), "upb")
    assert len(upb["host"]) == 12 + 8 + 8 and upb["status"] and upb["progress"]
    pbjs = _against_the_definition(stream, _lines(program, "protobufjs", stream, tmp_path), "protobufjs")
    assert not pbjs["host"] and len(pbjs["status"]) + len(pbjs["progress"]) == 24 + 24 + 9 + 8


def test_a_non_ascii_id_goes_to_the_cpu_in_both_dialects(program, tmp_path):
    stream = non_ascii_stream()
    for dialect in ops.DIALECTS:
        kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
        assert len(kinds["host"]) > 150 and len(kinds["status"]) > 10 and len(kinds["progress"]) > 30
        assert not kinds["error"]


def test_the_bucket_function(program):
    lasts = sorted(set(PERCENTAGES) | set(range(-12, 112)) | {-2 ** 31 + 1, 2 ** 31 - 2, 1000, -1000})
    cases = [(count, last) for count in (0, 1, 2, 2 ** 32 - 1) for last in lasts]
    got = _run(program, ["buckets"], "".join(f"{count} {last}\n" for count, last in cases))
    assert [BUCKETS[int(line)] for line in got] == [bucket_of(count, last) for count, last in cases]
    assert {BUCKETS[int(line)] for line in got} == set(BUCKETS)
