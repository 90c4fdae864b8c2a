"""The gfx950 hosts kernels' per-frame code (ops/hip/telemetry_hosts.hpp: the classification, the two
rows and the progress) on a CPU, under ASan and UBSan.

tests/native/hosts_host.cpp compiles the header for the host and decides every frame of a stream from
a heap block of exactly the frame's size: a read past it is a sanitizer report here. Its lines are
held to the service's codec in both dialects: not read / error / host / event with id, worker,
status, progress and both hashes. Nothing is loaded into Python under a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from beholder_amd import ops
from beholder_amd.models import proto
from beholder_amd.topics import PROGRESS_ID
from beholder_amd.transport.framing import iter_frames

np = pytest.importorskip("numpy")  # gpu_fold imports it
from beholder_amd.ops import gpu_fold  # noqa: E402
import wire_edges  # noqa: E402
from hosts_cases import (corpus, many_workers, non_ascii_stream, random_stream, shared_by_worker_stream,  # noqa: E402
                         stitch_stream)
from thin_cases import edge_stream, mixed_stream  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
PROGRESS = proto.load("api.TelemetryProgress")


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_thin_host.py."""
    out = str(tmp_path_factory.mktemp("hosts_host") / "hosts_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "hosts_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _lines(program: str, dialect: str, stream: bytes, tmp_path) -> list:
    """The program's line per frame of ``stream``; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, dialect, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _against_the_definition(stream: bytes, got: list, dialect: str) -> dict:
    """Asserts every line; returns the frames per kind of line."""
    decode = ops.codec_for(PROGRESS, dialect).decode
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
            try:
                m = decode(body)
            except proto.DecodeError:
                m = None
            if word[0] == "host":  # the device does not decide: never an error of the codec under protobufjs
                if dialect == "protobufjs":
                    assert m is not None and not (m.mediaId.isascii() and m.host.isascii()), (i, body)
                continue
            if m is None:
                want = ["error"]
            else:  # a frame the device decides has an ASCII id and an ASCII worker
                mid, worker = m.mediaId.encode("ascii"), m.host.encode("ascii")
                want = ["event", mid.hex() or "-", worker.hex() or "-", str(m.status), str(m.progress),
                        str(gpu_fold.hash64(mid)), str(gpu_fold.hash64(worker))]
        if word != want:
            bad.append((i, topic, body, line, want))
    assert not bad, (len(bad), bad[:5])
    return kinds


def _rule(stream: bytes) -> set:
    """The frames of a protobufjs stream that the rule hands to the CPU: topic 2, decodes, and the id
    or the host is not ASCII."""
    decode = ops.codec_for(PROGRESS, "protobufjs").decode

    def high(body):
        try:
            m = decode(body)
        except proto.DecodeError:
            return False
        return not (m.mediaId.isascii() and m.host.isascii())
    return {i for i, (topic, body) in enumerate(iter_frames(stream)) if topic == PROGRESS_ID and high(body)}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_lines_agree_with_the_definition_on_the_fold_corpus(program, tmp_path, dialect):
    stream = corpus()
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
    assert all(kinds.values())
    frames = sum(map(len, kinds.values()))
    assert frames == 5711 and len(kinds["host"]) <= 0.05 * frames  # the comparison covers what the device decides
    assert kinds["skip"] == {i for i, (topic, _) in enumerate(iter_frames(stream)) if topic != PROGRESS_ID}
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream) and len(kinds["host"]) == 127


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_lines_agree_with_the_definition_on_the_wire_edges(program, tmp_path, dialect):
    stream = wire_edges.stream()
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
    compared = sum(map(len, kinds.values())) - len(kinds["skip"])
    print(f"{dialect}: {compared} progress frames, {len(kinds['host'])} left to the host")
    assert compared == len(wire_edges.bodies()) and len(kinds["event"]) > 2000 and len(kinds["error"]) > 2000
    assert len(kinds["host"]) <= wire_edges.HOST_CAP[dialect] * compared
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_small_mixed_stream_and_the_percentage_edges(program, tmp_path, dialect):
    for stream in (mixed_stream(), edge_stream()):
        kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
        assert kinds["event"]
        if dialect == "protobufjs":
            assert kinds["host"] == _rule(stream)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_seeded_streams(program, tmp_path, dialect):
    stream = random_stream(1) + random_stream(2) + random_stream(3) + many_workers(70)
    kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
    assert len(kinds["event"]) > 250 and kinds["error"] and kinds["host"] and kinds["skip"]
    if dialect == "protobufjs":
        assert kinds["host"] == _rule(stream)


def test_a_group_goes_to_the_cpu_under_upb_only(program, tmp_path):
    stream = stitch_stream()
    upb = _against_the_definition(stream, _lines(program, "upb", stream, tmp_path), "upb")
    assert len(upb["host"]) == 9 + 9 + 6 and len(upb["event"]) == 9 + 9 + 9
    pbjs = _against_the_definition(stream, _lines(program, "protobufjs", stream, tmp_path), "protobufjs")
    assert not pbjs["host"] and len(pbjs["event"]) == 51


def test_a_non_ascii_worker_or_id_goes_to_the_cpu_in_both_dialects(program, tmp_path):
    stream = shared_by_worker_stream()
    for dialect in ops.DIALECTS:
        kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
        assert len(kinds["host"]) == 2 + 2 + 2 + 6 and len(kinds["event"]) == 30 - 12 and not kinds["error"]
        assert kinds["host"] == _rule(stream)
    stream = non_ascii_stream()
    for dialect in ops.DIALECTS:
        kinds = _against_the_definition(stream, _lines(program, dialect, stream, tmp_path), dialect)
        assert len(kinds["host"]) > 150 and len(kinds["event"]) > 40 and not kinds["error"]
