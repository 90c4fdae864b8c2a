"""The gfx950 coalesce kernels' per-frame decision and key hash (ops/hip/telemetry_coalesce.hpp) on a
CPU, under ASan and UBSan.

tests/native/coalesce_host.cpp compiles the header for the host and decides every frame of a stream
from a heap block of exactly the frame's size: a read past it is a sanitizer report here. Its lines
are held to ``coalesce.key_of``, the definition, for every policy in both dialects: keep and drop as
they are, a key by its topic, its status and the id bytes it points at; its host lines to the rule
that hands a frame to the host. The hash it prints is held to ``gpu_coalesce.key_hash``. Nothing is
loaded into Python under a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from beholder_amd import coalesce as co, ops
from beholder_amd.coalesce import DROP, KEEP, Policy
from beholder_amd.models import proto
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_coalesce as gc  # noqa: E402
import wire_edges  # noqa: E402
from coalesce_cases import POLICIES, mixed_stream, policy_id  # noqa: E402
from telemetry_corpus import fold_corpus  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
TYPES = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/native/Makefile's readers_host_asan rule."""
    out = str(tmp_path_factory.mktemp("coalesce_host") / "coalesce_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "coalesce_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _decisions(program: str, dialect: str, stream: bytes, policy: Policy, tmp_path) -> list:
    """The program's line per frame of ``stream``, split into words; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, dialect, str(path), str(gc.policy_flags(policy))], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return [line.split() for line in r.stdout.splitlines()]


def _against_the_definition(stream: bytes, got: list, policy: Policy, dialect: str) -> set:
    """Asserts the decisions; returns the frames that went to the host."""
    key = co.key_of(policy, dialect)
    events = list(iter_frames(stream))
    assert len(got) == len(events)
    codecs = {t: ops.codec_for(p, dialect) for t, p in TYPES.items()}
    per_status = policy.progress == "per-status"
    host, bad = set(), []
    for i, ((topic, body), words) in enumerate(zip(events, got)):
        want = key(topic, body)
        if words == ["host"]:
            host.add(i)
            assert topic in TYPES, (i, topic)
            if dialect == "protobufjs":  # the rule in full: it decodes, and its id is not ASCII
                assert not codecs[topic].decode(body).mediaId.isascii(), (i, body)
            continue
        if want is KEEP or want is DROP:
            ok = words == [want]
        else:
            ok = len(words) == 6 and words[0] == "key"
            if ok:
                got_topic, status, off, length = (int(w) for w in words[1:5])
                mid = body[off:off + length]
                status_want = want[2] if per_status and topic == PROGRESS_ID else 0
                ok = (got_topic == topic == want[0] and mid.isascii() and mid.decode("ascii") == want[1]
                      and status == status_want and int(words[5], 16) == gc.key_hash(mid, topic, status_want))
        if not ok:
            bad.append((i, topic, body, words, want))
    assert not bad, (len(bad), bad[:5])
    return host


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_decision_agrees_with_the_definition_on_the_fold_corpus(program, tmp_path, policy, dialect):
    stream = fold_corpus()
    got = _decisions(program, dialect, stream, policy, tmp_path)
    host = _against_the_definition(stream, got, policy, dialect)
    assert len(got) > 5000 and len(host) <= 0.05 * len(got)  # the comparison covers what the device decides itself
    kinds = {words[0] for words in got}
    if policy == Policy():
        assert host and kinds == {"keep", "key", "host"}
    if policy == Policy("all", "all", "keep"):
        assert kinds == {"keep"}  # nothing depends on what a frame holds: none is read
    if policy == Policy("last", "none", "drop"):
        assert kinds == {"drop", "key", "host"}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_host_set_is_the_rules_and_shrinks_with_what_is_read(program, tmp_path, dialect):
    stream = fold_corpus()
    events = list(iter_frames(stream))
    got = _decisions(program, dialect, stream, Policy(), tmp_path)
    default = _against_the_definition(stream, got, Policy(), dialect)
    if dialect == "protobufjs":
        codecs = {t: ops.codec_for(p, dialect) for t, p in TYPES.items()}

        def high(topic, body):
            try:
                return not codecs[topic].decode(body).mediaId.isascii()
            except proto.DecodeError:
                return False
        assert default == {i for i, (topic, body) in enumerate(events) if topic in TYPES and high(topic, body)}
    for policy in POLICIES[1:]:
        got = _decisions(program, dialect, stream, policy, tmp_path)
        host = {i for i, words in enumerate(got) if words == ["host"]}
        assert host <= default, policy
        read = {STATUS_ID: not (policy.status == "all" and policy.undecoded == "keep"),
                PROGRESS_ID: not (policy.progress == "all" and policy.undecoded == "keep"
                                  or policy.progress == "none" and policy.undecoded == "drop")}
        assert host == {i for i in default if read[events[i][0]]}, policy


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", [Policy(), Policy("last", "per-status", "drop")], ids=policy_id)
def test_the_decision_agrees_with_the_definition_on_the_wire_edges(program, tmp_path, policy, dialect):
    """Both policies read both topics; the second keys a progress by its status too."""
    stream = wire_edges.stream()
    got = _decisions(program, dialect, stream, policy, tmp_path)
    host = _against_the_definition(stream, got, policy, dialect)
    print(f"{dialect}: {len(got)} frames, {len(host)} left to the host")
    assert len(got) == 2 * len(wire_edges.bodies()) and sum(words[0] == "key" for words in got) > 4000
    assert len(host) <= wire_edges.HOST_CAP[dialect] * len(got)
    if dialect == "protobufjs":
        want = wire_edges.expected(dialect)
        assert host == {i for i, v in enumerate(want) if v is not None and not v.media_id.isascii()}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_small_mixed_stream(program, tmp_path, policy, dialect):
    stream = mixed_stream()
    _against_the_definition(stream, _decisions(program, dialect, stream, policy, tmp_path), policy, dialect)


def test_the_key_hash_helper():
    from beholder_amd.ops import gpu_fold
    assert gc.key_hash(b"m", STATUS_ID) != gc.key_hash(b"m", PROGRESS_ID) != gc.key_hash(b"m", PROGRESS_ID, 1)
    assert gc.key_hash(b"m", PROGRESS_ID, -1) == gc.key_hash(b"m", PROGRESS_ID, 0xFFFFFFFF)
    assert all(0 <= gc.key_hash(b, t, s) <= gpu_fold.ALL_ONES
               for b in (b"", b"abc") for t in (1, 2) for s in (0, 64, -1))
    assert [gc.policy_flags(p) for p in POLICIES[:4]] == [18, 2, 22, 6]
