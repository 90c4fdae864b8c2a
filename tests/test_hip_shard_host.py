"""The gfx950 shard kernels' per-frame decision (ops/hip/telemetry_shard.hpp) on a CPU, under ASan and
UBSan.

tests/native/shard_host.cpp compiles the header for the host and decides every frame of a stream
from a heap block of exactly the frame's size: a read past it is a sanitizer report here. Its lines
are held to ``shard.route_of``, the definition, for every policy in both dialects: a shard number or
drop as they are; its host lines to the rule that hands a frame to the host. Nothing is loaded into
Python under a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from beholder_amd import ops, shard as sh
from beholder_amd.models import proto
from beholder_amd.shard import DROP, Policy
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames
import wire_edges
from shard_cases import POLICIES, corpus, mixed_stream, policy_id

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
TYPES = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}
SF_UNDECODED_FIRST = 1  # telemetry_shard.hpp


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/native/Makefile's readers_host_asan rule."""
    out = str(tmp_path_factory.mktemp("shard_host") / "shard_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "shard_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _decisions(program: str, dialect: str, stream: bytes, policy: Policy, tmp_path) -> list:
    """The program's line per frame of ``stream``; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    flags = SF_UNDECODED_FIRST if policy.undecoded == "first" else 0
    r = subprocess.run([program, dialect, str(path), str(policy.shards), str(flags)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.split()


def _against_the_definition(stream: bytes, got: list, policy: Policy, dialect: str) -> set:
    """Asserts the decisions; returns the frames that went to the host."""
    route = sh.route_of(policy, dialect)
    events = list(iter_frames(stream))
    assert len(got) == len(events)
    codecs = {t: ops.codec_for(p, dialect) for t, p in TYPES.items()}
    host, bad = set(), []
    for i, ((topic, body), word) in enumerate(zip(events, got)):
        if word == "host":
            host.add(i)
            assert topic in TYPES, (i, topic)
            if dialect == "protobufjs":  # the rule in full: it decodes, and its id is not ASCII
                assert not codecs[topic].decode(body).mediaId.isascii(), (i, body)
            continue
        want = route(topic, body)
        if word != ("drop" if want is DROP else str(want)):
            bad.append((i, topic, body, word, want))
    assert not bad, (len(bad), bad[:5])
    return host


def _rule(events: list, dialect: str) -> set:
    """The frames of a protobufjs stream that the rule hands to the host: decoded, with an id that is
    not ASCII."""
    codecs = {t: ops.codec_for(p, dialect) for t, p in TYPES.items()}

    def high(topic, body):
        try:
            return not codecs[topic].decode(body).mediaId.isascii()
        except proto.DecodeError:
            return False
    return {i for i, (topic, body) in enumerate(events) if topic in TYPES and high(topic, body)}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_decision_agrees_with_the_definition_on_the_fold_corpus(program, tmp_path, policy, dialect):
    stream = corpus()
    got = _decisions(program, dialect, stream, policy, tmp_path)
    host = _against_the_definition(stream, got, policy, dialect)
    assert len(got) > 5000 and len(host) <= 0.05 * len(got)  # the comparison covers what the device decides itself
    kinds = set(got)
    if policy == Policy(1):
        assert kinds == {"0"}  # nothing depends on what a frame holds: none is read
    elif policy.undecoded == "drop":
        assert host and "drop" in kinds
    else:
        assert host and "drop" not in kinds
    numbers = {int(w) for w in kinds - {"drop", "host"}}
    assert numbers <= set(range(policy.shards))
    assert len(numbers) == policy.shards if policy.shards <= 7 else len(numbers) > 20  # some 70 ids


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", [Policy(7), Policy(256, "drop")], ids=policy_id)
def test_the_decision_agrees_with_the_definition_on_the_wire_edges(program, tmp_path, policy, dialect):
    stream = wire_edges.stream()
    got = _decisions(program, dialect, stream, policy, tmp_path)
    host = _against_the_definition(stream, got, policy, dialect)
    print(f"{dialect}: {len(got)} frames, {len(host)} left to the host")
    assert len(got) == 2 * len(wire_edges.bodies()) and len(set(got)) > 4  # the ids are few
    assert len(host) <= wire_edges.HOST_CAP[dialect] * len(got)
    if dialect == "protobufjs":
        assert host == _rule(list(wire_edges.events()), dialect)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_host_set_is_the_rules_and_empty_where_nothing_is_read(program, tmp_path, dialect):
    stream = corpus()
    events = list(iter_frames(stream))
    sets = {}
    for policy in POLICIES:
        got = _decisions(program, dialect, stream, policy, tmp_path)
        sets[policy] = {i for i, word in enumerate(got) if word == "host"}
    default = sets[Policy(2)]
    assert default
    if dialect == "protobufjs":
        assert default == _rule(events, dialect)
    for policy, host in sets.items():
        assert host == (set() if policy == Policy(1) else default), policy  # the shard count does not matter


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_small_mixed_stream(program, tmp_path, policy, dialect):
    stream = mixed_stream()
    host = _against_the_definition(stream, _decisions(program, dialect, stream, policy, tmp_path), policy, dialect)
    if dialect == "protobufjs" and policy != Policy(1):
        assert host == _rule(list(iter_frames(stream)), dialect) and host
