"""The gfx950 dedupe kernels' per-frame code (ops/hip/telemetry_dedupe.hpp) on a CPU, under ASan and
UBSan.

tests/native/dedupe_host.cpp compiles the header for the host and reads every frame of a stream from
a heap block of exactly the frame's size: a read past it is a sanitizer report here. Its kind and
hash per frame are held to ``dedupe.Policy`` and ``gpu_dedupe.frame_hash``, its answer for pairs of
frames to equality of the contents, for every topic set and both forms of the loops. Nothing is
loaded into Python under a sanitizer."""
from __future__ import annotations

import os
import random
import shutil
import subprocess

import pytest

from beholder_amd.dedupe import Policy
from beholder_amd.transport.framing import iter_frames
from dedupe_cases import TOPIC_SETS, aligned_stream, capped_stream, corpus, edge_stream, mixed_stream

np = pytest.importorskip("numpy")  # gpu_dedupe imports it
from beholder_amd.ops import gpu_dedupe as gd  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
STREAMS = {"corpus": corpus, "edge": edge_stream, "aligned": aligned_stream, "mixed": mixed_stream,
           "capped": lambda: capped_stream(gd.DEDUPE_DEVICE_MAX)}


def _topics_id(topics) -> str:
    return "all" if topics is None else "+".join(map(str, sorted(topics)))


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/native/Makefile's readers_host_asan rule."""
    out = str(tmp_path_factory.mktemp("dedupe_host") / "dedupe_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "dedupe_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _run(program: str, method: str, stream: bytes, topics, pairs, tmp_path) -> tuple:
    """``(the program's line per frame, its answer per pair)``; any sanitizer report fails."""
    path = tmp_path / "stream"
    path.write_bytes(stream)
    params = gd.dedupe_params(Policy(topics=topics), 2)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, method, str(path)] + [str(w) for w in params.topics] + [f"{i}:{j}" for i, j in pairs],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    lines = r.stdout.splitlines()
    n = len(lines) - len(pairs)
    answers = []
    for (i, j), line in zip(pairs, lines[n:]):
        name, answer = line.split()
        assert name == f"{i}:{j}"
        answers.append(answer == "1")
    return lines[:n], answers


def _pairs(events: list, topics, rng: random.Random) -> list:
    """Pairs of frames that take part on the device: every frame with the next one of its content
    (equal), with its neighbour and with a random one (mostly different)."""
    policy = Policy(topics=topics)
    rows = [i for i, (topic, body) in enumerate(events)
            if policy.takes_part(topic) and 1 + len(body) <= gd.DEDUPE_DEVICE_MAX]
    if not rows:
        return []
    pairs, seen = [], {}
    for k, i in enumerate(rows):
        if events[i] in seen:
            pairs.append((seen[events[i]], i))
        seen[events[i]] = i
        pairs.append((i, rows[(k + 1) % len(rows)]))
        pairs.append((rng.choice(rows), i))
    return pairs[:3000]


@pytest.mark.parametrize("method", gd.METHODS)
@pytest.mark.parametrize("topics", TOPIC_SETS, ids=_topics_id)
@pytest.mark.parametrize("stream", sorted(STREAMS))
def test_kind_hash_and_equality_agree_with_the_definition(program, tmp_path, stream, topics, method):
    data = STREAMS[stream]()
    events = list(iter_frames(data))
    pairs = _pairs(events, topics, random.Random(2))
    lines, answers = _run(program, method, data, topics, pairs, tmp_path)
    assert len(lines) == len(events)
    policy = Policy(topics=topics)
    kinds = set()
    for i, ((topic, body), line) in enumerate(zip(events, lines)):
        content = bytes([topic]) + body
        if not policy.takes_part(topic):
            want = "keep"
        elif len(content) > gd.DEDUPE_DEVICE_MAX:
            want = "host"
        else:
            want = f"row {gd.frame_hash(content):016x}"
        assert line == want, (i, topic, body[:40])
        kinds.add(want.split()[0])
    assert answers == [events[i] == events[j] for i, j in pairs]
    if pairs:
        assert any(answers) and not all(answers)
    if stream == "capped":  # one byte over the cap goes to the host, the cap itself does not
        lengths = {1 + len(body) for (topic, body), line in zip(events, lines) if line == "host"}
        assert lengths == ({gd.DEDUPE_DEVICE_MAX + 1} if topics != frozenset({7}) else set())
        assert kinds == ({"row", "host"} if topics is None else {"keep"} if topics == frozenset({7})
                         else {"keep", "row", "host"})
    if stream == "corpus":
        assert len(events) > 5000 and kinds == ({"row"} if topics is None else {"keep"} if topics == frozenset({7})
                                                else {"keep", "row"})


def test_frame_hash_is_the_folds_hash_of_the_content():
    from beholder_amd.ops import gpu_fold
    for content in (b"\x01", b"\x02abc", bytes(range(256)) * 3):
        assert gd.frame_hash(content) == gpu_fold.hash64(content)
    assert gd.frame_hash(b"\x01a") != gd.frame_hash(b"\x02a")  # the topic byte is part of the content
