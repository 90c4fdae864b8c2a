"""The gfx950 compare kernels' per-frame and per-position code (ops/hip/telemetry_compare.hpp) on a
CPU, under ASan and UBSan.

tests/native/compare_host.cpp compiles the header for the host, reads every frame of both streams
from a heap block of exactly the frame's size, sorts the rows itself with ``std::stable_sort`` and
runs the bounds rule and the match verdict over every sorted position, the bounds in heap arrays of
exactly one word per content. Its verdict and partner per frame and its counts are held to
``compare.compare_cpu`` and to the pairing rule written out here. Nothing is loaded into Python
under a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from beholder_amd.compare import compare_cpu
from compare_cases import POLICIES, capped_pair, copies, corpus, distinct, pieces, policy_id, shuffled, small_pairs

np = pytest.importorskip("numpy")  # gpu_compare imports it
from beholder_amd.ops import gpu_compare as gc  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
CAP = gc.DEDUPE_DEVICE_MAX


def _pairs() -> dict:
    both = dict(small_pairs())
    both["capped"] = capped_pair(CAP)
    both["corpus-shuffled-half"] = (corpus(), shuffled(b"".join(pieces(corpus())[::2]) + distinct(30), 2))
    both["run-edges"] = (copies(257) + distinct(5), distinct(3) + copies(256))
    return both


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of test_hip_dedupe_host.py."""
    out = str(tmp_path_factory.mktemp("compare_host") / "compare_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "compare_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _run(program: str, a: bytes, b: bytes, policy, tmp_path) -> list:
    """The program's lines; any sanitizer report fails."""
    path_a, path_b = tmp_path / "a", tmp_path / "b"
    path_a.write_bytes(a)
    path_b.write_bytes(b)
    params = gc.params_of(policy, 2)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, str(path_a), str(path_b)] + [str(w) for w in params.topics],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _rule(a: bytes, b: bytes, policy) -> tuple:
    """``(the verdict per joined frame, the device's counts)`` by the pairing rule, written out: the
    k-th occurrence of a content in A with the k-th in B. Contents above the cap are the host's."""
    parts_a, parts_b = pieces(a), pieces(b)
    n_a = len(parts_a)
    where = {}  # content -> (A's joined indices, B's)
    want = []
    for m, part in enumerate(parts_a + parts_b):
        if not policy.takes_part(part[4]):
            want.append(("skip",))
        elif len(part) - 4 > CAP:
            want.append(("host",))
        else:
            want.append(None)
            where.setdefault(part[4:], ([], []))[m >= n_a].append(m)
    counts = [0, 0, 0, 0]
    for content, (mine, theirs) in where.items():
        k = min(len(mine), len(theirs))
        digest = f"{gc.gpu_dedupe.frame_hash(content):016x}"
        for x, y in zip(mine[:k], theirs[:k]):
            want[x], want[y] = ("matched", digest, str(y)), ("matched", digest, str(x))
        for m in mine[k:] + theirs[k:]:
            want[m] = ("only", digest)
        counts = [counts[0] + k, counts[1] + bool(mine), counts[2] + bool(theirs), counts[3] + bool(mine and theirs)]
    return want, counts


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
@pytest.mark.parametrize("pair", sorted(_pairs()))
def test_verdicts_partners_and_counts_agree_with_the_definition(program, tmp_path, pair, policy):
    a, b = _pairs()[pair]
    lines = _run(program, a, b, policy, tmp_path)
    want, counts = _rule(a, b, policy)
    got = [tuple(line.split()) for line in lines]
    assert len(got) == len(want) + 1
    assert got[:-1] == want
    assert got[-1] == ("counts",) + tuple(map(str, counts))
    # and the definition itself: the frames only in one capture, and the order breaks from the partners
    c = compare_cpu(a, b, policy)
    n_a = c.a.frames
    hosts = sum(w == ("host",) for w in want)
    if hosts == 0:
        assert [m for m, w in enumerate(got[:n_a]) if w[0] == "only"] == c.a.indices
        assert [m - n_a for m, w in enumerate(got[:-1]) if m >= n_a and w[0] == "only"] == c.b.indices
        assert (c.matched, c.a.distinct, c.b.distinct, c.common) == tuple(counts)
        partners = [int(w[2]) for w in got[:n_a] if w[0] == "matched"]
        assert sum(1 for p, q in zip(partners, partners[1:]) if q < p) == c.order_breaks
        skipped = (sum(w[0] == "skip" for w in got[:n_a]), sum(w[0] == "skip" for w in got[n_a:-1]))
        assert skipped == (c.a.skipped, c.b.skipped)
    else:
        assert pair == "capped" and hosts == {None: 10, frozenset({1}): 8, frozenset({2}): 2}[policy.topics]
        assert c.matched >= counts[0]
