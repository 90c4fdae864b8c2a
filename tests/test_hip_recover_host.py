"""The gfx950 recover kernels' per-offset code (ops/hip/telemetry_recover.hpp: the candidate test and
the successor) on a CPU, under ASan and UBSan.

tests/native/recover_host.cpp compiles the header for the host and tests every offset of a buffer
that lies in a heap block of exactly its size: a read past it is a sanitizer report here. Its flags
and ends are held to ``recover.rules_of``, its reached set (a serial rendition of the kernels'
doubling rounds over its successors) to ``recover.recover_cpu``, and the offsets it leaves to the
host are exactly the rule's. Nothing is loaded into Python under a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from beholder_amd import ops, recover as rc
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

import recover_cases as cases  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
WF, ANCHOR, ASK_HOST = 1, 2, 4


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_normalise_host.py."""
    out = str(tmp_path_factory.mktemp("recover_host") / "recover_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "recover_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _run(program: str, dialect: str, data: bytes, max_frame: int, final: bool, resync: bool, answers, tmp_path):
    """``(flags, ends, succ, reached)`` of the program's lines; any sanitizer report fails."""
    (tmp_path / "buffer").write_bytes(data)
    (tmp_path / "answers").write_text("".join(f"{q}\n" for q in answers))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, dialect, str(tmp_path / "buffer"), str(max_frame), str(int(final)), str(int(resync)),
                        str(tmp_path / "answers")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    flags, ends, succ, reached = [], [], [], []
    for line in r.stdout.splitlines():
        word = line.split()
        if word[0] == "c":
            assert int(word[1]) == len(flags)
            flags.append(int(word[2]))
            ends.append(int(word[3]))
        elif word[0] == "s":
            assert int(word[1]) == len(succ)
            succ.append(int(word[2]))
        else:
            reached.append(int(word[1]))
    assert len(flags) == len(ends) == len(data) and len(succ) == len(data) + 1
    return flags, ends, succ, reached


def _high(b: bytes) -> bool:
    return any(c >= 0x80 for c in b)


def _asks_host(topic: int, body: bytes) -> bool:
    """The rule for a body under upb, written out on its own: the STRICT walk hands the body over at
    its first start-group; a body that is read to its end is handed over where its last mediaId span
    is not empty and that span, or in a progress message the last host span, holds a byte >= 0x80.
    An error on the way, or an empty id, decides the offset on the device."""
    spans = {}
    i, end = 0, len(body)

    def read(limit):
        nonlocal i
        v = 0
        for k in range(limit):
            if i >= end:
                return None
            b = body[i]
            i += 1
            v |= (b & 0x7f) << (7 * k)
            if not b & 0x80:
                return v
        return None
    while i < end:
        key = read(5)
        if key is None or key > 0xFFFFFFFF or key >> 3 == 0:
            return False
        field, wt = key >> 3, key & 7
        if wt == 0:
            if read(10) is None:
                return False
        elif wt == 2:
            n = read(10)
            if n is None or n > end - i:
                return False
            if field == 1 or (topic == PROGRESS_ID and field == 4):
                spans[field] = body[i:i + n]
            i += n
        elif wt in (1, 5):
            if end - i < (8 if wt == 1 else 4):
                return False
            i += 8 if wt == 1 else 4
        else:
            return wt == 3
    return bool(spans.get(1)) and any(_high(s) for s in spans.values())


def _against_the_definition(program, data: bytes, dialect: str, max_frame: int, tmp_path, final=True, resync=False):
    """Asserts every offset's flags and end, the successors and the reached set; returns the number
    of offsets left to the host."""
    policy = rc.Policy(max_frame)
    frame_end, anchor = rc.rules_of(data, policy, dialect)
    n = len(data)
    decided = rc.decided_end(n, policy, final)
    flags, ends, _, _ = _run(program, dialect, data, max_frame, final, resync, [], tmp_path)
    asked, bad = [], []
    for p in range(n):
        end = frame_end(p) if p < decided else 0
        f = flags[p]
        if bool(f & WF) != bool(end) or ends[p] != (end or n) or (f & ANCHOR and f & ASK_HOST) or (f and not f & WF):
            bad.append((p, f, ends[p], end))
            continue
        if f & ASK_HOST:
            asked.append(p)
        elif bool(f & ANCHOR) != (bool(end) and anchor(p)):
            bad.append((p, f, "anchor", anchor(p)))
    assert not bad, (len(bad), bad[:5])
    want_asked = []
    if dialect == "upb":
        for p in range(decided):
            end = frame_end(p)
            if end and data[p + 4] in (STATUS_ID, PROGRESS_ID) and (end == n or frame_end(end)) \
                    and _asks_host(data[p + 4], data[p + 5:end]):
                want_asked.append(p)
    assert asked == want_asked
    answers = [q for q in asked if anchor(q)]
    _, _, succ, reached = _run(program, dialect, data, max_frame, final, resync, answers, tmp_path)
    want = rc.recover_cpu(data, policy, dialect, final=final, resync=resync)
    # the nodes of the definition's walk: every frame it took in sync, and where each gap opened
    gap_ends = {a + length for a, length in want.gaps}
    nodes = {o for o in want.offsets if o not in gap_ends} | {a for a, _ in want.gaps}
    if resync:  # the walk starts at the first anchor, not at 0
        nodes.discard(0)
        nodes |= set(want.offsets[:1])
    assert [p for p in reached if p < decided] == sorted(nodes)
    for p in range(decided):
        end = frame_end(p)
        if end:
            assert succ[p] == end
    assert succ[n] == n and all(succ[p] == n for p in range(decided, n))
    return len(asked)


@pytest.mark.parametrize("max_frame", cases.MAX_FRAMES)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_offset_of_the_damage_cases(program, tmp_path, dialect, max_frame):
    asked = 0
    for name, data in cases.damage_cases().items():
        asked += _against_the_definition(program, data, dialect, max_frame, tmp_path)
    assert (asked > 0) == (dialect == "upb")


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_parts_that_are_not_the_last(program, tmp_path, dialect):
    """``final=False`` with and without a gap open on entry: nothing is decided in the last H - 1 offsets."""
    for name in ("damage_in_a_long_run", "gap_longer_than_two_chunks", "garbage_at_0", "intact", "one_frame"):
        data = cases.damage_cases()[name]
        for resync in (False, True):
            _against_the_definition(program, data, dialect, 64, tmp_path, final=False, resync=resync)
            _against_the_definition(program, data[3:], dialect, 64, tmp_path, final=True, resync=resync)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", cases.CORPORA)
def test_every_offset_of_the_damaged_corpora(program, tmp_path, name, dialect):
    data, _ = cases.damaged(name)
    asked = _against_the_definition(program, data, dialect, 1 << 20, tmp_path)
    print(f"{name} {dialect}: {asked} of {len(data)} offsets left to the host")
    assert asked == 0 or dialect == "upb"
