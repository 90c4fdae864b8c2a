"""``compare``'s definition (beholder_amd/compare.py compare_cpu): its laws, held to
``collections.Counter`` arithmetic written here and not to the code under test, its links to the
other capture commands, ``compare_file`` and the command."""
from __future__ import annotations

import io
import json
import random
import subprocess
import sys
from collections import Counter

import pytest

from beholder_amd import coalesce as co, compare as cm, dedupe as dd, extract as ex, shard as sh, thin as th
from beholder_amd.bench.generator import Workload
from beholder_amd.compare import Comparison, Policy, Side, compare_cpu, compare_file
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from compare_cases import (POLICIES, capped_pair, contents, copies, corpus, distinct, pieces, policy_id, shuffled,
                           small_pairs)

PAIRS = sorted(small_pairs())
policies = pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
pairs = pytest.mark.parametrize("pair", PAIRS)


def _frame_count(data: bytes) -> int:
    return len(pieces(data))


# ---- the laws ---------------------------------------------------------------------------------------

@pairs
@policies
def test_the_outputs_are_the_multiset_differences(pair, policy):
    a, b = small_pairs()[pair]
    in_a, in_b = Counter(contents(a, policy)), Counter(contents(b, policy))
    c = compare_cpu(a, b, policy)
    assert Counter(contents(c.a.data)) == in_a - in_b
    assert Counter(contents(c.b.data)) == in_b - in_a
    assert c.matched == sum((in_a & in_b).values())
    assert c.common == len(in_a.keys() & in_b.keys())
    assert (c.a.distinct, c.b.distinct) == (len(in_a), len(in_b))
    assert c.topics == policy.topics
    for side, data in ((c.a, a), (c.b, b)):
        parts = pieces(data)
        assert side.frames == len(parts) == side.skipped + c.matched + len(side.indices)
        assert side.skipped == len(parts) - len(contents(data, policy))
        assert side.indices == sorted(set(side.indices))
        assert side.data == b"".join(parts[i] for i in side.indices)
    assert c.equal == (in_a == in_b)


@pairs
@policies
def test_the_surplus_occurrences_are_the_last_ones(pair, policy):
    a, b = small_pairs()[pair]
    c = compare_cpu(a, b, policy)
    for side, data, other in ((c.a, a, b), (c.b, b, a)):
        theirs = Counter(contents(other, policy))
        seen, want = Counter(), []
        for i, (topic, content) in enumerate((p[4], p[4:]) for p in pieces(data)):
            if policy.takes_part(topic):
                seen[content] += 1
                if seen[content] > theirs[content]:
                    want.append(i)
        assert side.indices == want


@pairs
@policies
def test_a_capture_equals_itself_and_the_sides_swap(pair, policy):
    a, b = small_pairs()[pair]
    same = compare_cpu(a, a, policy)
    assert same.equal and same.order_breaks == 0
    assert same.matched == len(contents(a, policy)) == same.a.frames - same.a.skipped
    assert same.a == same.b == Side(b"", [], _frame_count(a), same.a.skipped, same.a.distinct)
    ab, ba = compare_cpu(a, b, policy), compare_cpu(b, a, policy)
    assert (ba.a, ba.b, ba.matched, ba.common, ba.topics) == (ab.b, ab.a, ab.matched, ab.common, ab.topics)
    assert (ba.order_breaks == 0) == (ab.order_breaks == 0)  # a permutation and its inverse: see the module's docstring


@pairs
def test_only_in_a_does_not_depend_on_bs_order(pair):
    a, b = small_pairs()[pair]
    want = compare_cpu(a, b)
    for seed in (1, 2):
        got = compare_cpu(a, shuffled(b, seed))
        assert got.a == want.a and got.matched == want.matched and got.common == want.common
        assert Counter(contents(got.b.data)) == Counter(contents(want.b.data))


def test_order_breaks_on_distinct_contents():
    a = distinct(40)
    parts = pieces(a)
    assert compare_cpu(a, a).order_breaks == 0
    backwards = compare_cpu(a, b"".join(parts[::-1]))
    assert backwards.equal and backwards.matched == 40 and backwards.order_breaks == backwards.matched - 1
    rotated = compare_cpu(a, b"".join(parts[1:] + parts[:1]))
    assert rotated.equal and rotated.order_breaks == 1
    # skipped and unmatched frames of either side do not count: the common frames are in one order
    fewer = compare_cpu(a + copies(3), distinct(3, 900) + b"".join(parts[::3]) + copies(1, 3))
    assert fewer.order_breaks == 0 and fewer.matched == 14 and not fewer.equal
    assert cm.order_breaks([]) == cm.order_breaks([7]) == 0 and cm.order_breaks([3, 1, 2, 0]) == 2


def test_order_breaks_against_a_plain_recount():
    """The partner of every matched frame, recomputed here by popping occurrence lists."""
    rng = random.Random(4)
    for _ in range(20):
        events = [(rng.choice((STATUS_ID, PROGRESS_ID)), b"c%d" % rng.randrange(12)) for _ in range(60)]
        other = events[:45] + [(STATUS_ID, b"new")] * 3
        rng.shuffle(other)
        where = {}
        for j, e in enumerate(other):
            where.setdefault(e, []).append(j)
        partners = [where[e].pop(0) for e in events if where.get(e)]
        c = compare_cpu(frames(events), frames(other))
        assert c.matched == len(partners)
        assert c.order_breaks == sum(1 for p, q in zip(partners, partners[1:]) if q < p)


# ---- the other commands -----------------------------------------------------------------------------

def test_against_dedupe_the_complement_of_the_kept_indices():
    for x in (corpus(), small_pairs()["mixed-itself"][0]):
        kept = dd.dedupe_cpu(x, dd.Policy("first"))
        c = compare_cpu(x, kept.data)
        assert c.b.indices == [] and c.b.data == b"" and c.order_breaks == 0
        assert c.a.indices == sorted(set(range(kept.frames)) - set(kept.indices))
        assert c.matched == len(kept.indices) == c.common == c.a.distinct == c.b.distinct
    last = dd.dedupe_cpu(corpus())  # under last the kept occurrence is not the one that is matched
    c = compare_cpu(corpus(), last.data)
    assert c.b.indices == [] and len(c.a.indices) == last.frames - len(last.indices) == 703


def test_against_thin_coalesce_and_extract_nothing_is_added_and_the_rest_is_in_order():
    """A cut of x adds nothing, and what it leaves is in x's order. The second half is a theorem
    where the cut's verdict is a function of the content (extract) or where x repeats no content
    (any cut): thin and coalesce decide by position, so they are held to it on the deduped corpus.
    On a capture with repeats they may drop an earlier occurrence of a content and keep a later
    one, and the pairing rule then matches the kept one with the earlier: see the next test."""
    x = corpus()
    once = dd.dedupe_cpu(x, dd.Policy("first")).data
    cuts = [(x, ex.extract_cpu(x, ex.Selector(topics={STATUS_ID}))),
            (x, ex.extract_cpu(x, ex.Selector(outcomes={"error"}))), (once, th.thin_cpu(once)),
            (once, th.thin_cpu(once, th.Policy(keep="first"))), (once, co.coalesce_cpu(once)),
            (x, th.thin_cpu(x)), (x, th.thin_cpu(x, th.Policy(keep="first"))), (x, co.coalesce_cpu(x))]
    for k, (whole, cut) in enumerate(cuts):
        c = compare_cpu(whole, cut.data)
        assert c.b.indices == [] and c.b.data == b""
        assert c.matched == len(cut.indices) and len(c.a.indices) == cut.frames - len(cut.indices) > 0
        assert Counter(contents(c.a.data)) == Counter(contents(whole)) - Counter(contents(cut.data))
        if k < 5:
            assert c.order_breaks == 0
            assert c.a.indices == sorted(set(range(cut.frames)) - set(cut.indices))


def test_a_cut_that_keeps_a_later_repeat_breaks_the_order():
    """x = X Y X cut down to its last two frames: the first X of x is paired with the only X of
    the cut, which lies after Y's partner. Nothing is out of order in the cut, and the definition
    says one break: with repeated contents ``order_breaks`` is about the pairing, not about the cut."""
    x = frames([(STATUS_ID, b"X"), (STATUS_ID, b"Y"), (STATUS_ID, b"X")])
    c = compare_cpu(x, b"".join(pieces(x)[1:]))
    assert c.b.indices == [] and c.a.indices == [2] and c.matched == 2 and c.order_breaks == 1


@pytest.mark.parametrize("shards", [1, 2, 7])
def test_the_shards_together_hold_exactly_the_capture(shards):
    x = corpus()
    parts = sh.shard_cpu(x, sh.Policy(shards))
    c = compare_cpu(x, b"".join(parts.data))
    assert c.equal and c.matched == parts.frames == 5711
    assert (c.order_breaks == 0) == (shards == 1)


def test_shard_by_shard_sums_to_the_whole():
    a = corpus()
    b = shuffled(b"".join(pieces(a)[::2]) + distinct(50) + b"".join(pieces(a)[:300]), 3)
    whole = compare_cpu(a, b).counts()
    for shards in (2, 7):
        in_a, in_b = sh.shard_cpu(a, sh.Policy(shards)), sh.shard_cpu(b, sh.Policy(shards))
        total = Counter()
        for k in range(shards):
            total.update(compare_cpu(in_a.data[k], in_b.data[k]).counts())
        for name, value in whole.items():
            if name not in ("order_breaks", "equal"):
                assert total[name] == value, name
    assert whole["matched"] > 2000 and whole["only_a"] > 0 and whole["only_b"] > 50


# ---- policies, framing --------------------------------------------------------------------------------

def test_policy_checks():
    assert Policy({1, 2}).topics == frozenset({1, 2}) and Policy().topics is None
    assert Policy({STATUS_ID}).takes_part(STATUS_ID) and not Policy({STATUS_ID}).takes_part(PROGRESS_ID)
    for bad in ("12", b"\x01", 3):
        with pytest.raises(TypeError):
            Policy(bad)
    with pytest.raises(TypeError):
        Policy({True})
    for bad in ({256}, {-1}):
        with pytest.raises(ValueError):
            Policy(bad)
    with pytest.raises(TypeError):
        compare_cpu(b"", b"", dd.Policy())
    assert compare_cpu(b"", b"") == Comparison() and Comparison().equal


def test_a_skipped_frame_equals_nothing():
    a = frames([(7, b"x"), (STATUS_ID, b"x"), (7, b"x")])
    c = compare_cpu(a, a, Policy({STATUS_ID}))
    assert c.equal and c.matched == 1 and c.a.skipped == c.b.skipped == 2 and c.a.distinct == 1
    c = compare_cpu(a, b"", Policy({7}))
    assert c.a.indices == [0, 2] and c.a.skipped == 1 and c.b == Side()


@pytest.mark.parametrize("side", ["A", "B"])
def test_broken_framing_names_the_side(side):
    good, bad = copies(3), copies(3)[:-2]
    with pytest.raises(ValueError, match=f"capture {side}"):
        compare_cpu(*((bad, good) if side == "A" else (good, bad)))
    with pytest.raises(ValueError, match=f"capture {side}.*truncated"):
        compare_cpu(*((b"\x01\x00", good) if side == "A" else (good, b"\x01\x00")))


# ---- compare_file -------------------------------------------------------------------------------------

def test_compare_file_outputs_and_counts(tmp_path):
    a, b = capped_pair(4096)
    want = compare_cpu(a, b)
    path_a, path_b = tmp_path / "a.bin", tmp_path / "b.bin"
    path_a.write_bytes(a)
    path_b.write_bytes(b)
    outs = [io.BytesIO(), io.BytesIO(), io.StringIO(), io.StringIO()]
    counts = compare_file(str(path_a), path_b, outs[0], outs[1], Policy(), "cpu", outs[2], outs[3])
    assert (outs[0].getvalue(), outs[1].getvalue()) == (want.a.data, want.b.data)
    assert [int(x) for x in outs[2].getvalue().split()] == want.a.indices
    assert [int(x) for x in outs[3].getvalue().split()] == want.b.indices
    assert counts == {"frames_a": 50, "frames_b": 50, "skipped_a": 0, "skipped_b": 0, "matched": 49, "only_a": 1,
                      "only_b": 1, "only_a_bytes": len(want.a.data), "only_b_bytes": len(want.b.data),
                      "distinct_a": want.a.distinct, "distinct_b": want.b.distinct, "distinct_common": want.common,
                      "order_breaks": want.order_breaks, "equal": False, "host_frames": 0}
    assert want.order_breaks > 0
    # open files, and no outputs at all
    assert compare_file(io.BytesIO(a), io.BytesIO(b)) == counts
    with pytest.raises(TypeError):
        compare_file(io.BytesIO(a), io.BytesIO(b), policy="all")
    with pytest.raises(ValueError, match="capture B"):
        compare_file(io.BytesIO(a), io.BytesIO(b[:-1]), outs[0])


def test_compare_file_beyond_the_devices_limit_names_the_shard_route(tmp_path, monkeypatch):
    import os
    path_a, path_b = tmp_path / "a.bin", tmp_path / "b.bin"
    path_a.write_bytes(copies(2))
    path_b.write_bytes(copies(2))
    sizes = {str(path_a): 2 ** 31 - 100, str(path_b): 100}
    monkeypatch.setattr(os.path, "getsize", lambda p: sizes[str(p)])
    with pytest.raises(ValueError, match=r"shard --shards N.*shard by shard"):
        compare_file(path_a, path_b, device="gpu")
    assert cm.device_limit_error(2 ** 30, 2 ** 30 - 1) is None
    assert "shard" in cm.device_limit_error(2 ** 30, 2 ** 30)
    assert cm.device_limit_error(10, 10, 1 << 29) is None and "shard" in cm.device_limit_error(10, 10, (1 << 29) + 1)
    assert compare_file(path_a, path_b)["equal"]  # the cpu path has no such limit


# ---- the command ----------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], capture_output=True, timeout=120)


def test_cli_compare(tmp_path):
    a = Workload(n_media=8, seed=5).framed(400)
    b = dd.dedupe_cpu(a).data + distinct(2)
    names = ("a.bin", "b.bin", "only_a.bin", "only_b.bin", "ia.txt", "ib.txt")
    paths = {name: str(tmp_path / name) for name in names}
    (tmp_path / "a.bin").write_bytes(a)
    (tmp_path / "b.bin").write_bytes(b)
    want = compare_cpu(a, b)
    r = _cli("compare", paths["a.bin"], paths["b.bin"], "--only-a", paths["only_a.bin"], "--only-b",
             paths["only_b.bin"], "--indices-a", paths["ia.txt"], "--indices-b", paths["ib.txt"])
    assert r.returncode == 0 and not r.stderr, r.stderr
    assert json.loads(r.stdout) == want.counts() and len(r.stdout.splitlines()) == 1
    assert (tmp_path / "only_a.bin").read_bytes() == want.a.data
    assert (tmp_path / "only_b.bin").read_bytes() == want.b.data
    assert [int(x) for x in (tmp_path / "ia.txt").read_text().split()] == want.a.indices
    assert [int(x) for x in (tmp_path / "ib.txt").read_text().split()] == want.b.indices
    assert want.b.indices == [want.b.frames - 2, want.b.frames - 1]
    # --exit-code: 3 where they differ, 0 where they do not; without it 0 either way
    assert _cli("compare", paths["a.bin"], paths["b.bin"], "--exit-code").returncode == 3
    r = _cli("compare", paths["a.bin"], paths["a.bin"], "--exit-code")
    assert r.returncode == 0 and json.loads(r.stdout)["equal"] is True
    r = _cli("compare", paths["a.bin"], paths["b.bin"], "--topic", "progress", "--topic", "7")
    assert r.returncode == 0 and json.loads(r.stdout) == compare_cpu(a, b, Policy({PROGRESS_ID, 7})).counts()


def test_cli_compare_errors(tmp_path):
    good, bad = tmp_path / "good.bin", tmp_path / "bad.bin"
    good.write_bytes(copies(3))
    bad.write_bytes(copies(3)[:-1])
    out = tmp_path / "only_a.bin"
    r = _cli("compare", str(good), str(bad), "--only-a", str(out), "--exit-code")
    assert r.returncode == 1 and b"capture B" in r.stderr and not r.stdout and not out.exists()
    assert _cli("compare", str(good), str(tmp_path / "missing.bin")).returncode == 1
    assert _cli("compare", str(good)).returncode == 2
    assert _cli("compare", str(good), str(good), "--topic", "256").returncode == 2
    assert _cli("compare", str(good), str(good), "--dialect", "upb").returncode == 2  # nothing is decoded


def test_cli_compare_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    path = tmp_path / "capture.bin"
    path.write_bytes(copies(3))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["compare", str(path), str(path), "--device", "gpu"]) == 1
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "no GPU" in err.err and not err.out
