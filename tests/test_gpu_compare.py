"""``compare`` on the GPU (ops/hip/telemetry_compare.hip, ops/gpu_compare.py) against its definition,
``compare.compare_cpu``: every comparison is full ``Comparison`` equality (both sides' bytes, indices
and counts, the pairs, the common contents and the order breaks), exact. ``host_frames`` is held to
the number of participating frames above the cap, so the device cannot pass by leaving its work to
the host."""
from __future__ import annotations

import functools
import io
import random

import pytest

from beholder_amd import coalesce as co, compare as cm, dedupe as dd, thin as th
from beholder_amd.compare import Comparison, Policy, compare_cpu, compare_gpu
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_compare as gc, gpu_dedupe as gd, gpu_fold, gpu_transitions, hip_lib  # noqa: E402
from compare_cases import (POLICIES, capped_pair, copies, corpus, distinct, over_cap, pieces, policy_id,  # noqa: E402
                           shuffled, small_pairs)
from telemetry_corpus import body as _body  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
CAP = gc.DEDUPE_DEVICE_MAX


@functools.lru_cache(maxsize=None)
def _want(a: bytes, b: bytes, policy: Policy) -> Comparison:
    """The definition's answer, computed once per pair and policy and never changed."""
    return compare_cpu(a, b, policy)


def _same(a: bytes, b: bytes, policy: Policy = Policy(), **kw) -> Comparison:
    """Asserts the device result against the definition and ``host_frames`` against the frames above
    the cap; returns the definition's ``Comparison``."""
    want = _want(a, b, policy)
    got, host_frames = gc.compare(a, b, policy, DEVICE, **kw)
    assert got.a.indices == want.a.indices and got.b.indices == want.b.indices
    assert got.a == want.a and got.b == want.b
    assert (got.matched, got.common, got.order_breaks) == (want.matched, want.common, want.order_breaks)
    assert got == want
    assert host_frames == over_cap(a, policy, CAP) + over_cap(b, policy, CAP)
    return want


def test_empty_captures_launch_nothing(monkeypatch):
    def no_library():
        raise AssertionError("two empty captures must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for policy in POLICIES:
        assert gc.compare(b"", b"", policy, DEVICE) == (compare_cpu(b"", b"", policy), 0)
        assert compare_gpu(b"", b"", policy, DEVICE) == Comparison(topics=policy.topics)


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_one_side_empty(policy):
    data = small_pairs()["mixed-itself"][0]
    want = _same(data, b"", policy)
    assert want.b == cm.Side() and want.matched == 0 and len(want.a.indices) == want.a.frames - want.a.skipped
    want = _same(b"", data, policy)
    assert want.a == cm.Side() and want.matched == 0 and len(want.b.indices) == want.b.frames - want.b.skipped
    one = frames([(STATUS_ID, b"x")])
    assert _same(one, b"").a.indices == [0] and _same(b"", one).b.indices == [0]


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_one_frame_each(topic):
    for body in (_body(b"m-1", 3), b"", b"\x2e"):
        one = frames([(topic, body)])
        for policy in POLICIES:
            want = _same(one, one, policy)
            assert want.equal and want.matched == int(policy.takes_part(topic))
        other = frames([(topic, body + b"\x00")])
        want = _same(one, other)
        assert want.matched == 0 and want.a.indices == want.b.indices == [0] and want.common == 0
    assert compare_gpu(one, other, Policy(), DEVICE) == compare_cpu(one, other)  # the public call


@pytest.mark.parametrize("in_b", [256, 257, 258])
def test_257_copies_against_the_block_edge(in_b):
    """The run holds 257 frames of A and then B's: the 256-lane block edge lies inside the run, one
    position before the side boundary."""
    want = _same(copies(257), copies(in_b))
    assert want.matched == min(257, in_b) and want.a.indices == list(range(in_b, 257))
    assert want.b.indices == list(range(257, in_b)) and want.order_breaks == 0


@pytest.mark.parametrize("swap", [False, True], ids=["ab", "ba"])
@pytest.mark.parametrize("in_b", [0, 1, 2049])
@pytest.mark.parametrize("in_a", [2047, 2048, 2049])
def test_one_run_around_the_sorts_block(in_a, in_b, swap):
    """One content ``in_a`` times in A and ``in_b`` times in B, among a few others so that there is a
    sort pass: the side boundary and the run's end lie on either side of the sort's 2,048-element block."""
    assert gpu_transitions.SORT_BLOCK == 2048
    a, b = copies(in_a) + distinct(2), distinct(3) + copies(in_b)
    if swap:
        a, b = b, a
    want = _same(a, b)
    assert want.matched == min(in_a, in_b) + 2 and want.common == (2 if in_b == 0 else 3)
    assert len(want.a.indices) + len(want.b.indices) == abs(in_a - in_b) + 1


def _by_home(count: int, joined: int) -> list:
    """``count`` status bodies whose contents home on pairwise different slots of the table for
    ``joined`` frames, in ascending order of the slot: with no collision that is the order of their
    content numbers, so of their runs in the sorted events."""
    mask = gpu_fold.table_slots(joined) - 1
    homes = {}
    for k in range(4000):
        homes.setdefault(gd.frame_hash(bytes([STATUS_ID]) + b"x%d" % k) & mask, b"x%d" % k)
    assert len(homes) >= count
    return [homes[h] for h in sorted(homes)][:count]


@pytest.mark.parametrize("swap", [False, True], ids=["a-first", "b-first"])
def test_runs_of_one_side_only_first_and_last_in_the_sorted_order(swap):
    """Six contents in the order of their runs: the first run is all A (3 frames), the last all B
    (2 frames), the others common; and the same with the captures swapped."""
    first, *middle, last = _by_home(6, 16)
    a = frames([(STATUS_ID, x) for x in [first, middle[0], first, middle[1], middle[2], first, middle[3], middle[0]]])
    b = frames([(STATUS_ID, x) for x in [middle[3], last, middle[2], middle[1], middle[0], last, middle[2], middle[1]]])
    assert len(pieces(a)) + len(pieces(b)) == 16
    want = _same(*((b, a) if swap else (a, b)))
    mine, theirs = (want.b, want.a) if swap else (want.a, want.b)
    assert mine.indices == [0, 2, 5, 7] and theirs.indices == [1, 5, 6, 7] and want.matched == 4 and want.common == 4


@pytest.mark.parametrize("count", [1, 256, 257, 65537])
def test_content_counts_around_the_sort_passes(count):
    """1 content: no sort pass; 256 and 257: one and two; 65,537: three. B is A rotated by a third,
    with every fifth frame again."""
    assert [gpu_transitions.sort_passes(c) for c in (1, 256, 257, 65536, 65537)] == [0, 1, 2, 2, 3]
    a = distinct(count)
    parts = pieces(a)
    cut = count // 3
    want = _same(a, b"".join(parts[cut:] + parts[:cut] + parts[::5]))
    assert want.matched == want.a.distinct == want.b.distinct == want.common == count and want.a.indices == []
    assert want.b.indices == list(range(count, count + len(parts[::5]))) and want.order_breaks == (1 if cut else 0)


@pytest.mark.parametrize("hash_mask", [0, 1, 0xFF])
def test_forced_collisions_stay_exact(hash_mask):
    """hash_mask 0 homes all contents in one slot, 1 in two, 0xFF in 256: every probe chain collides
    and the bytes decide. (The step from the last slot to slot 0 has the next test.)"""
    rng = random.Random(1)
    contents = [(rng.choice((STATUS_ID, PROGRESS_ID)), _body(b"media-%03d" % k, s)) for k in range(120) for s in (1, 2)]
    a = frames([rng.choice(contents) for _ in range(500)]) + small_pairs()["mixed-edge"][1]
    b = frames([rng.choice(contents) for _ in range(400)]) + small_pairs()["edge-twice"][1]
    want = _same(a, b, hash_mask=hash_mask)
    assert want.matched > 200 and want.a.indices and want.b.indices and want.order_breaks > 50
    assert compare_gpu(a, b, Policy(), DEVICE, hash_mask=hash_mask) == want


def test_a_probe_chain_wraps_at_the_tables_end():
    """Four joined frames have eight slots. The two contents are chosen so that both hashes home on
    the last slot: the second content collides there and steps to slot 0."""
    homed = [b"x%d" % k for k in range(4000) if gd.frame_hash(bytes([STATUS_ID]) + b"x%d" % k) & 7 == 7][:2]
    assert len(homed) == 2 and gpu_fold.table_slots(4) == 8
    x, y = homed
    want = _same(frames([(STATUS_ID, x), (STATUS_ID, y)]), frames([(STATUS_ID, y), (STATUS_ID, x)]))
    assert want.equal and want.matched == 2 and want.order_breaks == 1
    want = _same(frames([(STATUS_ID, x), (STATUS_ID, y), (STATUS_ID, x)]), frames([(STATUS_ID, y)]))
    assert want.a.indices == [0, 2] and want.matched == 1


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_cap(policy):
    """Contents of exactly DEDUPE_DEVICE_MAX bytes stay on the device, one byte more goes to the
    host, which pairs them by the same rule: matched across the captures and out of order."""
    a, b = capped_pair(CAP)
    for x, y in ((a, b), (b, a)):
        over = over_cap(x, policy, CAP) + over_cap(y, policy, CAP)
        assert over == (0 if policy.topics == {7} else 10 if policy.topics is None
                        else 8 if policy.topics == {STATUS_ID} else 2)
        want = _same(x, y, policy)  # holds host_frames to `over`
        if policy.topics is None:
            assert want.matched == 49 and len(want.a.indices) == len(want.b.indices) == 1 and want.order_breaks > 0
            assert len(want.a.data) == len(want.b.data) == 4 + CAP + 1  # both are contents above the cap


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
@pytest.mark.parametrize("pair", sorted(small_pairs()))
def test_small_pairs_under_every_topic_set(pair, policy):
    a, b = small_pairs()[pair]
    _same(a, b, policy)


@functools.lru_cache(maxsize=None)
def _corpus_pairs() -> dict:
    x = corpus()
    return {"itself": x, "shuffled": shuffled(x), "dedupe": dd.dedupe_cpu(x).data, "thin": th.thin_cpu(x).data,
            "coalesce": co.coalesce_cpu(x).data, "twice": x + x}


@pytest.mark.parametrize("policy", [POLICIES[0], POLICIES[2]], ids=policy_id)
@pytest.mark.parametrize("other", ["itself", "shuffled", "dedupe", "thin", "coalesce", "twice"])
def test_fold_corpus(other, policy):
    x, y = corpus(), _corpus_pairs()[other]
    want = _same(x, y, policy)
    assert want.a.frames == 5711
    if policy.topics is None:
        assert want.a.distinct == 5008 and want.common == want.b.distinct
        assert want.equal == (other in ("itself", "shuffled"))
        assert len(want.a.indices) == {"itself": 0, "shuffled": 0, "dedupe": 703, "thin": 137, "twice": 0}.get(
            other, len(want.a.indices))
        if other in ("itself", "twice"):
            assert want.order_breaks == 0
        if other == "twice":
            assert want.b.indices == list(range(5711, 11422))
    if other != "itself":
        _same(y, x, policy)


def test_the_comparison_is_deterministic():
    x, y = corpus(), _corpus_pairs()["shuffled"]
    first, again = gc.compare(x, y + x, Policy(), DEVICE), gc.compare(x, y + x, Policy(), DEVICE)
    assert first == again == (_want(x, y + x, Policy()), 0)


def test_compare_file_on_the_device(tmp_path):
    a, b = capped_pair(CAP)
    a, b = corpus() + a, shuffled(b + corpus(), 9)
    want = _want(a, b, Policy())
    path_a, path_b = tmp_path / "a.bin", tmp_path / "b.bin"
    path_a.write_bytes(a)
    path_b.write_bytes(b)
    outs = [io.BytesIO(), io.BytesIO(), io.StringIO(), io.StringIO()]
    counts = cm.compare_file(path_a, path_b, outs[0], outs[1], Policy(), DEVICE, outs[2], outs[3])
    assert (outs[0].getvalue(), outs[1].getvalue()) == (want.a.data, want.b.data)
    assert [int(x) for x in outs[2].getvalue().split()] == want.a.indices
    assert [int(x) for x in outs[3].getvalue().split()] == want.b.indices
    assert counts == want.counts(host_frames=10) and not counts["equal"] and counts["matched"] == 5711 + 49
    assert cm.compare_file(io.BytesIO(a), io.BytesIO(a), device="gpu") == _want(a, a, Policy()).counts(host_frames=10)


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    a = frames([(STATUS_ID, _body(b"m", 1))] * 2)
    n, offs = gpu_fold.index(a)
    joined = gc.join_offsets(offs, offs, len(a))
    assert joined.tolist() == [0, len(a) // 2, len(a), 3 * len(a) // 2, 2 * len(a)] and joined.dtype == np.int32
    buf, offs_dev = gc.upload(a, a, joined, DEVICE)
    assert buf.cpu().numpy().tobytes() == a + a
    tables = gc.allocate(buf, offs_dev, 2 * n, n)
    assert tables.t.slots == gpu_fold.table_slots(2 * n) and tables.t.counters.numel() == gc.N_COUNTERS

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gc.allocate(buf, offs_dev.to(torch.int64), 2 * n, n)  # wrong dtype
    with pytest.raises(ValueError):
        gc.allocate(buf.cpu(), offs_dev.cpu(), 2 * n, n)  # host tensors
    with pytest.raises(ValueError):
        gc.allocate(buf, offs_dev, 2 * n + 1, n)  # offs is not n + 1
    with pytest.raises(ValueError):
        gc.allocate(buf, offs_dev, 2 * n, 2 * n + 1)  # more frames of A than frames
    with pytest.raises(ValueError):
        gc.allocate(buf, offs_dev, 2 * n, -1)
    with pytest.raises(ValueError):
        gc.classify(tables, gc.params_of(Policy(), 2 * tables.t.slots))  # params of another table
    with pytest.raises(TypeError):
        gc.params_of(dd.Policy(), 8)
    with pytest.raises(ValueError):
        compare_gpu(a, a, Policy(), DEVICE, hash_mask=-1)
    with pytest.raises(ValueError):
        compare_gpu(a, a, Policy(), DEVICE, hash_mask=1 << 64)
    with pytest.raises(TypeError):
        compare_gpu(a, a, "all", DEVICE)
    with pytest.raises(ValueError):
        compare_gpu(a, a, Policy(), "cpu")
    with pytest.raises(ValueError, match="capture A"):
        compare_gpu(a[:-1], a, Policy(), DEVICE)  # broken framing never reaches the device
    with pytest.raises(ValueError, match="capture B"):
        compare_gpu(a, a[:-1], Policy(), DEVICE)
