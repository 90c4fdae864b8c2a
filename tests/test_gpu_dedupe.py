"""``dedupe`` on the GPU (ops/hip/telemetry_dedupe.hip, ops/gpu_dedupe.py) against its definition,
``dedupe.dedupe_cpu``: every comparison is full ``Deduped`` equality (the output bytes, the kept
indices and the frame count), exact, for both forms of the hash loop and the compare loop."""
from __future__ import annotations

import functools
import io
import random

import pytest

from beholder_amd import dedupe as dd
from beholder_amd.bench.generator import Workload
from beholder_amd.dedupe import Deduped, Policy, dedupe_cpu, dedupe_gpu
from beholder_amd.ops import frame, frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_dedupe as gd, gpu_fold, hip_lib  # noqa: E402
from dedupe_cases import (POLICIES, aligned_stream, capped_stream, corpus, edge_stream, mixed_stream,  # noqa: E402
                          policy_id, three_statuses)
from telemetry_corpus import body as _body  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
methods = pytest.mark.parametrize("method", gd.METHODS)


@functools.lru_cache(maxsize=None)
def _want(data: bytes, policy: Policy) -> Deduped:
    """The definition's answer, computed once per stream and policy and never changed."""
    return dedupe_cpu(data, policy)


def _same(data: bytes, policy: Policy = Policy(), method: str = gd.DEFAULT_METHOD, **kw) -> tuple:
    """Asserts the device result against the definition; returns ``(Deduped, host_frames)``."""
    want = _want(data, policy)
    got, host_frames = gd.dedupe(data, policy, DEVICE, method=method, **kw)
    assert got.frames == want.frames and got.indices == want.indices
    assert got.data == want.data
    assert got == want and len(got.hashes) == len(got.indices)
    return want, host_frames


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for policy in POLICIES:
        assert dedupe_gpu(b"", policy, DEVICE) == dedupe_cpu(b"", policy)
        assert dedupe_cpu(b"", policy) == Deduped(keep=policy.keep, topics=policy.topics)
        for method in gd.METHODS:
            assert gd.dedupe(b"", policy, DEVICE, method=method) == (dedupe_cpu(b"", policy), 0)


@methods
@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic, method):
    for body in (_body(b"m-1", 3), b"", b"\x2e"):
        data = frames([(topic, body)])
        for policy in POLICIES:
            want, host_frames = _same(data, policy, method)
            assert want.indices == [0] and want.data == data and host_frames == 0
    one = frames([(topic, b"x")])
    assert dedupe_gpu(one, Policy(), DEVICE) == dedupe_cpu(one)  # the public call


@methods
@pytest.mark.parametrize("keep", dd.KEEP_MODES)
def test_257_copies_of_one_frame(keep, method):
    """Block 0 is full and block 1 holds a single frame."""
    data = frames([(STATUS_ID, _body(b"m", 5))] * 257)
    want, host_frames = _same(data, Policy(keep), method)
    assert want.indices == ([256] if keep == "last" else [0]) and host_frames == 0


@methods
@pytest.mark.parametrize("keep", dd.KEEP_MODES)
@pytest.mark.parametrize("where", [0, 255, 256, 257])
def test_257_copies_and_one_different_frame(where, keep, method):
    events = [(STATUS_ID, _body(b"m", 5))] * 257
    events.insert(where, (STATUS_ID, _body(b"m", 4)))
    want, _ = _same(frames(events), Policy(keep), method)
    copies = [i for i in range(258) if i != where]
    assert want.indices == sorted([where, copies[-1] if keep == "last" else copies[0]])


@methods
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_edge_pairs(policy, method):
    """Contents that differ in the topic byte, the last byte or the first body byte only, strict
    prefixes, one-byte and empty bodies; then contents of 3, 4, 5, 7, 8 and 9 bytes starting at
    every offset mod 8."""
    want, _ = _same(edge_stream(), policy, method)
    if policy.topics is None:
        assert len(want.indices) == want.frames // 3  # every event was there three times
    want, _ = _same(aligned_stream(), policy, method)
    if policy.topics is None or STATUS_ID in policy.topics:
        assert len(want.indices) == 96 + 12  # the pads, and one of each content's eight
    _same(mixed_stream(), policy, method)
    _same(three_statuses(), policy, method)


@methods
@pytest.mark.parametrize("keep", dd.KEEP_MODES)
@pytest.mark.parametrize("hash_mask", [0, 1, 0xFF])
def test_forced_collisions_stay_exact(hash_mask, keep, method):
    """hash_mask 0 homes all contents in one slot, 1 in two, 0xFF in 256: every probe chain collides
    and the bytes decide. (The step from the last slot to slot 0 has the next test.)"""
    rng = random.Random(1)
    contents = [(rng.choice((STATUS_ID, PROGRESS_ID)), _body(b"media-%03d" % k, s)) for k in range(120) for s in (1, 2)]
    events = [rng.choice(contents) for _ in range(720)] + list(iter_frames(edge_stream()))
    rng.shuffle(events)
    data = frames(events)
    want, host_frames = _same(data, Policy(keep), method, hash_mask=hash_mask)
    assert host_frames == 0 and len(want.indices) == len(set(events)) > 200
    assert dedupe_gpu(data, Policy(keep), DEVICE, hash_mask=hash_mask) == want


@methods
@pytest.mark.parametrize("keep", dd.KEEP_MODES)
def test_a_probe_chain_wraps_at_the_tables_end(keep, method):
    """Four frames have eight slots. The two contents are chosen so that both hashes home on the
    last slot: the second content collides there and steps to slot 0."""
    homed = [b"x%d" % k for k in range(4000) if gd.frame_hash(bytes([STATUS_ID]) + b"x%d" % k) & 7 == 7][:2]
    assert len(homed) == 2 and gpu_fold.table_slots(4) == 8
    a, b = homed
    want, _ = _same(frames([(STATUS_ID, a), (STATUS_ID, b), (STATUS_ID, a), (STATUS_ID, b)]), Policy(keep), method)
    assert want.indices == ([2, 3] if keep == "last" else [0, 1])


@methods
@pytest.mark.parametrize("twice", [False, True], ids=["corpus", "corpus-twice"])
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_fold_corpus(policy, twice, method):
    data = corpus() * 2 if twice else corpus()
    want, host_frames = _same(data, policy, method)
    assert host_frames == 0 and want.frames == (11422 if twice else 5711)
    if policy.topics is None:
        assert len(want.indices) == 5008


@methods
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_cap(policy, method):
    """Contents of exactly DEDUPE_DEVICE_MAX bytes stay on the device, one byte more goes to the host."""
    data = capped_stream(gd.DEDUPE_DEVICE_MAX)
    over = sum(policy.takes_part(topic) and 1 + len(body) > gd.DEDUPE_DEVICE_MAX for topic, body in iter_frames(data))
    want, host_frames = _same(data, policy, method)
    assert host_frames == over == (0 if policy.topics == {7} else 5 if policy.topics is None
                                   else 4 if policy.topics == {STATUS_ID} else 1)
    if policy.topics is None:
        lengths = sorted(len(body) + 1 for _, body in iter_frames(want.data) if len(body) > 100)
        cap = gd.DEDUPE_DEVICE_MAX
        assert lengths == [cap, cap, cap, cap + 1, cap + 1, cap + 1]  # each content, its twin and the other topic's


@methods
def test_the_dedupe_is_deterministic(method):
    for policy in (Policy(), Policy("first")):
        first = gd.dedupe(corpus() * 2, policy, DEVICE, method=method)[0]
        again = gd.dedupe(corpus() * 2, policy, DEVICE, method=method)[0]
        assert first == again == _want(corpus() * 2, policy)
        assert first.data == again.data and first.indices == again.indices
        assert first.hashes.tolist() == again.hashes.tolist()


def test_the_hashes_that_come_back_are_frame_hash():
    data = mixed_stream()
    for method in gd.METHODS:
        got = gd.dedupe(data, Policy(topics={STATUS_ID}), DEVICE, method=method)[0]
        assert got.hashes.dtype == np.uint64
        for f, h in zip((frame(t, b) for t, b in iter_frames(got.data)), got.hashes.tolist()):
            assert h == (gd.frame_hash(f[4:]) if f[4] == STATUS_ID else 0)


@functools.lru_cache(maxsize=None)
def _shuffled_twice() -> bytes:
    """200,000 events: a Workload stream over 16 media followed by a shuffled copy of itself."""
    first = Workload(n_media=16, seed=9).framed(100_000)
    pieces = [frame(t, b) for t, b in iter_frames(first)]
    random.Random(5).shuffle(pieces)
    return first + b"".join(pieces)


@methods
@pytest.mark.parametrize("keep", dd.KEEP_MODES)
def test_larger_batch(keep, method):
    want, host_frames = _same(_shuffled_twice(), Policy(keep), method)
    assert want.frames == 200_000 and host_frames == 0 and len(want.indices) <= 100_000


@pytest.mark.parametrize("keep", dd.KEEP_MODES)
def test_dedupe_file_on_the_device_in_chunks(keep):
    """Some ten chunks, each through the device and joined on the host with the hashes the device
    sent back; contents cross chunk borders, and so do frames above the cap."""
    data = corpus() + capped_stream(gd.DEDUPE_DEVICE_MAX) + corpus()
    want = _want(data, Policy(keep))
    out, indices = io.BytesIO(), io.StringIO()
    counts = dd.dedupe_file(io.BytesIO(data), out, Policy(keep), device=DEVICE, chunk_bytes=50_000, indices_out=indices)
    assert out.getvalue() == want.data and [int(line) for line in indices.getvalue().split()] == want.indices
    assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                      "duplicates": want.frames - len(want.indices), "host_frames": 5}
    assert len(data) > 8 * 50_000
    one = io.BytesIO()
    assert dd.dedupe_file(io.BytesIO(data), one, Policy(keep), device="gpu")["kept"] == len(want.indices)
    assert one.getvalue() == want.data


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = frames([(STATUS_ID, _body(b"m", 1))] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gd.allocate(buf, offs_dev, n)
    params = gd.dedupe_params(Policy(), tables.slots)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gd.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gd.allocate(buf.to(torch.int8), offs_dev, n)
    with pytest.raises(ValueError):
        gd.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gd.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gd.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        gd.launch(tables, gd.dedupe_params(Policy(), 2 * tables.slots))  # params of another table
    with pytest.raises(ValueError):
        gd.launch(tables, params, stages=8)
    with pytest.raises(ValueError):
        gd.dedupe_params(Policy(), 6)
    with pytest.raises(ValueError):
        gd.dedupe_params(Policy(), 4, hash_mask=1 << 64)
    with pytest.raises(ValueError):
        gd.dedupe_params(Policy(), 4, method="dwords")
    with pytest.raises(TypeError):
        gd.dedupe_params("last", 4)
    with pytest.raises(ValueError):
        dedupe_gpu(data, Policy(), DEVICE, hash_mask=-1)
    with pytest.raises(ValueError):
        dedupe_gpu(data, Policy(), DEVICE, hash_mask=1 << 64)
    with pytest.raises(TypeError):
        dedupe_gpu(data, "last", DEVICE)
    with pytest.raises(ValueError):
        gd.dedupe(data, Policy(), DEVICE, method="dwords")
    with pytest.raises(ValueError):
        dedupe_gpu(data, Policy(), "cpu")
    with pytest.raises(ValueError):
        dedupe_gpu(data[:-1], Policy(), DEVICE)  # broken framing never reaches the device
