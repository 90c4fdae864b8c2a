"""``shard`` on the GPU (ops/hip/telemetry_shard.hip, ops/gpu_shard.py) against its definition,
``shard.shard_cpu``: every comparison is full ``Sharded`` equality (every shard's bytes and indices,
and the frame count), exact."""
from __future__ import annotations

import functools
import random

import pytest

from beholder_amd import ops, shard as sh
from beholder_amd.bench.generator import Workload
from beholder_amd.extract import Selector
from beholder_amd.ops import frames
from beholder_amd.shard import Policy, Sharded, shard_cpu, shard_gpu, shard_of
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_extract, gpu_fold, gpu_shard as gs, hip_lib  # noqa: E402
from shard_cases import POLICIES, corpus as _corpus, mixed_stream, pairs_stream, policy_id  # noqa: E402
from telemetry_corpus import body as _body  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
FFFD = "\ufffd"


@functools.lru_cache(maxsize=None)
def _want(data: bytes, policy: Policy, dialect: str) -> Sharded:
    return shard_cpu(data, policy, dialect)


def _same(data: bytes, policy: Policy, dialect: str = "protobufjs", public: bool = True, **kw) -> tuple:
    """Asserts the device result against the definition, for both in-block methods; returns
    ``(Sharded, host_frames)``."""
    want = _want(data, policy, dialect)
    host = set()
    for method in gs.METHODS:
        got, host_frames = gs.shard(data, policy, DEVICE, dialect, method=method, **kw)
        assert got.frames == want.frames and got.shards == want.shards and got.indices == want.indices, method
        assert got.data == want.data, method
        host.add(host_frames)
    assert len(host) == 1
    if public:
        assert shard_gpu(data, policy, DEVICE, dialect) == want  # the public call
    return want, host.pop()


@functools.lru_cache(maxsize=None)
def _extract_host_frames(dialect: str) -> int:
    return gpu_extract.extract(_corpus(), Selector(), DEVICE, dialect)[1]


def _two_ids_in_different_shards(shards: int) -> tuple:
    a = b"m-0"
    b = next(b"m-%d" % k for k in range(1, 100) if shard_of("m-%d" % k, shards) != shard_of("m-0", shards))
    return a, b


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for policy in (Policy(1), Policy(7, "drop"), Policy(256)):
        assert shard_gpu(b"", policy, DEVICE) == Sharded(policy.shards) == shard_cpu(b"", policy)
        assert gs.shard(b"", policy, DEVICE) == (Sharded(policy.shards), 0)


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (_body(b"m-1", 3), b"", b"\x2e"):
        data = frames([(topic, body)])
        for shards in (1, 2, 256):
            for undecoded in sh.UNDECODED_MODES:
                want, _ = _same(data, Policy(shards, undecoded), public=False)
                assert want.frames == 1 and sum(map(len, want.indices)) <= 1


def test_65_frames_of_one_media():
    """A wave boundary inside a shard."""
    data = frames([(STATUS_ID if i % 3 else PROGRESS_ID, _body(b"m", i % 7)) for i in range(65)])
    for shards in (1, 2, 256):
        want, host_frames = _same(data, Policy(shards))
        assert want.indices[shard_of("m", shards)] == list(range(65)) and host_frames == 0


@pytest.mark.parametrize("full", [256, 1024], ids=["tile", "block"])
@pytest.mark.parametrize("variant", ["one-media", "two-media-alternating", "last-alone-and-alone-in-its-shard"])
def test_one_frame_past_a_boundary(variant, full):
    """``full`` frames fill a tile of 256 (the running sums carry into the block's next tile), or
    the whole block of 1,024; the next unit holds a single frame."""
    shards = 8
    a, b = _two_ids_in_different_shards(shards)
    sa, sb = shard_of(a.decode(), shards), shard_of(b.decode(), shards)
    if variant == "one-media":  # one shard is full across the boundary, all the others are empty
        ids = [a] * (full + 1)
    elif variant == "two-media-alternating":
        ids = [a if i % 2 else b for i in range(full + 1)]
    else:
        ids = [a] * full + [b]
    data = frames([(STATUS_ID if i % 5 else PROGRESS_ID, _body(mid, i % 7)) for i, mid in enumerate(ids)])
    want, host_frames = _same(data, Policy(shards))
    assert host_frames == 0
    assert want.indices[sa] == [i for i, mid in enumerate(ids) if mid == a]
    assert want.indices[sb] == [i for i, mid in enumerate(ids) if mid == b]
    assert sum(bool(i) for i in want.indices) == len(set(ids))


def test_three_media_over_256_shards():
    """Mostly empty shards, and empty tiles in the totals scan: 3 blocks by 256 shards are 768 totals
    with three of them set per block; 9 blocks are 2,304 totals, past one tile of 2,048."""
    rng = random.Random(2)
    ids = [b"m-0", b"m-1", b"m-2"]
    data = frames([(rng.choice((STATUS_ID, PROGRESS_ID)), _body(rng.choice(ids), rng.randrange(7))) for _ in range(2400)])
    want, _ = _same(data, Policy(256))
    assert sum(bool(i) for i in want.indices) == len({shard_of(m.decode(), 256) for m in ids}) == 3
    many = frames([(STATUS_ID, _body(rng.choice(ids), 1)) for _ in range(8300)])
    _same(many, Policy(256, "drop"), public=False)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_fold_corpus(policy, dialect):
    want, host_frames = _same(_corpus(), policy, dialect, public=False)
    assert want.frames > 5000
    same_rule = _extract_host_frames(dialect)
    assert 0 < same_rule <= 0.05 * want.frames
    if policy == Policy(1):
        assert host_frames == 0  # the policy makes reading unnecessary
    else:
        assert host_frames == same_rule


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_small_mixed_stream(policy):
    for dialect in ops.DIALECTS:
        _same(mixed_stream(), policy, dialect, public=False)


@pytest.mark.parametrize("shape", sorted(gpu_extract.GATHER_SHAPES))
def test_both_gather_shapes(shape):
    for data in (mixed_stream(), _corpus(), pairs_stream()):
        for policy in (Policy(1), Policy(7, "drop"), Policy(256)):
            _same(data, policy, public=False, shape=shape)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_non_ascii_ids_take_the_host_path(dialect):
    rng = random.Random(4)
    plain = [b"ascii-%d" % k for k in range(20)]
    other = ["é".encode(), "メディア".encode(), b"\xff", b"\xfe", b"ok\x80", b"\xc3", b"caf\xc3\xa9",
             b"\xf0\x9f\x8e\xac"]
    events, host = [], 0
    for _ in range(600):
        mid = rng.choice(other) if rng.random() < 0.3 else rng.choice(plain)
        host += mid in other
        events.append((rng.choice((STATUS_ID, PROGRESS_ID)), _body(mid, rng.randrange(7))))
    data = frames(events)
    assert 100 < host < 300
    for policy in (Policy(2), Policy(7, "drop"), Policy(256)):
        want, host_frames = _same(data, policy, dialect)
        assert host_frames == host
    two = frames([(t, _body(mid, s)) for s, mid in enumerate((b"\xff", b"\xfe", b"\xff", b"\xfe"))
                  for t in (STATUS_ID, PROGRESS_ID)])
    for undecoded in sh.UNDECODED_MODES:
        want, host_frames = _same(two, Policy(64, undecoded), dialect)
        assert host_frames == 8
        if dialect == "protobufjs":  # one media, U+FFFD: all eight in its shard
            assert want.indices[shard_of(FFFD, 64)] == list(range(8)) and shard_of(FFFD, 64) != 0
        elif undecoded == "first":  # upb raises on invalid UTF-8: eight errors
            assert want.indices[0] == list(range(8))
        else:
            assert not any(want.indices)


def test_the_shard_is_deterministic():
    policy = Policy(64)
    first = shard_gpu(_corpus(), policy, DEVICE)
    assert first == shard_gpu(_corpus(), policy, DEVICE) == _want(_corpus(), policy, "protobufjs")


def test_larger_batch():
    data = Workload(n_media=256, seed=9).framed(200_000)
    want, host_frames = _same(data, Policy(8), public=False)
    assert want.frames == 200_000 == sum(map(len, want.indices)) and all(want.indices) and host_frames == 0


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_shard_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device and written before the next is read."""
    import io
    data = _corpus()
    policy = Policy(7)
    want = _want(data, policy, dialect)
    outs, indices = [io.BytesIO() for _ in range(7)], [io.StringIO() for _ in range(7)]
    counts = sh.shard_file(io.BytesIO(data), outs, policy, device=DEVICE, dialect=dialect, chunk_bytes=30_000,
                           indices_outs=indices)
    assert [o.getvalue() for o in outs] == want.data
    assert [[int(line) for line in i.getvalue().split()] for i in indices] == want.indices
    assert counts == {"frames": want.frames, "kept": want.frames, "kept_bytes": len(data),
                      "host_frames": _extract_host_frames(dialect),
                      "per_shard": [{"frames": len(i), "bytes": len(d)} for i, d in zip(want.indices, want.data)]}
    assert len(data) > 7 * 30_000


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = frames([(STATUS_ID, _body(b"m", 1))] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gs.allocate(buf, offs_dev, n, 4)
    params = gs.shard_params(Policy(4))

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gs.allocate(buf, offs_dev.to(torch.int64), n, 4)  # wrong dtype
    with pytest.raises(ValueError):
        gs.allocate(buf.to(torch.int8), offs_dev, n, 4)
    with pytest.raises(ValueError):
        gs.allocate(buf.cpu(), offs_dev.cpu(), n, 4)  # host tensors
    with pytest.raises(ValueError):
        gs.allocate(buf, offs_dev, n + 1, 4)  # offs is not n + 1
    with pytest.raises(ValueError):
        gs.allocate(buf[:0], offs_dev[:1], 0, 4)  # n >= 1
    for shards in (0, 257, -1):
        with pytest.raises(ValueError):
            gs.allocate(buf, offs_dev, n, shards)
    with pytest.raises(ValueError):
        gs.route(tables, params, dialect="proto2")
    with pytest.raises(ValueError):
        gs.route(tables, gs.shard_params(Policy(5)))  # params of another shard count
    with pytest.raises(ValueError):
        gs.partition(tables, method="sort")
    with pytest.raises(ValueError):
        gs.partition(tables, stages=8)
    with pytest.raises(TypeError):
        gs.shard_params(4)
    with pytest.raises(TypeError):
        shard_gpu(data, 4, DEVICE)  # a non-Policy
    with pytest.raises(ValueError):
        shard_gpu(data, Policy(4), DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        shard_gpu(data, Policy(4), "cpu")
    with pytest.raises(ValueError):
        gs.shard(data, Policy(4), DEVICE, shape="scatter")
    with pytest.raises(ValueError):
        gs.shard(data, Policy(4), DEVICE, method="sort")
    with pytest.raises(ValueError):
        shard_gpu(data[:-1], Policy(4), DEVICE)  # broken framing never reaches the device
