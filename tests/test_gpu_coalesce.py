"""``coalesce`` on the GPU (ops/hip/telemetry_coalesce.hip, ops/gpu_coalesce.py) against its
definition, ``coalesce.coalesce_cpu``: every comparison is full ``Coalesced`` equality (the output
bytes, the kept indices, their keys and the frame count), exact."""
from __future__ import annotations

import functools
import itertools
import random

import pytest

from beholder_amd import ops
from beholder_amd.bench.generator import Workload
from beholder_amd.coalesce import Coalesced, Policy, coalesce_cpu, coalesce_gpu
from beholder_amd.extract import Selector
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_coalesce as gc, gpu_extract, gpu_fold, hip_lib  # noqa: E402
from coalesce_cases import POLICIES, mixed_stream, policy_id  # noqa: E402
from extract_cases import collision_pairs  # noqa: E402
from telemetry_corpus import body as _body, fold_corpus as _corpus  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
FFFD = "\ufffd"


def _same(data: bytes, policy: Policy = Policy(), dialect: str = "protobufjs", **kw) -> tuple:
    """Asserts the device result against the definition; returns ``(Coalesced, host_frames)``."""
    want = coalesce_cpu(data, policy, dialect)
    got, host_frames = gc.coalesce(data, policy, DEVICE, dialect, **kw)
    assert got.frames == want.frames and got.indices == want.indices and got.keys == want.keys
    assert got.data == want.data
    assert coalesce_gpu(data, policy, DEVICE, dialect, **kw) == want  # the public call
    return want, host_frames


@functools.lru_cache(maxsize=None)
def _extract_host_frames(dialect: str) -> int:
    return gpu_extract.extract(_corpus(), Selector(), DEVICE, dialect)[1]


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for policy in (Policy(), Policy("all", "none", "drop")):
        assert coalesce_gpu(b"", policy, DEVICE) == Coalesced() == coalesce_cpu(b"", policy)
        assert gc.coalesce(b"", policy, DEVICE) == (Coalesced(), 0)


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (_body(b"m-1", 3), b"", b"\x2e"):
        data = frames([(topic, body)])
        for policy in POLICIES:
            want, _ = _same(data, policy)
            assert want.frames == 1 and want.data in (data, b"")


@pytest.mark.parametrize("variant", ["winner-alone-in-block-1", "winner-255-then-other-topic", "winner-0"])
def test_257_frames_of_one_key(variant):
    """Block 0 is full and block 1 holds a single frame."""
    if variant == "winner-alone-in-block-1":
        events = [(STATUS_ID, _body(b"m", i % 7)) for i in range(257)]
        kept = [256]
    elif variant == "winner-255-then-other-topic":
        events = [(STATUS_ID, _body(b"m", i % 7)) for i in range(256)] + [(9, _body(b"m", 1))]
        kept = [255, 256]
    else:
        events = [(STATUS_ID, _body(b"m", 5))] + [(PROGRESS_ID, _body(b"m", i % 7)) for i in range(256)]
        kept = [0, 256]
    want, host_frames = _same(frames(events))
    assert want.indices == kept and host_frames == 0


def test_the_topic_and_the_status_are_part_of_the_key():
    events = [(t, _body(b"m", s)) for s in (1, 2, 3, 1, 2, 3) for t in (STATUS_ID, PROGRESS_ID)]
    data = frames(events)
    want, _ = _same(data)
    assert want.indices == [10, 11] and want.keys == [(STATUS_ID, "m"), (PROGRESS_ID, "m")]
    want, _ = _same(data, Policy(progress="per-status"))
    assert want.indices == [7, 9, 10, 11]
    assert want.keys == [(PROGRESS_ID, "m", 1), (PROGRESS_ID, "m", 2), (STATUS_ID, "m"), (PROGRESS_ID, "m", 3)]
    odd = frames([(PROGRESS_ID, _body(b"m", s)) for s in (64, -1, 64, -1, 0)])
    assert _same(odd, Policy(progress="per-status"))[0].indices == [2, 3, 4]


@pytest.mark.parametrize("policy", [Policy(), Policy(progress="per-status")], ids=policy_id)
@pytest.mark.parametrize("hash_mask", [0x3, 0])
def test_forced_collisions_stay_exact(hash_mask, policy):
    """hash_mask 0x3 homes all 240 keys in four slots (0: in one), so every probe chain collides and
    wraps; a -y id differs from its -x in the last byte only. Each keeps its own last frame per topic."""
    pairs = collision_pairs()
    rng = random.Random(1)
    events = [(topic, _body(mid, rng.randrange(6))) for pair in pairs for mid in pair
              for topic in (STATUS_ID, PROGRESS_ID) for _ in range(3)]
    rng.shuffle(events)
    want, host_frames = _same(frames(events), policy, hash_mask=hash_mask)
    assert host_frames == 0 and want.frames == 720
    last = {}
    for i, (topic, body) in enumerate(events):
        last[(topic, body[2:12])] = i
    if policy == Policy():
        assert want.indices == sorted(last.values()) and len(last) == 240
        assert {k[1] for k in want.keys} == {mid.decode() for pair in pairs for mid in pair}
    else:
        assert len(want.indices) > 240


def test_probing_wraps_at_the_end_of_the_table():
    """64 ids chosen so that, under the mask slots - 1, each status key's home is among the last eight
    of the table's 256 slots: 64 keys do not fit into eight slots, so chains run off the end and go on
    from slot 0."""
    slots = gpu_fold.table_slots(128)
    assert slots == 256
    ids, k = [], 0
    while len(ids) < 64:
        mid = b"w%d" % k
        k += 1
        if gc.key_hash(mid, STATUS_ID) & (slots - 1) >= slots - 8:
            ids.append(mid)
    homes = {gc.key_hash(mid, STATUS_ID) & (slots - 1) for mid in ids}
    assert len(ids) > 8 >= len(homes) and min(homes) >= slots - 8  # more keys than slots up to the end: a chain wraps
    rng = random.Random(2)
    events = [(STATUS_ID, _body(mid, rng.randrange(6))) for mid in ids for _ in range(2)]
    rng.shuffle(events)
    want, host_frames = _same(frames(events), hash_mask=slots - 1)
    assert host_frames == 0 and want.frames == 128 and len(want.indices) == 64
    assert {key[1] for key in want.keys} == {mid.decode() for mid in ids}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_fold_corpus(policy, dialect):
    want, host_frames = _same(_corpus(), policy, dialect)
    assert want.frames > 5000
    same_rule = _extract_host_frames(dialect)
    assert 0 < same_rule <= 0.05 * want.frames
    if policy == Policy():
        assert host_frames == same_rule
    else:
        assert host_frames <= same_rule


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_small_mixed_stream(policy):
    for dialect in ops.DIALECTS:
        _same(mixed_stream(), policy, dialect)


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
    for policy in (Policy(), Policy(progress="per-status"), Policy(undecoded="drop")):
        want, host_frames = _same(data, policy, dialect)
        assert host_frames == host
    two = frames([(t, _body(mid, s)) for s, mid in enumerate((b"\xff", b"\xfe", b"\xff", b"\xfe"))
                  for t in (STATUS_ID, PROGRESS_ID)])
    want, host_frames = _same(two, Policy(), dialect)
    assert host_frames == 8
    if dialect == "protobufjs":  # one media, U+FFFD: one kept frame per topic
        assert want.indices == [6, 7] and want.keys == [(STATUS_ID, FFFD), (PROGRESS_ID, FFFD)]
    else:  # upb raises on invalid UTF-8: eight errors
        assert want.indices == list(range(8)) and want.keys == [None] * 8


def _progress(mid: bytes, status: int, host: bytes) -> bytes:
    return _body(mid, status) + b"\x22" + bytes([len(host)]) + host


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("order", list(itertools.permutations(range(3))), ids=lambda o: "".join(map(str, o)))
def test_a_key_shared_between_the_host_and_the_device(order, dialect):
    """Three progress frames of media ``m`` with hosts ``a``, ``é`` and ``b``. Under upb the second is
    decided on the host (a valid non-ASCII host) and shares its key with the other two, which the
    device decides: exactly the last is kept, whichever side decided it."""
    hosts = [b"a", "é".encode(), b"b"]
    events = [(PROGRESS_ID, _progress(b"m", k, hosts[k])) for k in order]
    for policy in (Policy(), Policy(status="all")):
        want, host_frames = _same(frames(events), policy, dialect)
        assert want.indices == [2] and want.keys == [(PROGRESS_ID, "m")]
        assert host_frames == (1 if dialect == "upb" else 0)
    # more of the same around it: other media and the other topic do not take part
    around = [(STATUS_ID, _body(b"m", 1)), (PROGRESS_ID, _progress(b"n", 1, "é".encode()))] + events + \
        [(PROGRESS_ID, _progress(b"n", 2, b"a")), (STATUS_ID, _body(b"n", 1))]
    want, _ = _same(frames(around), Policy(), dialect)
    assert want.indices == [0, 4, 5, 6]
    want, _ = _same(frames(around), Policy(progress="per-status"), dialect)
    assert want.indices == [0, 1, 2, 3, 4, 5, 6]


def test_the_coalesce_is_deterministic():
    first = coalesce_gpu(_corpus(), Policy(), DEVICE)
    assert first == coalesce_gpu(_corpus(), Policy(), DEVICE) == coalesce_cpu(_corpus())


def test_larger_batch():
    data = Workload(n_media=256, seed=9).framed(200_000)
    want, host_frames = _same(data)
    assert want.frames == 200_000 and 256 < len(want.keys) <= 512 and None not in want.keys and host_frames == 0


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_coalesce_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device and merged on the host: keys cross chunk borders,
    and so do host-decided ones."""
    import io

    from beholder_amd import coalesce as co
    data = _corpus()
    want = coalesce_cpu(data, Policy(), dialect)
    out, indices = io.BytesIO(), io.StringIO()
    counts = co.coalesce_file(io.BytesIO(data), out, Policy(), device=DEVICE, dialect=dialect, chunk_bytes=30_000,
                              indices_out=indices)
    assert out.getvalue() == want.data and [int(line) for line in indices.getvalue().split()] == want.indices
    assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                      "keys": sum(k is not None for k in want.keys), "host_frames": _extract_host_frames(dialect)}
    assert len(data) > 7 * 30_000


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = frames([(STATUS_ID, _body(b"m", 1))] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gc.allocate(buf, offs_dev, n)
    params = gc.coalesce_params(Policy(), tables.slots)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gc.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gc.allocate(buf.to(torch.int8), offs_dev, n)
    with pytest.raises(ValueError):
        gc.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gc.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gc.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        gc.launch(tables, params, dialect="proto2")
    with pytest.raises(ValueError):
        gc.launch(tables, gc.coalesce_params(Policy(), 2 * tables.slots))  # params of another table
    with pytest.raises(ValueError):
        gc.launch(tables, params, stages=8)
    with pytest.raises(ValueError):
        gc.coalesce_params(Policy(), 6)
    with pytest.raises(ValueError):
        gc.coalesce_params(Policy(), 4, hash_mask=1 << 64)
    with pytest.raises(ValueError):
        coalesce_gpu(data, Policy(), DEVICE, hash_mask=-1)
    with pytest.raises(TypeError):
        coalesce_gpu(data, "last", DEVICE)
    with pytest.raises(ValueError):
        coalesce_gpu(data, Policy(), DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        coalesce_gpu(data, Policy(), "cpu")
    with pytest.raises(ValueError):
        coalesce_gpu(data[:-1], Policy(), DEVICE)  # broken framing never reaches the device
