"""The stream fold on the GPU (ops/hip/telemetry_fold.hip, ops/gpu_fold.py) against its definition,
``replay.fold_cpu``: every comparison is full ``Summary`` equality, integers and strings, exact."""
from __future__ import annotations

import functools
import random

import pytest

from beholder_amd import ops, replay
from beholder_amd.bench.generator import Workload
from beholder_amd.models import proto
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_fold, hip_lib  # noqa: E402
from telemetry_corpus import body as _body, fold_corpus as _corpus  # noqa: E402

pytestmark = pytest.mark.gpu

PROGRESS = ops.codec_for(proto.load("api.TelemetryProgress"))
STATUS = ops.codec_for(proto.load("api.TelemetryStatus"))
DEVICE = "cuda:0"


@functools.lru_cache(maxsize=None)
def _corpus_cpu(dialect: str) -> replay.Summary:
    return replay.fold_cpu(_corpus(), dialect)


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    assert replay.fold_gpu(b"", DEVICE) == replay.Summary() == replay.fold_cpu(b"")


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (_body(b"m-1", 3), b"", b"\x2e"):
        data = frames([(topic, body)])
        assert replay.fold_gpu(data, DEVICE) == replay.fold_cpu(data), (topic, body)


@pytest.mark.parametrize("status_at", [256, 0])
def test_one_hot_media_across_a_block_boundary(status_at):
    """257 frames, one block and one lane, all for one media: the last status frame wins by its
    index, at the far end (index 256) and at the near end (index 0), whatever order lanes arrive in."""
    rng = random.Random(status_at)
    events = []
    for i in range(257):
        if i == status_at:
            events.append((STATUS_ID, _body(b"hot", 4)))
        elif i < status_at and i % 3 == 0:
            events.append((STATUS_ID, _body(b"hot", rng.randrange(4))))
        else:
            events.append((PROGRESS_ID, PROGRESS.encode({"mediaId": "hot", "status": i % 7, "progress": i % 101})))
    data = frames(events)
    want = replay.fold_cpu(data)
    assert want.media["hot"].last_status_index == status_at and want.media["hot"].last_status == 4
    assert want.media["hot"].status_events == (87 if status_at else 1)  # indices 0, 3, ..., 255 and 256
    assert replay.fold_gpu(data, DEVICE) == want


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_mixed_corpus(dialect):
    want = _corpus_cpu(dialect)
    assert want.status_decode_errors and want.progress_decode_errors
    assert want.progress_unknown_status and want.other_topic == 15
    assert want.frames > 5000 and len(want.media) > 64
    got = replay.fold_gpu(_corpus(), DEVICE, dialect)
    assert got == want


def test_the_fold_is_deterministic():
    first = replay.fold_gpu(_corpus(), DEVICE)
    assert first == replay.fold_gpu(_corpus(), DEVICE) == _corpus_cpu("protobufjs")


def _collision_ids(extra: int) -> list:
    ids = [b"", b"a", b"ab", b"a\0", b"b", b"a\0\0", b"\0", b"\0\0"]
    for k in range(60):  # pairs of one length that differ only in the last byte
        ids += [b"pair-%03d-x" % k, b"pair-%03d-y" % k]
    ids += [b"id-%d" % k for k in range(extra - len(ids))]
    assert len(set(ids)) == len(ids) == extra
    return ids


def _two_frames_each(ids, rng: random.Random) -> bytes:
    events = [(STATUS_ID, _body(mid, rng.randrange(6))) for mid in ids]
    events += [(PROGRESS_ID, _body(mid, rng.randrange(8))) for mid in ids]
    rng.shuffle(events)
    return frames(events)


def test_forced_collisions_stay_exact():
    """hash_mask 0x3 homes all 500 ids in four slots: every probe chain collides, and equality is
    decided by the bytes, never by the hash."""
    data = _two_frames_each(_collision_ids(500), random.Random(1))
    want = replay.fold_cpu(data)
    assert len(want.media) == 500
    assert replay.fold_gpu(data, DEVICE, hash_mask=0x3) == want
    assert replay.fold_gpu(data, DEVICE, hash_mask=0) == want


def test_probing_wraps_at_the_end_of_the_table():
    """500 ids chosen so that, under the mask slots - 1, each one's home is among the table's last
    eight slots: all but a few probe chains run off the end and go on from slot 0."""
    slots = gpu_fold.table_slots(1000)
    assert slots == 2048
    ids, k = [], 0
    while len(ids) < 500:
        mid = b"w%d" % k
        k += 1
        if gpu_fold.hash64(mid) & (slots - 1) >= slots - 8:
            ids.append(mid)
    data = _two_frames_each(ids, random.Random(2))
    want = replay.fold_cpu(data)
    assert want.frames == 1000 and len(want.media) == 500
    assert replay.fold_gpu(data, DEVICE, hash_mask=slots - 1) == want


def test_all_distinct_ids_fill_the_table_to_its_designed_load():
    rng = random.Random(3)
    events = [(STATUS_ID if k % 4 == 0 else PROGRESS_ID, _body(b"media-%05d" % k, rng.randrange(6)))
              for k in range(5000)]
    data = frames(events)
    want = replay.fold_cpu(data)
    assert len(want.media) == 5000
    assert replay.fold_gpu(data, DEVICE) == want


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_non_ascii_ids_take_the_host_path(dialect):
    rng = random.Random(4)
    plain = [b"ascii-%d" % k for k in range(20)]
    other = ["é".encode(), "メディア".encode(), b"\xff", b"\xfe", b"ok\x80", b"\xc3", b"caf\xc3\xa9", b"\xf0\x9f\x8e\xac"]
    events, host = [], 0
    for _ in range(600):
        mid = rng.choice(other) if rng.random() < 0.3 else rng.choice(plain)
        host += mid in other
        events.append((rng.choice((STATUS_ID, PROGRESS_ID)), _body(mid, rng.randrange(7))))
    data = frames(events)
    want = replay.fold_cpu(data, dialect)
    if dialect == "protobufjs":
        assert "�" in want.media and want.media["�"].status_events + want.media["�"].progress_events > 20
    else:
        assert want.status_decode_errors and want.progress_decode_errors  # upb rejects invalid UTF-8
    got, host_frames = gpu_fold.fold(data, DEVICE, dialect)
    assert got == want
    assert host_frames == host and 100 < host < 300


def test_larger_batch():
    data = Workload(n_media=256, seed=9).framed(200_000)
    want = replay.fold_cpu(data)
    assert want.frames == 200_000 and len(want.media) == 256
    assert replay.fold_gpu(data, DEVICE) == want


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = frames([(STATUS_ID, _body(b"m", 1))] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gpu_fold.allocate(buf, offs_dev, n)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gpu_fold.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gpu_fold.allocate(buf.to(torch.int8), offs_dev, n)
    with pytest.raises(ValueError):
        gpu_fold.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gpu_fold.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gpu_fold.launch(tables, dialect="proto2")
    with pytest.raises(ValueError):
        replay.fold_gpu(data, DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        replay.fold_gpu(data, "cpu")
    with pytest.raises(ValueError):
        replay.fold_gpu(data[:-1], DEVICE)  # broken framing never reaches the device
