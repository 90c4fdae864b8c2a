"""``transitions`` on the GPU (ops/hip/telemetry_transitions.hip, ops/gpu_transitions.py) against its
definition, ``transitions.transitions_cpu``: every comparison is full ``Transitions`` equality (the
counters, the matrix and every media's row), exact."""
from __future__ import annotations

import functools
import io
import random

import pytest

from beholder_amd import ops
from beholder_amd.bench.generator import Workload
from beholder_amd.models import proto
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transitions import (MediaFlow, Transitions, transitions_cpu, transitions_file, transitions_gpu)
from beholder_amd.transport.framing import iter_frames

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_fold, gpu_transitions as gt, hip_lib  # noqa: E402
from telemetry_corpus import body as _body  # noqa: E402
from transitions_cases import (MANY_EXTRA, boundary_ids, corpus as _corpus, many_media_stream, mixed_stream,  # noqa: E402
                               pairs_stream, shared_media_stream, status_stream)

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
FFFD = "�"


@functools.lru_cache(maxsize=None)
def _want(data: bytes, dialect: str) -> Transitions:
    return transitions_cpu(data, dialect)


def _same(data: bytes, dialect: str = "protobufjs", public: bool = True, **kw) -> tuple:
    """Asserts the device result against the definition; returns ``(Transitions, host_frames)``."""
    want = _want(data, dialect)
    got, host_frames = gt.transitions(data, DEVICE, dialect, **kw)
    assert (got.frames, got.status_events, got.status_decode_errors) == \
        (want.frames, want.status_events, want.status_decode_errors)
    assert got.matrix == want.matrix
    assert got.media == want.media
    assert got == want
    if public:
        assert transitions_gpu(data, DEVICE, dialect, **kw) == want  # the public call
    return want, host_frames


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for dialect in ops.DIALECTS:
        assert transitions_gpu(b"", DEVICE, dialect) == Transitions() == transitions_cpu(b"", dialect)
        assert gt.transitions(b"", DEVICE, dialect) == (Transitions(), 0)
    assert transitions_file(io.BytesIO(b""), DEVICE) == (Transitions(), 0)


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (_body(b"m-1", 3), b"", b"\x2e", _body(b"", 64)):
        for dialect in ops.DIALECTS:
            want, host_frames = _same(frames([(topic, body)]), dialect, public=False)
            assert want.frames == 1 and want.matrix == {} and host_frames == 0
            assert len(want.media) == (topic == STATUS_ID and body != b"\x2e")


def test_two_status_events():
    one, _ = _same(frames([(STATUS_ID, _body(b"m", 0)), (STATUS_ID, _body(b"m", 4))]))
    assert one.matrix == {(0, 4): 1} and one.media == {"m": MediaFlow(2, 1, 0, 0, 4, 1)}
    two, _ = _same(frames([(STATUS_ID, _body(b"m", 0)), (STATUS_ID, _body(b"n", 4))]))
    assert two.matrix == {} and len(two.media) == 2
    apart, _ = _same(frames([(STATUS_ID, _body(b"m", 5)), (PROGRESS_ID, _body(b"m", 1)), (STATUS_ID, _body(b"m", 5))]))
    assert apart.matrix == {(5, 5): 1} and apart.media == {"m": MediaFlow(2, 0, 5, 0, 5, 2)}


def test_65_status_events_of_one_media():
    """A wave boundary inside a media's run."""
    want, host_frames = _same(status_stream([b"m"] * 65, other_every=3))
    assert want.media["m"].status_events == 65 and want.transitions == 64 and host_frames == 0
    _same(status_stream([b"m"] * 65, statuses=1))


@pytest.mark.parametrize("full", [gt.SORT_TILE, gt.SORT_BLOCK], ids=["tile", "block"])
@pytest.mark.parametrize("variant", ["one-media", "two-media-alternating", "last-alone-in-its-media"])
def test_one_frame_past_a_boundary(variant, full):
    """``full`` status events fill a tile of the sort (the running sums carry into the block's next
    tile), or the whole block; the next unit holds a single one. With two media the sort runs one
    pass; the pairs kernel reads the last event of the full unit from the unit after it."""
    ids = boundary_ids(full, variant)
    want, host_frames = _same(status_stream(ids))
    assert host_frames == 0 and want.status_events == full + 1 and len(want.media) == len(set(ids))
    assert want.transitions == full + 1 - len(set(ids))
    _same(status_stream(ids, other_every=5), public=False)  # the events are not the frames
    _same(status_stream(ids + ids[:3]), public=False)       # and a few more in the next unit


@pytest.mark.parametrize("media", [1, 2, 256, 257, 65_537])
def test_pass_counts(media):
    """Zero passes for one media, one up to 256, two from 257, three from 65,537."""
    assert gt.sort_passes(media) == {1: 0, 2: 1, 256: 1, 257: 2, 65_537: 3}[media]
    data, a, b = many_media_stream(media)
    want, host_frames = _same(data, public=False)
    assert want.frames == want.status_events == media + MANY_EXTRA and len(want.media) == media and host_frames == 0
    if media > 1:
        assert want.media[a.decode()].status_events >= 7 and want.media[b.decode()].status_events >= 7
    assert sum(flow.status_events >= 3 for flow in want.media.values()) >= min(media, 4)


def test_sort_passes():
    assert [gt.sort_passes(g) for g in (0, 1, 2, 256, 257, 65_536, 65_537, 2 ** 24, 2 ** 24 + 1, 2 ** 31)] == \
        [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]


def test_more_passes_than_needed_change_nothing():
    """The probe sorts a stream of few media in up to three passes."""
    import torch
    data = pairs_stream()
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    results = []
    for passes in (None, 1, 2, 3, 4):
        t = gt.allocate(buf, offs_dev, n)
        gt.classify(t)
        gt.claim(t)
        gt.rank(t)
        groups, events = gt.counts(t)
        assert (groups, events) == (120, 360)
        s = gt.sort(gt.compact(t, groups, events), passes)
        assert bool((s.keys[1:] >= s.keys[:-1]).all())
        gt.pairs(s, gpu_fold.known_mask({k: "" for k in range(6)}))
        torch.cuda.synchronize()
        results.append(gt.finish(data, offs, n, gt.collect(t, s), s))
    assert all(r == _want(data, "protobufjs") for r in results)


def test_every_key_in_one_probe_chain():
    for dialect in ops.DIALECTS:
        _same(mixed_stream(), dialect, hash_mask=0)
    want, _ = _same(pairs_stream(), hash_mask=0)
    assert len(want.media) == 120 and want.status_events == 360
    _same(pairs_stream(), hash_mask=0xFF, public=False)


def test_probing_wraps_at_the_end_of_the_table():
    """64 ids chosen so that, under the mask slots - 1, each one's home is among the last eight of the
    table's 256 slots: 64 media do not fit into eight slots, so chains run off the end and go on from
    slot 0."""
    slots = gpu_fold.table_slots(128)
    assert slots == 256
    ids, k = [], 0
    while len(ids) < 64:
        mid = b"w%d" % k
        k += 1
        if gpu_fold.hash64(mid) & (slots - 1) >= slots - 8:
            ids.append(mid)
    homes = {gpu_fold.hash64(mid) & (slots - 1) for mid in ids}
    assert len(ids) > 8 >= len(homes) and min(homes) >= slots - 8  # more media than slots up to the end: a chain wraps
    rng = random.Random(2)
    events = [(STATUS_ID, _body(mid, rng.randrange(6))) for mid in ids for _ in range(2)]
    rng.shuffle(events)
    want, host_frames = _same(frames(events), hash_mask=slots - 1)
    assert host_frames == 0 and want.frames == want.status_events == 128
    assert set(want.media) == {mid.decode() for mid in ids}
    assert all(flow.status_events == 2 for flow in want.media.values())


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_fold_corpus(dialect):
    want, host_frames = _same(_corpus(), dialect)
    assert want.frames > 5000 and 0 < host_frames <= 0.05 * want.frames
    if dialect == "protobufjs":
        decode = ops.codec_for(proto.load("api.TelemetryStatus"), dialect).decode

        def high(body):
            try:
                return not decode(body).mediaId.isascii()
            except proto.DecodeError:
                return False
        assert host_frames == sum(topic == STATUS_ID and high(body) for topic, body in iter_frames(_corpus()))


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_small_mixed_stream(dialect):
    _same(mixed_stream(), dialect)


def test_a_media_shared_between_host_and_device():
    data = shared_media_stream()
    want, host_frames = _same(data, "upb")
    assert host_frames == 12 and {m: f.status_events for m, f in want.media.items()} == {"m": 12, "shared-2": 12, "plain": 9}
    same, none = _same(data, "protobufjs")
    assert none == 0 and same == want
    _same(data, "upb", hash_mask=0, public=False)
    # the host's frames first and last in the shared media, and a media that only the host holds
    group = b"\x2b\x2c"
    events = [(STATUS_ID, _body(b"m", 1) + group), (STATUS_ID, _body(b"m", 2)), (STATUS_ID, _body(b"host-only", 3) + group),
              (STATUS_ID, _body(b"m", 2)), (STATUS_ID, _body(b"host-only", 4) + group), (STATUS_ID, _body(b"m", 6) + group)]
    want, host_frames = _same(frames(events), "upb")
    assert host_frames == 4 and want.media["m"] == MediaFlow(4, 2, 1, 0, 6, 5)
    assert _same(frames(events[::2]), "upb")[1] == 3  # the device holds no event at all


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_non_ascii_ids_take_the_host_path(dialect):
    rng = random.Random(4)
    plain = [b"ascii-%d" % k for k in range(20)]
    other = ["é".encode(), "メディア".encode(), b"\xff", b"\xfe", b"ok\x80", b"\xc3", b"caf\xc3\xa9",
             b"\xf0\x9f\x8e\xac"]
    events, host = [], 0
    for _ in range(600):
        mid = rng.choice(other) if rng.random() < 0.3 else rng.choice(plain)
        topic = rng.choice((STATUS_ID, PROGRESS_ID))
        host += mid in other and topic == STATUS_ID
        events.append((topic, _body(mid, rng.randrange(7))))
    want, host_frames = _same(frames(events), dialect)
    assert 50 < host < 150 and host_frames == host
    two = frames([(STATUS_ID, _body(mid, s)) for s, mid in enumerate((b"\xff", b"\xfe", b"\xff", b"\xfe"))])
    want, host_frames = _same(two, dialect)
    assert host_frames == 4
    if dialect == "protobufjs":  # one media, U+FFFD
        assert want.media == {FFFD: MediaFlow(4, 3, 0, 0, 3, 3)}
    else:  # upb raises on invalid UTF-8: four errors
        assert want.status_decode_errors == 4 and not want.media


def test_transitions_are_deterministic():
    first = transitions_gpu(_corpus(), DEVICE)
    assert first == transitions_gpu(_corpus(), DEVICE) == _want(_corpus(), "protobufjs")


def test_larger_batch():
    data = Workload(n_media=256, seed=9).framed(200_000)
    want, host_frames = _same(data, public=False)
    assert want.frames == 200_000 and len(want.media) == 256 and host_frames == 0
    assert want.status_events > 10_000


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_transitions_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device; a media's history crosses the cuts."""
    data = _corpus()
    assert len(data) > 7 * 30_000
    got, host_frames = transitions_file(io.BytesIO(data), DEVICE, dialect, chunk_bytes=30_000)
    assert got == _want(data, dialect)
    assert host_frames == gt.transitions(data, DEVICE, dialect)[1] > 0


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = frames([(STATUS_ID, _body(b"m", 1))] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gt.allocate(buf, offs_dev, n)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gt.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gt.allocate(buf.to(torch.int8), offs_dev, n)
    with pytest.raises(ValueError):
        gt.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gt.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gt.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        gt.classify(tables, dialect="proto2")
    for bad in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError):
            gt.claim(tables, hash_mask=bad)
        with pytest.raises(ValueError):
            gt.transitions(data, DEVICE, hash_mask=bad)
    with pytest.raises(ValueError):
        gt.compact(tables, 0, 0)  # no event: nothing to sort
    with pytest.raises(ValueError):
        gt.compact(tables, 3, 2)  # more media than events
    with pytest.raises(ValueError):
        gt.sort_pass(tables.rows, tables.rows, 2, 4, tables.rows, tables.rows, tables.rows, tables.rows)  # shift
    with pytest.raises(ValueError):
        gt.sort_pass(tables.rows, tables.rows, 2, 8, tables.rows, tables.rows, tables.rows, tables.rows, stages=8)
    with pytest.raises(ValueError):
        transitions_gpu(data, DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        transitions_gpu(data, "cpu")
    with pytest.raises(ValueError):
        transitions_gpu(data[:-1], DEVICE)  # broken framing never reaches the device
    with pytest.raises(ValueError):
        transitions_file(io.BytesIO(data), DEVICE, dialect="proto2")
