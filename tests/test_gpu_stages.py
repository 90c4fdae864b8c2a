"""``stages`` on the GPU (ops/hip/telemetry_stages.hip, ops/gpu_stages.py) against its definition,
``stages.stages_cpu``: every comparison is full ``StageReport`` equality (the counters, the three
tables, every media's row), exact, in both dialects unless noted."""
from __future__ import annotations

import functools
import io
import random

import pytest

from beholder_amd import ops, replay
from beholder_amd.ops import frames
from beholder_amd.stages import MediaStand, StageReport, stages_cpu, stages_file, stages_gpu
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_fold, gpu_stages as gs, gpu_transitions as gt, hip_lib  # noqa: E402
from extract_cases import collision_pairs  # noqa: E402
from stages_cases import (P, S, bucket_edges, corpus as _corpus, joined_stream, non_ascii_stream, one_media,  # noqa: E402
                          placed_stream, random_stream, stitch_stream)
from telemetry_corpus import body as _body  # noqa: E402
from thin_cases import UNKNOWN_STATUSES, boundary_ids, mixed_stream, progress_body  # noqa: E402
from transitions_cases import GROUP_TAIL  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
BLOCK = gs.CARRY_BLOCK


@functools.lru_cache(maxsize=None)
def _want(data: bytes, dialect: str) -> StageReport:
    return stages_cpu(data, dialect)


def _same(data: bytes, dialect: str = "protobufjs", public: bool = False, **kw) -> tuple:
    """Asserts the device result against the definition; returns ``(StageReport, host_frames)``."""
    want = _want(data, dialect)
    got, host_frames = gs.stages(data, DEVICE, dialect, **kw)
    assert (got.frames, got.status_events, got.progress_events, got.status_decode_errors, got.progress_decode_errors) \
        == (want.frames, want.status_events, want.progress_events, want.status_decode_errors,
            want.progress_decode_errors)
    assert got.entered == want.entered
    assert got.matrix == want.matrix
    assert got.closed == want.closed
    assert got.media == want.media
    assert got == want
    if public:
        assert stages_gpu(data, DEVICE, dialect, **kw) == want  # the public call
    return want, host_frames


def _both(data: bytes, **kw) -> StageReport:
    """Both dialects; returns the protobufjs report."""
    _same(data, "upb", **kw)
    return _same(data, "protobufjs", **kw)[0]


def _carried(data: bytes):
    """The stages up to the carry by hand: ``(keys, is_status, stand, head)`` per sorted position."""
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tb = gs.allocate(buf, offs_dev, n)
    gs.classify(tb)
    gt.claim(tb.t)
    gt.rank(tb.t)
    s = gt.sort(gt.compact(tb.t, *gt.counts(tb.t)))
    k = gs.prepare(tb, s)
    gs.carry(tb, s, k)
    return (s.keys.cpu().numpy(), (k.saux.cpu().numpy() & gs.AUX_STATUS) != 0, k.stand.cpu().numpy(),
            k.head.cpu().numpy())


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for dialect in ops.DIALECTS:
        assert stages_gpu(b"", DEVICE, dialect) == StageReport() == stages_cpu(b"", dialect)
        assert gs.stages(b"", DEVICE, dialect) == (StageReport(), 0)
    assert stages_file(io.BytesIO(b""), DEVICE) == (StageReport(), 0)


def test_a_stream_with_no_device_event_stops_after_the_counts(monkeypatch):
    def no_launch(*a, **kw):
        raise AssertionError("nothing to sort, to carry or to settle")
    for module, name in ((gt, "compact"), (gt, "sort"), (gs, "prepare"), (gs, "carry"), (gs, "settle"), (gs, "leads")):
        monkeypatch.setattr(module, name, no_launch)
    data = frames([(STATUS_ID, b"\x2e"), (PROGRESS_ID, b"\x2e"), (9, progress_body(b"m", 2, 5, b"a"))] * 3)
    want = _both(data)
    assert (want.frames, want.status_decode_errors, want.progress_decode_errors, want.media) == (9, 3, 3, {})
    # and where the CPU holds the only events
    data = joined_stream([(S, "é".encode(), 2), (P, "é".encode(), 2, 5), (P, "ü".encode(), 2, 4)] * 2)
    want, host_frames = _same(data)
    assert host_frames == 6 and want.status_events == 2 and want.lead_events == 2
    # upb: every frame has a group, so the device holds no event at all
    data = frames([(STATUS_ID, _body(b"m", 1) + GROUP_TAIL), (PROGRESS_ID, progress_body(b"m", 1, 5) + GROUP_TAIL)] * 2)
    want, host_frames = _same(data, "upb")
    assert host_frames == 4 and want.media == {"m": MediaStand({}, None, 4, (2, 1, 1, 5))}


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (progress_body(b"m-1", 3, 40, b"node-a"), _body(b"m-1", 3), b"", b"\x2e", progress_body(b"", 64, -1, b"")):
        for dialect in ops.DIALECTS:
            want, host_frames = _same(frames([(topic, body)]), dialect)
            assert want.frames == 1 and host_frames == 0
            assert want.status_events + want.progress_events == (topic != 9 and body != b"\x2e")


def test_the_hand_cases():
    r = _both(joined_stream([(S, b"m", 2), (P, b"m", 2, 10), (P, b"m", 3, 40)]), public=True)
    assert r.media == {"m": MediaStand({}, None, 3, (0, 2, 2, 40))} and r.matrix == {(2, 2): 1, (2, 3): 1}
    r = _both(joined_stream([(P, b"m", 2, 10), (P, b"m", 6, 20), (P, b"m", 2, 30), (S, b"m", 3)]))
    assert r.lead_events == 3 and r.media["m"].open == (3, 3, 0, None)
    # a lead only, status events only, and both
    r = _both(joined_stream([(P, b"p", 2, 100), (S, b"s", 4), (P, b"b", 1, -3), (P, b"p", 2, 7), (S, b"s", 4), (S, b"b", 1),
                             (P, b"b", 1, 100)]))
    assert r.media == {"p": MediaStand({2: 2}, 7, 2, None), "s": MediaStand({}, None, 2, (4, 4, 0, None)),
                       "b": MediaStand({1: 1}, -3, 3, (5, 1, 1, 100))}
    r = _both(joined_stream([(S, b"m", 0), (P, b"m", 0, 100), (S, b"m", 5), (P, b"m", 0, 15), (P, b"m", 5, 15), (S, b"m", 0),
                             (P, b"n", 0, 1), (P, b"m", 0, 0)]))
    assert r.closed == {(0, "full"): 1, (5, "1"): 1} and r.open == {(0, "0"): 1} and r.disagree == 1


def test_65_events_of_one_media():
    """A wave edge inside the carry: the status event first, and the status event as the wave's last lane."""
    want = _both(joined_stream(one_media({0}, 65)))
    assert want.media["m"].open == (0, 2, 64, 64) and want.lead_events == 0
    want = _both(joined_stream(one_media({63}, 65)))
    assert want.media["m"].open == (63, 2, 1, 64) and want.lead_events == 63
    _both(joined_stream(one_media({0, 64}, 130)))


def test_the_status_event_at_the_end_of_a_scan_block():
    """Position BLOCK - 1 holds the status event and the next block its progress events; then the same
    with the status event as the next block's first position."""
    for at in (BLOCK - 1, BLOCK):
        data = joined_stream(one_media({at}, BLOCK + 40))
        want = _both(data)
        assert want.lead_events == at and want.media["m"].open[:3] == (at, 2 + at % 3, BLOCK + 39 - at)
        keys, is_status, stand, head = _carried(data)
        assert list(np.nonzero(is_status)[0]) == [at] and (head == 0).all()
        assert (stand[:at] == -1).all() and (stand[at:] == at).all()


def test_a_value_carried_through_a_whole_block():
    """One status event, then 2 * BLOCK + 1 progress events: the middle block holds no status event."""
    data = joined_stream(one_media({0}, 2 * BLOCK + 2))
    want = _both(data)
    assert want.media["m"].open == (0, 2, 2 * BLOCK + 1, (2 * BLOCK + 1) % 101) and want.agree == 2 * BLOCK + 1
    stand = _carried(data)[2]
    assert (stand == 0).all()
    # and a status event in every block but the middle one
    _both(joined_stream(one_media({3, 2 * BLOCK + 5}, 3 * BLOCK)))


def test_the_second_step_of_the_totals_scan():
    """BLOCK * BLOCK + 1 events behind one status event: the totals scan carries into its second tile."""
    count = BLOCK * BLOCK + 2
    data = joined_stream(one_media({0}, count))
    want = _same(data)[0]
    assert want.media["m"].open == (0, 2, count - 1, (count - 1) % 101) and want.frames == count
    # a status event in the last block only: everything before it is lead
    data = joined_stream(one_media({count - 3}, count))
    want = _same(data, "upb")[0]
    assert want.lead_events == count - 3 and want.media["m"].open == (count - 3, 2 + (count - 3) % 3, 2, (count - 1) % 101)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_a_lead_run_at_a_block_edge_does_not_inherit_the_neighbour(delta):
    """A media with no status event whose run starts at a block's first position, one before it and
    one after it, behind a media that has one. Which media sorts first depends on the ids' slots, so
    both arrangements run, and one of them must have the run where the case wants it."""
    first = BLOCK + delta
    met = False
    for with_status, lead_only in ((b"a", b"b"), (b"b", b"a")):
        data = joined_stream([(S, with_status, 3)] + [(P, with_status, 3, k % 101) for k in range(first - 1)]
                             + [(P, lead_only, 2, k % 101) for k in range(70)])
        want = _both(data)
        assert want.media[lead_only.decode()] == MediaStand({2: 70}, 69, 70, None)
        assert want.media[with_status.decode()].open == (0, 3, first - 1, (first - 2) % 101)
        assert want.matrix == {(3, 3): first - 1} and want.lead_events == 70
        keys, is_status, stand, head = _carried(data)
        if is_status[0]:  # the media with the status event sorts first
            met = True
            assert (head[first:] == first).all() and (stand[first:] == 0).all()  # carried over, and not valid
    assert met


@pytest.mark.parametrize("full", [gt.SORT_TILE, gt.SORT_BLOCK], ids=["tile", "block"])
@pytest.mark.parametrize("media", [1, 2])
def test_one_event_past_a_boundary(media, full):
    """``full`` events fill a tile of the sort and the settle, or their whole block; the next unit
    holds a single one, a status event that closes a stage across the edge."""
    ids = boundary_ids(full + 1, media)
    events = [(S, mid, 2) if k < media or k == full else (P, mid, 2, k % 101) for k, mid in enumerate(ids)]
    want = _both(joined_stream(events))
    assert sum(want.closed.values()) == 1 and want.status_events == media + 1
    assert want.media[ids[-1].decode()].open == (full, 2, 0, None)
    # and a progress event across the edge
    events[-1] = (P, ids[-1], 3, 100)
    want = _both(joined_stream(events))
    assert want.closed == {} and want.disagree == 1 and want.media[ids[-1].decode()].open[3] == 100


@pytest.mark.parametrize("media", [2, 257])
def test_pass_counts(media):
    """One sort pass for two media, two for 257."""
    assert gt.sort_passes(media) == {2: 1, 257: 2}[media]
    rng = random.Random(media)
    ids = [b"media-%04d" % k for k in range(media)] * 8
    rng.shuffle(ids)
    events = [(S, mid, rng.randrange(6)) if rng.random() < 0.3 else (P, mid, rng.randrange(6), rng.choice((0, 50, 100)))
              for mid in ids]
    want = _both(joined_stream(events))
    assert len(want.media) == media and want.lead_events > 0 and want.closed and want.disagree > media


def test_every_bucket_edge_and_the_unknown_classes():
    want = _both(bucket_edges(), public=True)
    assert {b for _, b in want.closed} == {"none", "below", "0", "1", "9", "full", "over"}
    assert "unknown" in {a for a, _ in want.closed} and ("unknown", "unknown") in want.matrix
    for seed in (1, 2, 3):
        _both(random_stream(seed))
    _both(mixed_stream())


def test_every_block_of_the_settle_receives_every_class():
    """More than two blocks of the settle, over 40 media whose events of both topics walk through
    every class, the unknown one included."""
    count = 2 * gt.SORT_BLOCK + 100
    statuses = (0, 1, 2, 3, 4, 5) + UNKNOWN_STATUSES[:1]
    events = []
    for k in range(count):
        mid, status = b"m-%02d" % (k % 40), statuses[(k // 3) % 7]
        events.append((S, mid, status) if (k // 40) % 5 == 0 else (P, mid, statuses[(k // 11) % 7], (13 * k) % 120 - 10))
    want = _both(joined_stream(events))
    assert len(want.entered) == 7 and len(want.matrix) == 49 and len({a for a, _ in want.closed}) == 7


def test_everything_in_one_probe_chain():
    for mask in (0, 0xFF):
        _both(random_stream(1), hash_mask=mask)
        _both(mixed_stream(), hash_mask=mask)
        _both(bucket_edges(), hash_mask=mask)


def test_ids_that_differ_in_the_last_byte_only():
    rng = random.Random(1)
    names = [name for pair in collision_pairs() for name in pair]
    ids = names * 4
    rng.shuffle(ids)
    events = [(S, mid, rng.randrange(4)) if rng.random() < 0.3 else (P, mid, rng.randrange(4), rng.choice((0, 5, 100)))
              for mid in ids]
    for mask in (None, 0):
        want = _both(joined_stream(events), hash_mask=mask)
        assert len(want.media) == len(names)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_non_ascii_ids_are_decided_on_the_cpu(dialect):
    want, host_frames = _same(non_ascii_stream(), dialect)
    assert host_frames > 150 and want.status_events > 20 and want.lead_events > 0
    two = joined_stream([(S, b"\xff", 2), (P, b"\xfe", 2, 6), (P, b"\xff", 3, 7), (S, b"\xfe", 1)])
    want, host_frames = _same(two, dialect)
    assert host_frames == 4
    # protobufjs: one media, U+FFFD; upb raises on invalid UTF-8: no event
    assert (want.status_events, want.progress_events, len(want.media)) == ((2, 2, 1) if dialect == "protobufjs" else (0, 0, 0))


def test_a_media_shared_between_cpu_and_device():
    """upb leaves the frames with a group to the CPU: most events of the shared media have their
    neighbour on the other side, and in ``m`` every status event that a device progress event stands
    on is the CPU's, so the CPU must take the device's contributions out and decide the whole run."""
    data = stitch_stream()
    want, host_frames = _same(data, "upb", public=True)
    assert host_frames == 12 + 8 + 8 and want.status_events > 10 and want.disagree > 0 and want.closed
    same, none = _same(data, "protobufjs")
    assert none == 0 and same == want
    _same(data, "upb", hash_mask=0)
    for where in ("first", "middle", "last"):
        data = placed_stream(where)
        want, host_frames = _same(data, "upb", public=True)
        assert host_frames == 4 + 1 and set(want.media) == {"m", "dev-only", "cpu-only"}
        assert _same(data, "protobufjs") == (want, 0)
    # the CPU's frame is the status event that the device's progress events stand on, and the other way round
    group = GROUP_TAIL
    events = [(STATUS_ID, _body(b"m", 2) + group), (PROGRESS_ID, progress_body(b"m", 2, 9)),
              (PROGRESS_ID, progress_body(b"m", 3, 100)), (STATUS_ID, _body(b"m", 3)),
              (PROGRESS_ID, progress_body(b"m", 3, 5) + group), (PROGRESS_ID, progress_body(b"cpu-only", 3, 4) + group)]
    want, host_frames = _same(frames(events), "upb")
    assert host_frames == 3 and want.lead_events == 1 and want.closed == {(2, "full"): 1}
    assert want.media["m"] == MediaStand({}, None, 5, (3, 3, 1, 5))


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_fold_corpus(dialect):
    want, host_frames = _same(_corpus(), dialect, public=True)
    assert want.frames == 5711 and 0 < host_frames <= 0.05 * want.frames
    assert want.lead_events and want.disagree and want.closed and want.open
    _same(_corpus(), dialect, hash_mask=0xFFF)


def test_two_runs_are_equal():
    first = stages_gpu(_corpus(), DEVICE)
    second = stages_gpu(_corpus(), DEVICE)
    assert first == second == _want(_corpus(), "protobufjs")
    assert first.to_json(True) == second.to_json(True)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_stages_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device; media and stages cross the cuts."""
    data = _corpus()
    assert len(data) > 7 * 30_000
    want = _want(data, dialect)
    whole_host_frames = gs.stages(data, DEVICE, dialect)[1]
    for chunk_bytes in (30_000, 1 << 30):
        got, host_frames = stages_file(io.BytesIO(data), DEVICE, dialect, chunk_bytes=chunk_bytes)
        assert got == want and host_frames == whole_host_frames > 0
    assert stages_file(io.BytesIO(data), "gpu", dialect, chunk_bytes=100_000)[0] == want


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = joined_stream([(S, b"m", 1), (P, b"m", 1, 5)])
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gs.allocate(buf, offs_dev, n)
    gs.classify(tables)
    gt.claim(tables.t)
    gt.rank(tables.t)
    assert gt.counts(tables.t) == (1, 2)
    s = gt.sort(gt.compact(tables.t, 1, 2))
    k = gs.prepare(tables, s)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gs.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gs.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gs.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gs.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        gs.classify(tables, dialect="proto2")
    with pytest.raises(ValueError):
        gs.prepare(tables, s._replace(groups=3))  # more media than events
    with pytest.raises(ValueError):
        gs.prepare(tables, s._replace(events=n + 1))  # more events than frames
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError):
            gs.stages(data, DEVICE, hash_mask=bad)
        with pytest.raises(ValueError):
            gs.settle(s, k, bad)
    with pytest.raises(ValueError):
        stages_gpu(data, DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        stages_gpu(data, "cpu")
    with pytest.raises(ValueError):
        stages_gpu(data[:-1], DEVICE)  # broken framing never reaches the device
    with pytest.raises(ValueError):
        stages_file(io.BytesIO(data), DEVICE, dialect="proto2")


def test_the_entry_points_refuse_null_pointers_and_impossible_counts():
    """Each returns hipErrorInvalidValue (1) and launches nothing; a count <= 0 returns 0."""
    torch = pytest.importorskip("torch")
    so = hip_lib.lib()
    assert so.bh_stages_classify(None, None, 0, 1, None, None, None, None, None, None) == 0
    assert so.bh_stages_classify(None, None, 4, 1, None, None, None, None, None, None) == 1
    assert so.bh_stages_carry(None, None, -1, 4, None, None, None, None, None, None, None, None) == 0
    assert so.bh_stages_carry(None, None, 4, 4, None, None, None, None, None, None, None, None) == 1
    assert so.bh_stages_settle(None, None, None, None, None, None, 0, 1, 0, None, None, None, None) == 0
    assert so.bh_stages_settle(None, None, None, None, None, None, 4, 1, 0, None, None, None, None) == 1
    data = joined_stream([(S, b"m", 1)] + [(P, b"m", 1, 5)] * 3)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tb = gs.allocate(buf, offs_dev, n)
    assert so.bh_stages_classify(buf.data_ptr(), offs_dev.data_ptr(), n, 2, tb.t.rows.data_ptr(), tb.aux.data_ptr(),
                                 tb.t.is_event.data_ptr(), tb.t.counters.data_ptr(), tb.t.overflow.data_ptr(),
                                 None) == 1  # no such dialect
    gs.classify(tb)
    gt.claim(tb.t)
    gt.rank(tb.t)
    s = gt.sort(gt.compact(tb.t, 1, 4))
    k = gs.prepare(tb, s)
    k.stand.fill_(-7)
    p = [x.data_ptr() for x in (s.keys, s.vals, tb.aux, k.saux, k.totals, k.base, k.stand, k.stood, k.head)]
    assert so.bh_stages_carry(p[0], p[1], 5, 4, *p[2:], None) == 1  # more events than frames
    assert so.bh_stages_carry(p[0], p[1], 4, 4, p[2], None, *p[4:], None) == 1  # a null pointer among the outputs
    q = [x.data_ptr() for x in (s.keys, s.vals, k.saux, k.stand, k.stood, k.head)]
    r = [x.data_ptr() for x in (k.tables, k.media_rows, k.lead_scan.keep_len)]
    assert so.bh_stages_settle(*q, 4, 5, 0, *r, None) == 1  # more media than events
    assert so.bh_stages_settle(*q, 4, 0, 0, *r, None) == 1  # no media
    torch.cuda.synchronize()
    assert int(k.tables.sum()) == 0 and int(k.media_rows.sum()) == 0 and int((k.stand != -7).sum()) == 0  # nothing ran
    assert replay.status_names()  # the enum is there for the mask
