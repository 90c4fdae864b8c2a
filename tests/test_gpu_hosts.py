"""``hosts`` on the GPU (ops/hip/telemetry_hosts.hip, ops/gpu_hosts.py) against its definition,
``hosts.hosts_cpu``: every comparison is full ``HostReport`` equality (the counters, every host's row,
every pair, every media's edge events), exact, in both dialects unless noted."""
from __future__ import annotations

import functools
import io
import random

import pytest

from beholder_amd import ops
from beholder_amd.hosts import HostReport, HostRow, hosts_cpu, hosts_file, hosts_gpu
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_extract, gpu_fold, gpu_hosts as gh, gpu_transitions as gt, hip_lib  # noqa: E402
from extract_cases import collision_pairs  # noqa: E402
from hosts_cases import (ASCII_WORKERS, corpus as _corpus, many_workers, non_ascii_stream, random_stream,  # noqa: E402
                         relay, shared_by_worker_stream, stitch_stream, worker_stream)
from telemetry_corpus import body as _body  # noqa: E402
from thin_cases import PERCENTAGES, UNKNOWN_STATUSES, boundary_ids, mixed_stream, progress_body  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"


@functools.lru_cache(maxsize=None)
def _want(data: bytes, dialect: str) -> HostReport:
    return hosts_cpu(data, dialect)


def _same(data: bytes, dialect: str = "protobufjs", public: bool = False, **kw) -> tuple:
    """Asserts the device result against the definition; returns ``(HostReport, host_frames)``."""
    want = _want(data, dialect)
    got, host_frames = gh.hosts(data, DEVICE, dialect, **kw)
    assert (got.frames, got.progress_events, got.progress_decode_errors) == \
        (want.frames, want.progress_events, want.progress_decode_errors)
    assert got.hosts == want.hosts
    assert got.pairs == want.pairs
    assert got.media == want.media
    assert got == want
    if public:
        assert hosts_gpu(data, DEVICE, dialect, **kw) == want  # the public call
    return want, host_frames


def _both(data: bytes, **kw) -> HostReport:
    """Both dialects; returns the protobufjs report."""
    _same(data, "upb", **kw)
    return _same(data, "protobufjs", **kw)[0]


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for dialect in ops.DIALECTS:
        assert hosts_gpu(b"", DEVICE, dialect) == HostReport() == hosts_cpu(b"", dialect)
        assert gh.hosts(b"", DEVICE, dialect) == (HostReport(), 0)
    assert hosts_file(io.BytesIO(b""), DEVICE) == (HostReport(), 0)


def test_a_stream_with_no_progress_event_stops_after_the_counts(monkeypatch):
    def no_launch(*a, **kw):
        raise AssertionError("nothing to sort or to walk")
    for module, name in ((gt, "compact"), (gt, "sort"), (gh, "prepare"), (gh, "number"), (gh, "pairs"), (gh, "walk")):
        monkeypatch.setattr(module, name, no_launch)
    data = frames([(STATUS_ID, _body(b"m", 1)), (PROGRESS_ID, b"\x2e"), (9, progress_body(b"m", 2, 5, b"a"))] * 3)
    want = _both(data)
    assert (want.frames, want.progress_events, want.progress_decode_errors) == (9, 0, 3)
    # and where the CPU holds the only events
    data = worker_stream([("é".encode(), b"a", 2, 5), (b"m", "é".encode(), 2, 4)] * 2)
    want, host_frames = _same(data)
    assert host_frames == 4 and want.rewinds == 0 and want.progress_events == 4


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (progress_body(b"m-1", 3, 40, b"node-a"), progress_body(b"m-1", 3, 40), b"", b"\x2e",
                 progress_body(b"", 64, -1, b"")):
        for dialect in ops.DIALECTS:
            want, host_frames = _same(frames([(topic, body)]), dialect)
            assert want.frames == 1 and host_frames == 0
            assert want.progress_events == (topic == PROGRESS_ID and body != b"\x2e")


def test_two_events():
    same = _both(worker_stream([(b"m", b"a", 2, 11), (b"m", b"a", 2, 19)]))
    assert same.hosts == {"a": HostRow(2, {2: 2}, 1, 0, 0, 0)}
    fell = _both(worker_stream([(b"m", b"a", 2, 19), (b"m", b"a", 2, 11)]))
    assert fell.hosts == {"a": HostRow(2, {2: 2}, 1, 0, 0, 1)}
    two = _both(worker_stream([(b"m", b"a", 2, 19), (b"m", b"b", 2, 11)]))
    assert two.hosts == {"a": HostRow(1, {2: 1}, 1, 0, 1, 0), "b": HostRow(1, {2: 1}, 1, 1, 0, 0)}
    apart = _both(worker_stream([(b"m", b"a", 2, 19), (b"n", b"a", 2, 11)]))
    assert apart.hosts == {"a": HostRow(2, {2: 2}, 2, 0, 0, 0)} and len(apart.pairs) == 2


def test_two_media_interleaved_across_three_workers():
    events = [(b"a", b"w1", 2, 1), (b"b", b"w2", 2, 1), (b"a", b"w1", 2, 0), (b"b", b"w3", 2, 12), (b"a", b"w2", 2, 13),
              (b"b", b"w3", 3, 2), (b"a", b"w1", 3, 13), (b"b", b"w2", 3, 1)]
    want = _both(worker_stream(events), public=True)
    assert want.handovers == 4 and want.rewinds == 1 and len(want.pairs) == 4
    assert want.hosts["w1"] == HostRow(3, {2: 2, 3: 1}, 2, 1, 1, 1)


@pytest.mark.parametrize("workers", [(b"a", b"b"), (b"a",)], ids=["alternating", "one"])
def test_65_events_of_one_media(workers):
    """A wave boundary inside a media's run."""
    for rising in (True, False):
        want = _both(relay([b"m"] * 65, workers, rising=rising))
        assert want.handovers == (64 if len(workers) == 2 else 0)
        assert want.rewinds == (64 if len(workers) == 1 and not rising else 0)


@pytest.mark.parametrize("full", [gt.SORT_TILE, gt.SORT_BLOCK], ids=["tile", "block"])
@pytest.mark.parametrize("media", [1, 2])
def test_one_event_past_a_boundary(media, full):
    """``full`` events fill a tile of the sort and the walk, or their whole block; the next unit holds
    a single one, whose predecessor the walk reads across the edge: once as the stint goes on, once
    as a handover, once as a rewind."""
    ids = boundary_ids(full + 1, media)
    stint = _both(relay(ids, (b"a",)))
    assert stint.hosts["a"].stints == media and stint.rewinds == 0
    # the worker changes every 2 * media events but for the last event, whose worker is new
    events = [(mid, b"w%d" % (k // (2 * media) % 3), 2, k) for k, mid in enumerate(ids[:-1])]
    events.append((ids[-1], b"late", 2, 0))
    handover = _both(worker_stream(events))
    assert handover.hosts["late"] == HostRow(1, {2: 1}, 1, 1, 0, 0)
    rewind = _both(relay(ids[:-1], (b"a",)) + worker_stream([(ids[-1], b"a", 2, -5)]))
    assert rewind.rewinds == 1 and rewind.handovers == 0
    falling = _both(relay(ids, (b"a",), rising=False))
    assert falling.rewinds == full + 1 - media


@pytest.mark.parametrize("media", [2, 257])
def test_pass_counts(media):
    """One sort pass for two media, two for 257."""
    assert gt.sort_passes(media) == {2: 1, 257: 2}[media]
    rng = random.Random(media)
    ids = [b"media-%04d" % k for k in range(media)] * 8
    rng.shuffle(ids)
    events = [(mid, rng.choice(ASCII_WORKERS[:2]), 2, rng.choice((0, 5, 10))) for mid in ids]
    want = _both(worker_stream(events))
    assert len(want.media) == media and want.handovers > media and want.rewinds > 0


@pytest.mark.parametrize("workers", [gh.LDS_WORKERS - 1, gh.LDS_WORKERS, gh.LDS_WORKERS + 1, 3 * gh.LDS_WORKERS + 5])
def test_workers_around_the_lds_cap(workers):
    want = _both(many_workers(workers))
    assert len(want.hosts) == workers and want.rewinds == workers and want.handovers == workers - 3
    assert all(row == HostRow(2, {2 + int(name[2:]) % 2: 2}, 1, int(name[2:]) >= 3, int(name[2:]) < workers - 3, 1)
               for name, row in want.hosts.items())


def test_one_frame_past_a_block_of_the_scan():
    count = gpu_extract.SCAN_BLOCK + 1
    want = _both(relay(boundary_ids(count, 3), (b"a", b"b")))
    assert want.progress_events == count
    data = frames([(STATUS_ID, _body(b"m", 1))] * (count - 1) + [(PROGRESS_ID, progress_body(b"m", 2, 5, b"a"))])
    assert _both(data).media["m"].first == (count - 1, "a", 2, 5)


def test_everything_in_one_probe_chain():
    """Every id, every worker and every pair meet in one chain of their table."""
    for mask in (0, 0xFF):
        _both(random_stream(1), hash_mask=mask)
        _both(mixed_stream(), hash_mask=mask)
        _both(many_workers(70), hash_mask=mask)
        _both(relay(boundary_ids(300, 7), ASCII_WORKERS + (b"",)), hash_mask=mask)


def test_strings_that_differ_in_the_last_byte_only():
    rng = random.Random(1)
    names = [name for pair in collision_pairs() for name in pair]
    ids = names * 3
    rng.shuffle(ids)
    events = [(mid, rng.choice(names[:6]), 2, rng.choice((0, 5, 10))) for mid in ids]
    for mask in (None, 0):
        want = _both(worker_stream(events), hash_mask=mask)
        assert len(want.media) == len(names) and len(want.hosts) == 6


def test_worker_strings_and_ids():
    # a worker string whose bytes equal a media id's; the empty worker and the absent one are one; a
    # worker that is a prefix of another
    events = [(b"node", b"node", 2, 1), (b"node", b"m", 2, 2), (b"m", b"node", 2, 3), (b"m", b"", 2, 4),
              (b"m", None, 2, 3), (b"", b"node", 2, 1), (b"", b"node-1", 2, 0), (b"m", b"nod", 2, 9),
              (b"m", b"node-1", 2, 9), (b"node-1", b"nod", 2, 9), (b"", None, 2, 9)]
    want = _both(worker_stream(events), public=True)
    assert set(want.hosts) == {"node", "m", "", "node-1", "nod"} and set(want.media) == {"node", "m", "", "node-1"}
    assert want.hosts[""] == HostRow(3, {2: 3}, 2, 2, 1, 1)
    _both(worker_stream(events), hash_mask=0)


def test_unknown_statuses_and_the_percentage_edges():
    events = []
    for status in (2, 3) + UNKNOWN_STATUSES:
        for p in PERCENTAGES + PERCENTAGES[::-1]:
            events.append((b"edge", ASCII_WORKERS[len(events) // 5 % 3], status, p))
            events.append((b"edge", ASCII_WORKERS[len(events) // 5 % 3], status, p))
    want = _both(worker_stream(events))
    assert want.rewinds > 10 and any("unknown" in row.by_class for row in want.hosts.values())
    for dialect in ops.DIALECTS:
        _same(random_stream(2), dialect)
        _same(random_stream(3), dialect)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_fold_corpus(dialect):
    want, host_frames = _same(_corpus(), dialect, public=True)
    assert want.frames == 5711 and 0 < host_frames <= 0.05 * want.frames and want.handovers > 1000
    if dialect == "protobufjs":
        assert host_frames == 127
    _same(_corpus(), dialect, hash_mask=0xFFF)


def test_a_media_shared_between_cpu_and_device():
    """upb leaves the frames with a group to the CPU, and both dialects those with a non-ASCII worker:
    most events of the shared media have their neighbour on the other side, so the CPU must take the
    device's contributions out and decide the whole run."""
    data = stitch_stream()
    want, host_frames = _same(data, "upb", public=True)
    assert host_frames == 9 + 9 + 6 and want.progress_events == 51 and want.handovers > 10 and want.rewinds > 0
    same, none = _same(data, "protobufjs")
    assert none == 0 and same == want
    _same(data, "upb", hash_mask=0)
    # the CPU's frames first, last and in the middle of the run, and a media that only the CPU holds
    data = shared_by_worker_stream()
    for dialect in ops.DIALECTS:
        want, host_frames = _same(data, dialect, public=True)
        assert host_frames == 12 and set(want.media) == {"first", "last", "middle", "cpu-only", "dev-only"}
        assert want.media["first"].first[1] == "nœud" and want.media["last"].last[1] == "nœud"
        assert want.hosts["ノード"].taken == 1 + 2 and want.hosts["ノード"].lost == 1 + 3
        _same(data, dialect, hash_mask=0)
    group = b"\x2b\x2c"
    events = [(PROGRESS_ID, progress_body(b"m", 2, 9, b"a") + group), (PROGRESS_ID, progress_body(b"m", 2, 2, b"a")),
              (PROGRESS_ID, progress_body(b"host-only", 3, 3, b"b") + group),
              (PROGRESS_ID, progress_body(b"m", 2, 3, b"b")),
              (PROGRESS_ID, progress_body(b"host-only", 3, 4, b"a") + group),
              (PROGRESS_ID, progress_body(b"m", 2, 1, b"b") + group)]
    want, host_frames = _same(frames(events), "upb")
    assert host_frames == 4 and want.rewinds == 2 and want.handovers == 2
    assert _same(frames(events[::2]), "upb")[1] == 3  # the device holds no event at all


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_non_ascii_ids_are_decided_on_the_cpu(dialect):
    want, host_frames = _same(non_ascii_stream(), dialect)
    assert host_frames > 150 and want.handovers > 50
    two = worker_stream([(b"\xff", b"a", 2, 5), (b"\xfe", b"b", 2, 6), (b"\xff", b"a", 2, 7), (b"\xfe", b"a", 2, 1)])
    want, host_frames = _same(two, dialect)
    assert host_frames == 4
    # protobufjs: one media, U+FFFD; upb raises on invalid UTF-8: no event
    assert (want.progress_events, want.handovers, want.rewinds) == ((4, 2, 1) if dialect == "protobufjs" else (0, 0, 0))


def test_the_small_streams_and_two_runs_are_equal():
    for data in (mixed_stream(), random_stream(1)):
        _both(data)
    first = hosts_gpu(_corpus(), DEVICE)
    assert first == hosts_gpu(_corpus(), DEVICE) == _want(_corpus(), "protobufjs")
    assert first.to_json(True) == hosts_gpu(_corpus(), DEVICE).to_json(True)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_hosts_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device; media and stints cross the cuts."""
    data = _corpus()
    assert len(data) > 7 * 30_000
    want = _want(data, dialect)
    whole_host_frames = gh.hosts(data, DEVICE, dialect)[1]
    for chunk_bytes in (30_000, 1 << 30):
        got, host_frames = hosts_file(io.BytesIO(data), DEVICE, dialect, chunk_bytes=chunk_bytes)
        assert got == want and host_frames == whole_host_frames > 0
    assert hosts_file(io.BytesIO(data), "gpu", dialect, chunk_bytes=100_000)[0] == want


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = worker_stream([(b"m", b"a", 1, 5)] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gh.allocate(buf, offs_dev, n)
    gh.classify(tables)
    gh.claim(tables)
    gh.rank(tables)
    assert gh.counts(tables) == (1, 2, 1)
    s = gt.sort(gt.compact(tables.t, 1, 2))
    k = gh.prepare(tables, s, 1)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gh.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gh.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gh.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gh.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        gh.classify(tables, dialect="proto2")
    for workers in (0, 3):
        with pytest.raises(ValueError):
            gh.prepare(tables, s, workers)
    for bad in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError):
            gh.hosts(data, DEVICE, hash_mask=bad)
        with pytest.raises(ValueError):
            gh.pairs(tables, s, k, hash_mask=bad)
        with pytest.raises(ValueError):
            gh.walk(s, k, bad)
    with pytest.raises(ValueError):
        hosts_gpu(data, DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        hosts_gpu(data, "cpu")
    with pytest.raises(ValueError):
        hosts_gpu(data[:-1], DEVICE)  # broken framing never reaches the device
    with pytest.raises(ValueError):
        hosts_file(io.BytesIO(data), DEVICE, dialect="proto2")


def test_the_entry_points_refuse_null_pointers_and_impossible_counts():
    """Each returns hipErrorInvalidValue (1) and launches nothing; a count <= 0 returns 0."""
    so = hip_lib.lib()
    assert so.bh_hosts_classify(None, None, 0, 1, None, None, None, None, None, None, None) == 0
    assert so.bh_hosts_classify(None, None, 4, 1, None, None, None, None, None, None, None) == 1
    assert so.bh_hosts_number(None, -1, 4, None, None, 8, None, None, None, None) == 0
    assert so.bh_hosts_number(None, 4, 4, None, None, 8, None, None, None, None) == 1
    assert so.bh_hosts_pairs(None, None, 0, 0, None, None, None, 8, None) == 0
    assert so.bh_hosts_pairs(None, None, 4, 0, None, None, None, 8, None) == 1
    assert so.bh_hosts_walk(None, None, None, None, 0, 1, 1, 0, None, None, None, None) == 0
    assert so.bh_hosts_walk(None, None, None, None, 4, 1, 1, 0, None, None, None, None) == 1
    data = worker_stream([(b"m", b"a", 1, 5)] * 4)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tb = gh.allocate(buf, offs_dev, n)
    gh.classify(tb)
    gh.claim(tb)
    gh.rank(tb)
    s = gt.sort(gt.compact(tb.t, 1, 4))
    k = gh.prepare(tb, s, 1)
    p = [x.data_ptr() for x in (s.keys, s.vals, k.worker_of, k.prog, k.worker_rows, k.run_start, k.run_end)]
    assert so.bh_hosts_walk(p[0], p[1], p[2], p[3], 4, 5, 1, 0, p[4], p[5], p[6], None) == 1  # more media than events
    assert so.bh_hosts_walk(p[0], p[1], p[2], p[3], 4, 1, 0, 0, p[4], p[5], p[6], None) == 1  # no worker
    assert so.bh_hosts_pairs(p[0], p[2], 4, 0, k.pair_claim.data_ptr(), k.pair_scan.keep_len.data_ptr(),
                             k.pair_count.data_ptr(), 6, None) == 1  # a table that is no power of two
    assert so.bh_hosts_pairs(p[0], p[2], 4, 0, k.pair_claim.data_ptr(), k.pair_scan.keep_len.data_ptr(),
                             k.pair_count.data_ptr(), 4, None) == 1  # a table below twice the events
    assert so.bh_hosts_number(p[1], 5, 4, tb.w.slot_of.data_ptr(), tb.w.slot_scan.pos.data_ptr(), tb.w.slots,
                              tb.progress.data_ptr(), p[2], p[3], None) == 1  # more events than frames
    torch = pytest.importorskip("torch")
    torch.cuda.synchronize()
    assert int(k.worker_rows.sum()) == 0  # nothing was launched
