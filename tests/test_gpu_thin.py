"""``thin`` on the GPU (ops/hip/telemetry_thin.hip, ops/gpu_thin.py) against its definition,
``thin.thin_cpu``: every comparison is full ``Thinned`` equality (the kept bytes, the kept indices,
the frame and event counts), exact, for both ``keep`` unless noted."""
from __future__ import annotations

import functools
import io
import random

import pytest

from beholder_amd import ops
from beholder_amd.ops import frames
from beholder_amd.thin import Policy, Thinned, thin_cpu, thin_file, thin_gpu
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_extract, gpu_fold, gpu_thin as gth, gpu_transitions as gt, hip_lib  # noqa: E402
from extract_cases import collision_pairs  # noqa: E402
from telemetry_corpus import body as _body  # noqa: E402
from thin_cases import (KEEPS, POLICIES, boundary_ids, corpus as _corpus, course, edge_stream,  # noqa: E402
                        mixed_stream, non_ascii_stream, policy_id, progress_body, progress_stream, random_stream,
                        stitch_stream)

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"


@functools.lru_cache(maxsize=None)
def _want(data: bytes, policy: Policy, dialect: str) -> Thinned:
    return thin_cpu(data, policy, dialect)


def _same(data: bytes, policy: Policy = Policy(), dialect: str = "protobufjs", public: bool = False, **kw) -> tuple:
    """Asserts the device result against the definition; returns ``(Thinned, host_frames)``."""
    want = _want(data, policy, dialect)
    got, host_frames = gth.thin(data, policy, DEVICE, dialect, **kw)
    assert (got.frames, got.progress_events, got.step, got.keep) == \
        (want.frames, want.progress_events, want.step, want.keep)
    assert got.indices == want.indices
    assert got.data == want.data
    assert got == want
    if public:
        assert thin_gpu(data, policy, DEVICE, dialect, **kw) == want  # the public call
    return want, host_frames


def _both(data: bytes, step: int = 10, dialect: str = "protobufjs", **kw) -> dict:
    """Both ``keep`` modes; returns the kept indices per mode."""
    return {keep: _same(data, Policy(step, keep), dialect, **kw)[0].indices for keep in KEEPS}


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for dialect in ops.DIALECTS:
        for policy in POLICIES:
            want = Thinned(b"", [], 0, policy.step, policy.keep, dialect, 0)
            assert thin_gpu(b"", policy, DEVICE, dialect) == want == thin_cpu(b"", policy, dialect)
            assert gth.thin(b"", policy, DEVICE, dialect) == (want, 0)
    out = io.BytesIO()
    assert thin_file(io.BytesIO(b""), out, Policy(), DEVICE)["frames"] == 0 and out.getvalue() == b""


def test_a_stream_with_no_progress_event_never_reaches_the_sort(monkeypatch):
    def no_sort(*a, **kw):
        raise AssertionError("nothing to sort")
    monkeypatch.setattr(gt, "compact", no_sort)
    monkeypatch.setattr(gt, "sort", no_sort)
    monkeypatch.setattr(gth, "mark", no_sort)
    data = frames([(STATUS_ID, _body(b"m", 1)), (PROGRESS_ID, b"\x2e"), (9, progress_body(b"m", 2, 5))] * 3)
    for dialect in ops.DIALECTS:
        assert _both(data, dialect=dialect) == {"last": list(range(9)), "first": list(range(9))}
    # and where the host holds the only events
    data = progress_stream([("é".encode(), 2, 5)] * 3)
    want, host_frames = _same(data)
    assert want.indices == [2] and host_frames == 3


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (progress_body(b"m-1", 3, 40), b"", b"\x2e", progress_body(b"", 64, -1)):
        for dialect in ops.DIALECTS:
            for keep in KEEPS:
                want, host_frames = _same(frames([(topic, body)]), Policy(10, keep), dialect)
                assert want.frames == 1 and want.indices == [0] and host_frames == 0
                assert want.progress_events == (topic == PROGRESS_ID and body != b"\x2e")


def test_two_events():
    assert _both(progress_stream([(b"m", 2, 11), (b"m", 2, 19)])) == {"last": [1], "first": [0]}
    assert _both(progress_stream([(b"m", 2, 9), (b"m", 2, 10)])) == {"last": [0, 1], "first": [0, 1]}
    assert _both(progress_stream([(b"m", 2, 11), (b"m", 3, 11)])) == {"last": [0, 1], "first": [0, 1]}
    assert _both(progress_stream([(b"m", 2, 11), (b"n", 2, 11)])) == {"last": [0, 1], "first": [0, 1]}
    assert _both(progress_stream([(b"m", 2, -1), (b"m", 2, 0)])) == {"last": [0, 1], "first": [0, 1]}


def test_two_media_interleaved():
    events = [(b"a", 2, 1), (b"b", 2, 1), (b"a", 2, 2), (b"b", 2, 12), (b"a", 2, 13), (b"b", 2, 14), (b"a", 3, 13)]
    assert _both(progress_stream(events)) == {"last": [1, 2, 4, 5, 6], "first": [0, 1, 3, 4, 6]}
    _same(progress_stream(events), public=True)


def test_65_events_of_one_media_with_one_mark():
    """A wave boundary inside a media's run."""
    assert _both(course([b"m"] * 65, "constant")) == {"last": [64], "first": [0]}
    kept = _both(course([b"m"] * 65, "constant", status_every=3))
    assert len(kept["last"]) == len(kept["first"]) == 1 + 22
    assert _both(course([b"m"] * 65))["last"] == list(range(65))


@pytest.mark.parametrize("full", [gt.SORT_TILE, gt.SORT_BLOCK], ids=["tile", "block"])
@pytest.mark.parametrize("media", [1, 2])
def test_one_event_past_a_boundary(media, full):
    """``full`` events fill a tile of the sort, or its whole block; the next unit holds a single one,
    whose neighbour the mark kernel reads across the edge."""
    ids = boundary_ids(full + 1, media)
    assert _both(course(ids)) == {"last": list(range(full + 1)), "first": list(range(full + 1))}  # nothing is dropped
    assert _both(course(ids, "constant")) == {"last": list(range(full + 1 - media, full + 1)),
                                               "first": list(range(media))}
    kept = _both(course(ids, "constant", status_every=5))  # the events are not the frames
    assert len(kept["last"]) == len(kept["first"]) == media + (full + 5) // 5


@pytest.mark.parametrize("media", [2, 257])
def test_pass_counts(media):
    """One sort pass for two media, two for 257; every media has a stretch to drop."""
    assert gt.sort_passes(media) == {2: 1, 257: 2}[media]
    rng = random.Random(media)
    ids = [b"media-%04d" % k for k in range(media)] * 4
    rng.shuffle(ids)
    seen = {}
    events = []
    for mid in ids:
        k = seen[mid] = seen.get(mid, -1) + 1
        events.append((mid, 2, (0, 5, 10, 12)[k]))  # marks a, a, b, b: two of four survive
    kept = _both(progress_stream(events))
    assert len(kept["last"]) == len(kept["first"]) == 2 * media and kept["last"] != kept["first"]


def test_one_frame_past_a_block_of_the_scan():
    count = gpu_extract.SCAN_BLOCK + 1
    kept = _both(course(boundary_ids(count, 3), "constant"))
    assert kept == {"last": [count - 3, count - 2, count - 1], "first": [0, 1, 2]}
    data = frames([(STATUS_ID, _body(b"m", 1))] * (count - 1) + [(PROGRESS_ID, progress_body(b"m", 2, 5))])
    assert _both(data)["last"] == list(range(count))


def test_every_id_in_one_probe_chain():
    for dialect in ops.DIALECTS:
        _both(random_stream(1), dialect=dialect, hash_mask=0)
        _both(mixed_stream(), dialect=dialect, hash_mask=0)
    _both(course(boundary_ids(300, 7), "constant"), hash_mask=0xFF)


def test_ids_that_differ_in_the_last_byte_only():
    rng = random.Random(1)
    ids = [mid for pair in collision_pairs() for mid in pair] * 3
    rng.shuffle(ids)
    events = [(mid, 2, rng.choice((0, 5, 10))) for mid in ids]
    for mask in (None, 0):
        kept = _both(progress_stream(events), hash_mask=mask)
        assert 120 <= len(kept["last"]) < 360


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_percentage_and_step_edges(policy):
    for dialect in ops.DIALECTS:
        want, host_frames = _same(edge_stream(), policy, dialect)
        assert host_frames == 0 and len(want.indices) < want.frames
        _same(random_stream(2), policy, dialect)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_fold_corpus(dialect):
    for keep in KEEPS:
        want, host_frames = _same(_corpus(), Policy(10, keep), dialect, public=keep == "last")
        assert want.frames > 5000 and 0 < host_frames <= 0.05 * want.frames and len(want.indices) < want.frames
    _same(_corpus(), Policy(25), dialect, hash_mask=0xFFF)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_small_streams(dialect):
    for data in (mixed_stream(), random_stream(1), random_stream(3)):
        _both(data, dialect=dialect)
        _both(data, step=1, dialect=dialect)


def test_a_media_shared_between_host_and_device():
    """upb leaves the frames with a group to the host: most events of the two shared media have
    their neighbour on the other side, so the host must rewrite decisions the device made."""
    data = stitch_stream()
    for keep in KEEPS:
        want, host_frames = _same(data, Policy(10, keep), "upb", public=True)
        assert host_frames == 9 + 9 + 6 > 0 and want.progress_events == 51
        assert len(want.indices) == 6 + 6 + 3 + 3  # stretches of three, three and two
        same, none = _same(data, Policy(10, keep), "protobufjs")
        assert none == 0 and same.indices == want.indices
        _same(data, Policy(10, keep), "upb", hash_mask=0)
    # the host's frames first and last in the shared media, and a media that only the host holds
    group = b"\x2b\x2c"
    events = [(PROGRESS_ID, progress_body(b"m", 2, 1) + group), (PROGRESS_ID, progress_body(b"m", 2, 2)),
              (PROGRESS_ID, progress_body(b"host-only", 3, 3) + group), (PROGRESS_ID, progress_body(b"m", 2, 3)),
              (PROGRESS_ID, progress_body(b"host-only", 3, 4) + group),
              (PROGRESS_ID, progress_body(b"m", 2, 4) + group)]
    for keep, kept in (("last", [4, 5]), ("first", [0, 2])):
        want, host_frames = _same(frames(events), Policy(10, keep), "upb")
        assert host_frames == 4 and want.indices == kept
        assert _same(frames(events[::2]), Policy(10, keep), "upb")[1] == 3  # the device holds no event at all


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_non_ascii_ids_are_decided_on_the_host(dialect):
    data = non_ascii_stream()
    for keep in KEEPS:
        want, host_frames = _same(data, Policy(10, keep), dialect)
        assert host_frames > 150 and len(want.indices) < want.frames
    two = progress_stream([(b"\xff", 2, 5), (b"\xfe", 2, 6), (b"\xff", 2, 7), (b"\xfe", 2, 15)])
    want, host_frames = _same(two, Policy(), dialect)
    assert host_frames == 4
    # protobufjs: one media, U+FFFD; upb raises on invalid UTF-8: no event
    assert want.indices == ([2, 3] if dialect == "protobufjs" else [0, 1, 2, 3])


def test_the_dropped_counter_counts_the_dropped_frames():
    data = course(boundary_ids(gt.SORT_BLOCK + 70, 3), "constant", status_every=4)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    for policy in (Policy(), Policy(keep="first")):
        tb = gth.allocate(buf, offs_dev, n)
        gth.classify(tb, policy)
        gt.claim(tb.t)
        gt.rank(tb.t)
        groups, events = gt.counts(tb.t)
        assert (groups, events) == (3, gt.SORT_BLOCK + 70)
        s = gt.sort(gt.compact(tb.t, groups, events))
        gth.mark(tb, s, policy)
        counters = tb.t.counters.cpu().numpy().tolist()
        assert counters == [0, 0, events - 3]
        assert int((tb.keep_len == 0).sum()) == events - 3


def test_thin_is_deterministic():
    first = thin_gpu(_corpus(), Policy(), DEVICE)
    assert first == thin_gpu(_corpus(), Policy(), DEVICE) == _want(_corpus(), Policy(), "protobufjs")


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("keep", KEEPS)
def test_thin_file_on_the_device_in_chunks(keep, dialect):
    """Eight chunks or so, each through the device; a media's course crosses the cuts."""
    data = _corpus()
    assert len(data) > 7 * 30_000
    policy = Policy(10, keep)
    want = _want(data, policy, dialect)
    for chunk_bytes in (30_000, 1 << 30):
        out, indices = io.BytesIO(), io.StringIO()
        counts = thin_file(io.BytesIO(data), out, policy, DEVICE, dialect, chunk_bytes=chunk_bytes, indices_out=indices)
        assert out.getvalue() == want.data
        assert [int(line) for line in indices.getvalue().split()] == want.indices
        assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                          "progress_events": want.progress_events, "dropped": want.frames - len(want.indices),
                          "host_frames": gth.thin(data, policy, DEVICE, dialect)[1]}
        assert counts["host_frames"] > 0


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = progress_stream([(b"m", 1, 5)] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gth.allocate(buf, offs_dev, n)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gth.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gth.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gth.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gth.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        gth.classify(tables, Policy(), dialect="proto2")
    with pytest.raises(TypeError):
        gth.classify(tables, 10)
    bad_step = Policy()
    object.__setattr__(bad_step, "step", 0)  # a policy that got past its own check
    for call in (lambda: gth.classify(tables, bad_step), lambda: gth.thin(data, bad_step, DEVICE)):
        with pytest.raises(ValueError):
            call()
    object.__setattr__(bad_step, "step", 2 ** 31)
    with pytest.raises(ValueError):
        gth.thin(data, bad_step, DEVICE)
    for bad in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError):
            gth.thin(data, Policy(), DEVICE, hash_mask=bad)
    with pytest.raises(TypeError):
        gth.thin(data, "last", DEVICE)
    with pytest.raises(ValueError):
        thin_gpu(data, Policy(), DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        thin_gpu(data, Policy(), "cpu")
    with pytest.raises(ValueError):
        thin_gpu(data[:-1], Policy(), DEVICE)  # broken framing never reaches the device
    with pytest.raises(ValueError):
        thin_file(io.BytesIO(data), io.BytesIO(), Policy(), DEVICE, dialect="proto2")
