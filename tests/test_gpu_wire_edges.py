"""The systematic wire-format corpus (wire_edges.py) on the device. Every assertion is exact equality.

* decode: the kernel's table over every body against ``gpu_decode.reference_table`` in both dialects,
  and in protobufjs against what the service's codec decodes.
* The per-frame table that a classify, mark or route launch leaves on the device, read back after
  that launch alone and compared frame by frame with ``wire_edges.expected``, the codec's reading:
  the kind (not read, error, left to the host, event), the id span's bytes, and the status, the
  progress, the worker string and the hash where the table holds them. These are the STRICT upb
  reader, the TelemetryStatus reads and the per-frame headers as hipcc compiled them for gfx950; the
  host programs of test_hip_*_host.py check the same headers as g++ compiled them.
* Every command whole over ``wire_edges.stream(6000)`` against its CPU definition, with the
  full-result equality of its own test file, in both dialects and with every id in one probe chain."""
from __future__ import annotations

import functools

import pytest

from beholder_amd import coalesce as co, ops, replay, shard as sh, thin as th
from beholder_amd.extract import extract_cpu
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import (gpu_coalesce as gc, gpu_decode as gd, gpu_extract as gx, gpu_fold,  # noqa: E402
                              gpu_hosts as gh, gpu_shard as gsh, gpu_stages as gst, gpu_thin as gth,
                              gpu_transitions as gt)
import test_gpu_coalesce  # noqa: E402  the commands' own comparisons with their definitions
import test_gpu_dedupe  # noqa: E402
import test_gpu_extract  # noqa: E402
import test_gpu_hosts  # noqa: E402
import test_gpu_shard  # noqa: E402
import test_gpu_stages  # noqa: E402
import test_gpu_thin  # noqa: E402
import test_gpu_transitions  # noqa: E402
import wire_edges  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
SKIP, ERROR, HOST, EVENT = 0, 1, 2, 3  # TR_* of telemetry_transitions.hpp, which thin, hosts and stages share
MASKS = [None, 0]
WHOLE = 6000  # frames of the stream the whole commands run over: the size of the fold corpus


# ---- decode ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_decode_rows_equal_the_definition_on_every_body(dialect):
    bodies = wire_edges.bodies()
    got = gd.decode_bodies(bodies, DEVICE, dialect)
    want = gd.reference_table(bodies, dialect)
    assert got.shape == want.shape == (len(bodies), 8)
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert len(bad) == 0, (len(bad), [(bodies[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    if dialect == "protobufjs":  # and the rows materialise to what the service decodes
        buf, _ = gd.pack(bodies)
        rows = gd.materialise(buf, got)
        values = [None if v is None else tuple(v) for v in wire_edges.expected(dialect)[1::2]]  # the progress frames
        diffs = [(bodies[i], rows[i], values[i]) for i in range(len(bodies)) if rows[i] != values[i]]
        assert not diffs, (len(diffs), diffs[:5])


# ---- the per-frame tables ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _uploaded() -> tuple:
    """``(stream, n, offs, buf, offs_dev)`` of the whole corpus; no launch writes to the two device tensors."""
    stream = wire_edges.stream()
    n, offs = gpu_fold.index(stream)
    assert n == len(wire_edges.events())
    buf, offs_dev = gpu_fold.upload(stream, offs, DEVICE)
    return stream, n, offs, buf, offs_dev


def _hashes(rows) -> list:
    """The 64-bit hash of every row of a ``(n, 6)`` int32 table: its first two words."""
    words = rows[:, :2].astype(np.int64) & 0xFFFFFFFF
    return ((words[:, 1] << 32) | words[:, 0]).astype(np.uint64).tolist()


def _ascii(text: str):
    """The bytes of a string the device keeps itself, None for one it must hand over."""
    return text.encode("ascii") if text.isascii() else None


def _compare(dialect: str, topics: set, kinds, want_event, got_event) -> set:
    """Every frame's kind against the codec; an event's ``got_event(i)`` against ``want_event(i, values)``
    (None where the device must not decide the frame). Returns the frames the device left to the host."""
    expected = wire_edges.expected(dialect)
    host, bad = set(), []
    for i, ((topic, body), values) in enumerate(zip(wire_edges.events(), expected)):
        kind = kinds[i]
        if kind == HOST:
            host.add(i)
            continue
        if topic not in topics:
            want = (SKIP, None)
        elif values is None:
            want = (ERROR, None)
        else:
            want = (EVENT, want_event(i, values))
        got = (kind, got_event(i) if kind == EVENT else None)
        if got != want:
            bad.append((i, topic, body, got, want))
    assert not bad, (len(bad), bad[:5])
    return host


def _held_to_the_rule(dialect: str, topics: set, host: set, overflow, high=lambda v: not v.media_id.isascii()) -> None:
    """The host set is the overflow list, stays under the cap, and under protobufjs is the rule's:
    the frame decodes and a string the command keys by is not ASCII."""
    compared = sum(topic in topics for topic, _ in wire_edges.events())
    print(f"{dialect}: {compared} frames compared, {len(host)} left to the host")
    assert sorted(overflow.tolist()) == sorted(host)
    assert all(wire_edges.events()[i][0] in topics for i in host)
    assert len(host) <= wire_edges.HOST_CAP[dialect] * compared
    if dialect == "protobufjs":
        expected = wire_edges.expected(dialect)
        assert host == {i for i, (topic, _) in enumerate(wire_edges.events())
                        if topic in topics and expected[i] is not None and high(expected[i])}


def _span(stream: bytes, offs, i: int, off: int, length: int) -> bytes:
    """The bytes of a span the device reported for frame ``i``; it lies inside the frame's body."""
    assert length == 0 or int(offs[i]) + 5 <= off and off + length <= int(offs[i + 1]), (i, off, length)
    return stream[off:off + length]


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_transitions_classify_frame_by_frame(dialect):
    stream, n, offs, buf, offs_dev = _uploaded()
    t = gt.allocate(buf, offs_dev, n)
    gt.classify(t, dialect)
    rows, is_event, counters = t.rows.cpu().numpy(), t.is_event.cpu().numpy(), t.counters.cpu().numpy()
    hashes = _hashes(rows)
    host = _compare(
        dialect, {STATUS_ID}, rows[:, 5].tolist(),
        lambda i, v: None if _ascii(v.media_id) is None else (_ascii(v.media_id), v.status, wire_edges.id_hash(v)),
        lambda i: (_span(stream, offs, i, int(rows[i, 2]), int(rows[i, 3])), int(rows[i, 4]), hashes[i]))
    _held_to_the_rule(dialect, {STATUS_ID}, host, t.overflow[:int(counters[gt.C_OVERFLOW])].cpu().numpy())
    assert is_event.tolist() == [int(k == EVENT) for k in rows[:, 5].tolist()]
    assert int(counters[gt.C_STATUS_ERR]) == int((rows[:, 5] == ERROR).sum()) > 2000
    assert not rows[rows[:, 5] != EVENT, :5].any()  # nothing but the kind where there is no event


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_thin_classify_frame_by_frame(dialect):
    stream, n, offs, buf, offs_dev = _uploaded()
    policy = th.Policy(10)
    tb = gth.allocate(buf, offs_dev, n)
    gth.classify(tb, policy, dialect)
    rows, marks, counters = tb.t.rows.cpu().numpy(), tb.marks.cpu().numpy().tolist(), tb.t.counters.cpu().numpy()
    hashes = _hashes(rows)

    def want_event(i, v):
        if _ascii(v.media_id) is None or dialect == "upb" and _ascii(v.host) is None:
            return None
        return _ascii(v.media_id), v.status, gth._word((v.media_id, v.status, v.progress // policy.step)), wire_edges.id_hash(v)
    host = _compare(
        dialect, {PROGRESS_ID}, rows[:, 5].tolist(), want_event,
        lambda i: (_span(stream, offs, i, int(rows[i, 2]), int(rows[i, 3])), int(rows[i, 4]), marks[i], hashes[i]))
    _held_to_the_rule(dialect, {PROGRESS_ID}, host, tb.t.overflow[:int(counters[gth.C_OVERFLOW])].cpu().numpy())
    assert int(counters[gth.C_PROGRESS_ERR]) == int((rows[:, 5] == ERROR).sum()) > 2000
    assert tb.keep_len.cpu().numpy().tolist() == np.diff(offs).tolist()  # every frame is kept until mark drops it
    assert not np.asarray(marks)[rows[:, 5] != EVENT].any()


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_hosts_classify_frame_by_frame(dialect):
    stream, n, offs, buf, offs_dev = _uploaded()
    tb = gh.allocate(buf, offs_dev, n)
    gh.classify(tb, dialect)
    rows, workers = tb.t.rows.cpu().numpy(), tb.w.rows.cpu().numpy()
    progress, counters = tb.progress.cpu().numpy().tolist(), tb.t.counters.cpu().numpy()
    hashes, worker_hashes = _hashes(rows), _hashes(workers)

    def want_event(i, v):
        if _ascii(v.media_id) is None or _ascii(v.host) is None:
            return None
        return (_ascii(v.media_id), _ascii(v.host), v.status, v.status, v.progress, wire_edges.id_hash(v),
                gpu_fold.hash64(_ascii(v.host)))
    host = _compare(
        dialect, {PROGRESS_ID}, rows[:, 5].tolist(), want_event,
        lambda i: (_span(stream, offs, i, int(rows[i, 2]), int(rows[i, 3])),
                   _span(stream, offs, i, int(workers[i, 2]), int(workers[i, 3])), int(rows[i, 4]), int(workers[i, 4]),
                   progress[i], hashes[i], worker_hashes[i]))
    _held_to_the_rule(dialect, {PROGRESS_ID}, host, tb.t.overflow[:int(counters[gh.C_OVERFLOW])].cpu().numpy(),
                      high=lambda v: not (v.media_id.isascii() and v.host.isascii()))
    assert workers[:, 5].tolist() == rows[:, 5].tolist()
    assert int(counters[gh.C_PROGRESS_ERR]) == int((rows[:, 5] == ERROR).sum()) > 2000
    assert not np.asarray(progress)[rows[:, 5] != EVENT].any()


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_stages_classify_frame_by_frame(dialect):
    stream, n, offs, buf, offs_dev = _uploaded()
    tb = gst.allocate(buf, offs_dev, n)
    gst.classify(tb, dialect)
    rows, aux, counters = tb.t.rows.cpu().numpy(), tb.aux.cpu().numpy().tolist(), tb.t.counters.cpu().numpy()
    hashes = _hashes(rows)
    topic_of = [topic for topic, _ in wire_edges.events()]

    def want_event(i, v):
        if _ascii(v.media_id) is None or dialect == "upb" and _ascii(v.host) is None:
            return None
        word = gst.AUX_STATUS if topic_of[i] == STATUS_ID else v.progress & 0xFFFFFFFF
        return _ascii(v.media_id), v.status, word, wire_edges.id_hash(v)
    host = _compare(
        dialect, {STATUS_ID, PROGRESS_ID}, rows[:, 5].tolist(), want_event,
        lambda i: (_span(stream, offs, i, int(rows[i, 2]), int(rows[i, 3])), int(rows[i, 4]), aux[i], hashes[i]))
    _held_to_the_rule(dialect, {STATUS_ID, PROGRESS_ID}, host,
                      tb.t.overflow[:int(counters[gst.C_OVERFLOW])].cpu().numpy())
    errors = np.asarray(topic_of)[rows[:, 5] == ERROR]
    assert int(counters[gst.C_STATUS_ERR]) == int((errors == STATUS_ID).sum()) > 2000
    assert int(counters[gst.C_PROGRESS_ERR]) == int((errors == PROGRESS_ID).sum()) > 2000


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_extract_mark_frame_by_frame(dialect):
    """The kept length of every frame the device decides, under a selector that keeps by media and by
    status, and the overflow list."""
    stream, n, offs, buf, offs_dev = _uploaded()
    selector = wire_edges.selector()
    names = replay.status_names()
    ids = gx.ascii_ids(selector.media)
    params = gx.select_params(selector, gx.table_slots(len(ids)))
    table, blob = gx.build_media_table(ids, params.hash_mask)
    t = gx.allocate(buf, offs_dev, n, table, blob)
    gx.mark(t, params, dialect)
    keep_len, lengths = t.keep_len.cpu().numpy().tolist(), np.diff(offs).tolist()
    overflow = t.overflow[:int(t.cursor.item())].cpu().numpy()
    listed = set(overflow.tolist())
    kept = [v is not None and v.media_id in selector.media and (v.status in selector.statuses or v.status not in names)
            for v in wire_edges.expected(dialect)]
    bad = [(i, wire_edges.events()[i], keep_len[i], kept[i]) for i in range(n)
           if i not in listed and keep_len[i] != (lengths[i] if kept[i] else 0)]
    assert not bad, (len(bad), bad[:5])
    assert 1000 < sum(kept) < n - 1000
    _held_to_the_rule(dialect, {STATUS_ID, PROGRESS_ID}, listed, overflow)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", [sh.Policy(7), sh.Policy(256, "drop")], ids=test_gpu_shard.policy_id)
def test_shard_route_frame_by_frame(policy, dialect):
    stream, n, offs, buf, offs_dev = _uploaded()
    t = gsh.allocate(buf, offs_dev, n, policy.shards)
    gsh.route(t, gsh.shard_params(policy), dialect)
    shard_of = t.shard_of.cpu().numpy().tolist()
    overflow = t.overflow[:int(t.cursor.item())].cpu().numpy()
    listed = set(overflow.tolist())
    undecoded = 0 if policy.undecoded == "first" else -1
    want = [undecoded if v is None else sh.shard_of(v.media_id, policy.shards) for v in wire_edges.expected(dialect)]
    bad = [(i, wire_edges.events()[i], shard_of[i], want[i]) for i in range(n) if i not in listed and shard_of[i] != want[i]]
    assert not bad, (len(bad), bad[:5])
    assert len(set(want)) > 4
    _held_to_the_rule(dialect, {STATUS_ID, PROGRESS_ID}, listed, overflow)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", [co.Policy(), co.Policy("last", "per-status", "drop")],
                         ids=test_gpu_coalesce.policy_id)
def test_coalesce_classify_frame_by_frame(policy, dialect):
    """The row the classify stage writes: kept or dropped where the codec raises, a key of id span,
    status (under per-status, for a progress), topic flag and key hash where it decodes."""
    stream, n, offs, buf, offs_dev = _uploaded()
    t = gc.allocate(buf, offs_dev, n)
    gc.launch(t, gc.coalesce_params(policy, t.slots), dialect, stages=gc.STAGE_CLASSIFY)
    rows = t.rows.cpu().numpy()
    hashes = _hashes(rows)
    overflow = t.overflow[:int(t.cursor.item())].cpu().numpy()
    undecoded = gc.CL_KEEP if policy.undecoded == "keep" else gc.CL_DROP
    host, bad = set(), []
    for i, ((topic, body), v) in enumerate(zip(wire_edges.events(), wire_edges.expected(dialect))):
        flags = int(rows[i, 5])
        if flags & gc.R_KIND == gc.CL_HOST:
            host.add(i)
            continue
        if v is None:
            want, got = (undecoded, None), (flags, None)
        elif _ascii(v.media_id) is None or dialect == "upb" and _ascii(v.host) is None:
            want, got = "left to the host", flags
        else:
            status = v.status if topic == PROGRESS_ID and policy.progress == "per-status" else 0
            want = (gc.CL_KEYED | (gc.R_STATUS if topic == STATUS_ID else 0),
                    (_ascii(v.media_id), status, gc.key_hash(_ascii(v.media_id), topic, status)))
            got = (flags, (_span(stream, offs, i, int(rows[i, 2]), int(rows[i, 3])), int(rows[i, 4]), hashes[i]))
        if got != want:
            bad.append((i, topic, body, got, want))
    assert not bad, (len(bad), bad[:5])
    _held_to_the_rule(dialect, {STATUS_ID, PROGRESS_ID}, host, overflow)


# ---- every command whole, against its CPU definition ---------------------------------------------------

def _whole() -> bytes:
    data = wire_edges.stream(WHOLE)
    assert WHOLE // 2 < len(wire_edges.events(WHOLE)) <= WHOLE
    return data


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_fold_whole(dialect, mask):
    want = replay.fold_cpu(_whole(), dialect)
    assert want.status_decode_errors > 1000 and want.progress_decode_errors > 1000 and len(want.media) > 5
    assert replay.fold_gpu(_whole(), DEVICE, dialect, hash_mask=mask) == want


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_extract_whole(dialect, mask):
    want = extract_cpu(_whole(), wire_edges.selector(), dialect)
    assert 0 < len(want.indices) < want.frames
    test_gpu_extract._both_shapes(_whole(), wire_edges.selector(), want, dialect, hash_mask=mask)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_coalesce_whole(dialect, mask):
    for policy in (co.Policy(), co.Policy("last", "per-status", "drop")):
        want, _ = test_gpu_coalesce._same(_whole(), policy, dialect, hash_mask=mask)
        assert 0 < len(want.indices) < want.frames


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_shard_whole(dialect, mask):
    """The route reads no table, so the shard takes no ``hash_mask``: the two cases are two policies."""
    policy = sh.Policy(7) if mask is None else sh.Policy(256, "drop")
    want, _ = test_gpu_shard._same(_whole(), policy, dialect)
    assert sum(bool(i) for i in want.indices) > 4


@pytest.mark.parametrize("mask", MASKS)
def test_dedupe_whole(mask):
    """The dedupe compares bytes and reads no message: it has no dialect."""
    for policy in (test_gpu_dedupe.Policy(), test_gpu_dedupe.Policy("first")):
        want, _ = test_gpu_dedupe._same(_whole(), policy, hash_mask=mask)
        assert len(want.indices) == want.frames  # every body once per topic: nothing repeats
    want, _ = test_gpu_dedupe._same(_whole() * 2, test_gpu_dedupe.Policy(), hash_mask=mask)
    assert 2 * len(want.indices) == want.frames


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_transitions_whole(dialect, mask):
    want, _ = test_gpu_transitions._same(_whole(), dialect, hash_mask=mask)
    assert want.status_events > 200 and want.status_decode_errors > 1000


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_thin_whole(dialect, mask):
    for keep in test_gpu_thin.KEEPS:
        want, _ = test_gpu_thin._same(_whole(), th.Policy(10, keep), dialect, hash_mask=mask)
        assert want.progress_events > 200 and len(want.indices) < want.frames


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_hosts_whole(dialect, mask):
    want, _ = test_gpu_hosts._same(_whole(), dialect, hash_mask=mask)
    assert want.progress_events > 200 and want.progress_decode_errors > 1000


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_stages_whole(dialect, mask):
    want, _ = test_gpu_stages._same(_whole(), dialect, hash_mask=mask)
    assert want.status_events > 200 and want.progress_events > 200
