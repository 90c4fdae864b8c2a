"""``hosts``: the definition (beholder_amd/hosts.py) against its laws, the fold, the shard, its JSON
form, its chunked file form, the command line and hand-written cases."""
from __future__ import annotations

import io
import itertools
import json
import subprocess
import sys

import pytest

from beholder_amd import ops, replay, shard
from beholder_amd.hosts import HostReport, HostRow, MediaEdge, course_of, hosts_cpu, hosts_file
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transitions import UNKNOWN, class_of
from beholder_amd.transport.framing import iter_frames
from hosts_cases import corpus, one_worker, random_stream, stitch_stream, worker_stream
from telemetry_corpus import body
from thin_cases import progress_body

SEEDS = (1, 2, 3)


def _boundaries(data: bytes):
    off = 0
    yield 0
    for _, b in iter_frames(data):
        off += 5 + len(b)
        yield off


def _check_laws(r: HostReport) -> None:
    assert sum(row.events for row in r.hosts.values()) == r.progress_events == sum(r.pairs.values()) \
        == sum(edge.events for edge in r.media.values())
    assert all(count > 0 for count in r.pairs.values())
    assert sum(row.taken for row in r.hosts.values()) == sum(row.lost for row in r.hosts.values()) == r.handovers
    assert sum(row.stints for row in r.hosts.values()) == len(r.media) + r.handovers
    starts = r.starts()
    for worker, row in r.hosts.items():
        assert row.stints == starts.get(worker, 0) + row.taken
        assert r.media_of(worker) <= row.stints <= row.events
        assert sum(row.by_class.values()) == row.events and all(row.by_class.values())
    assert sum(count for held in r.holding().values() for count in held.values()) == len(r.media)
    assert set(starts) <= set(r.hosts) and set(r.holding()) <= set(r.hosts)
    assert {mid for mid, _ in r.pairs} == set(r.media) and {w for _, w in r.pairs} == set(r.hosts)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("seed", SEEDS)
def test_conservation(seed, dialect):
    r = hosts_cpu(random_stream(seed), dialect)
    assert r.progress_events > 60 and r.handovers > 5 and r.rewinds > 0 and len(r.hosts) >= 5
    _check_laws(r)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_fold_corpus_numbers(dialect):
    r = hosts_cpu(corpus(), dialect)
    _check_laws(r)
    got = (r.frames, r.progress_events, r.progress_decode_errors, len(r.hosts), len(r.media), len(r.pairs), r.handovers,
           r.rewinds)
    assert got == {"protobufjs": (5711, 2865, 553, 77, 351, 629, 1865, 46),
                   "upb": (5711, 2452, 966, 4, 68, 260, 1740, 44)}[dialect]


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("seed", SEEDS)
def test_the_merge_law_at_every_frame_boundary(seed, dialect):
    data = random_stream(seed, 120)
    whole = hosts_cpu(data, dialect)
    cuts = list(_boundaries(data))
    assert len(cuts) == whole.frames + 1
    for cut in cuts:
        assert hosts_cpu(data[:cut], dialect).merge(hosts_cpu(data[cut:], dialect)) == whole


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_merge_law_on_the_stitch_stream_and_the_corpus(dialect):
    data = stitch_stream()
    whole = hosts_cpu(data, dialect)
    for cut in _boundaries(data):
        assert hosts_cpu(data[:cut], dialect).merge(hosts_cpu(data[cut:], dialect)) == whole
    data = corpus()
    whole = hosts_cpu(data, dialect)
    cuts = list(_boundaries(data))
    for cut in cuts[::701]:
        a, b = hosts_cpu(data[:cut], dialect), hosts_cpu(data[cut:], dialect)
        before = (a.to_json(True), b.to_json(True))
        assert a.merge(b) == whole
        assert (a.to_json(True), b.to_json(True)) == before  # neither operand changes


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_merge_is_associative(dialect):
    data = random_stream(2)
    cuts = list(_boundaries(data))
    whole = hosts_cpu(data, dialect)
    for i, j in ((10, 11), (40, 120), (1, len(cuts) - 2), (77, 78), (0, 50), (50, len(cuts) - 1)):
        a, b, c = (hosts_cpu(data[x:y], dialect) for x, y in ((0, cuts[i]), (cuts[i], cuts[j]), (cuts[j], len(data))))
        assert a.merge(b).merge(c) == a.merge(b.merge(c)) == whole
    assert HostReport().merge(whole) == whole == whole.merge(HostReport())


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("seed", SEEDS)
def test_one_constant_host(seed, dialect):
    data = one_worker(random_stream(seed))
    r = hosts_cpu(data, dialect)
    assert list(r.hosts) == ["only"] and r.handovers == 0
    row = r.hosts["only"]
    assert row.stints == len(r.media) == r.media_of("only") and row.taken == row.lost == 0
    if dialect == "protobufjs":  # under upb a host that was no UTF-8 decodes now
        before = hosts_cpu(random_stream(seed), dialect)
        assert (r.progress_events, set(r.media)) == (before.progress_events, set(before.media))
    _check_laws(r)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("stream", [lambda: random_stream(1), lambda: random_stream(3), corpus],
                         ids=["r1", "r3", "corpus"])
def test_against_the_fold(stream, dialect):
    data = stream()
    r, fold = hosts_cpu(data, dialect), replay.fold_cpu(data, dialect)
    assert r.frames == fold.frames and r.progress_decode_errors == fold.progress_decode_errors
    assert {mid: edge.events for mid, edge in r.media.items()} == \
        {mid: m.progress_events for mid, m in fold.media.items() if m.progress_events}
    names = replay.status_names()
    by_class = {}
    for row in r.hosts.values():
        for cls, count in row.by_class.items():
            by_class[cls] = by_class.get(cls, 0) + count
    assert by_class.pop(UNKNOWN, 0) == fold.progress_unknown_status
    assert {names[cls].lower(): count for cls, count in by_class.items()} == fold.progress_updates


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("shards", [1, 3, 8])
def test_the_shard_law(shards, dialect):
    data = corpus() if shards == 3 else random_stream(2)
    whole = hosts_cpu(data, dialect)
    sharded = shard.shard_cpu(data, shard.Policy(shards), dialect)
    parts = [hosts_cpu(part, dialect) for part in sharded.data]
    seen = set()
    for part in parts:
        assert not seen & set(part.media)  # a media lives in one shard
        seen |= set(part.media)
    orders = itertools.islice(itertools.permutations(range(shards)), 6)
    for order in orders:
        total = HostReport()
        for k in order:
            total = total.merge(parts[k])
        assert total.hosts == whole.hosts and total.pairs == whole.pairs
        assert total.progress_events == whole.progress_events
        assert total.progress_decode_errors == whole.progress_decode_errors
        assert {mid: (e.events, e.first[1:], e.last[1:]) for mid, e in total.media.items()} == \
            {mid: (e.events, e.first[1:], e.last[1:]) for mid, e in whole.media.items()}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_json_round_trip(dialect):
    for data in (random_stream(1), corpus(), b""):
        r = hosts_cpu(data, dialect)
        full = json.loads(json.dumps(r.to_json(per_media=True)))
        assert HostReport.from_json(full) == r
        short = r.to_json()
        assert "media" not in short and {k: v for k, v in full.items() if k != "media"} == json.loads(json.dumps(short))
        assert short["host_count"] == len(r.hosts) and short["media_count"] == len(r.media)
        assert short["handovers"] == r.handovers and short["rewinds"] == r.rewinds
        assert list(short["hosts"]) == sorted(r.hosts)
        for worker, row in short["hosts"].items():
            assert row["media"] == r.media_of(worker) and sum(row["by_status"].values()) == row["events"]
        assert sum(v for row in short["hosts"].values() for v in row["holding"].values()) == len(r.media)
        with pytest.raises(ValueError):
            HostReport.from_json(short)  # no per-media rows: not a whole result
    names = hosts_cpu(random_stream(1), dialect).to_json()["hosts"]
    classes = {k for row in names.values() for k in row["by_status"]}
    assert "unknown" in classes and classes - {"unknown"} <= set(replay.status_names().values())
    bad = hosts_cpu(random_stream(1), dialect).to_json(True)
    bad["hosts"]["node-a"]["by_status"]["NO_SUCH"] = 1
    with pytest.raises(ValueError):
        HostReport.from_json(bad)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_hosts_file_in_chunks_equals_the_whole(dialect, tmp_path):
    data = random_stream(3)
    want = hosts_cpu(data, dialect)
    for chunk_bytes in (1, 64, 1000, 1 << 20):  # 1: one frame per chunk
        assert hosts_file(io.BytesIO(data), dialect=dialect, chunk_bytes=chunk_bytes) == (want, 0)
    whole = corpus()
    assert len(whole) > 7 * 30_000
    assert hosts_file(io.BytesIO(whole), dialect=dialect, chunk_bytes=30_000) == (hosts_cpu(whole, dialect), 0)
    path = tmp_path / "capture.bin"
    path.write_bytes(data)
    assert hosts_file(str(path), "cpu", dialect) == (want, 0)
    assert hosts_file(io.BytesIO(b"")) == (HostReport(), 0)
    with pytest.raises(ValueError):
        hosts_file(io.BytesIO(data[:-1]), chunk_bytes=64)
    with pytest.raises(ValueError):
        hosts_file(io.BytesIO(data), dialect="proto2")


def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_cli_on_the_cpu(tmp_path):
    data = random_stream(1)
    path = tmp_path / "capture.bin"
    path.write_bytes(data)
    want = hosts_cpu(data)
    r = _cli("hosts", str(path), "--device", "cpu", "--chunk-bytes", "200", "--per-media")
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out.pop("host_frames") == 0
    assert out == json.loads(json.dumps(want.to_json(per_media=True))) and HostReport.from_json(out) == want
    r = _cli("hosts", "--dialect", "upb", stdin=data)  # stdin, default device, no rows
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out.pop("host_frames") == 0 and "media" not in out
    assert out == json.loads(json.dumps(hosts_cpu(data, "upb").to_json()))
    r = _cli("hosts", stdin=data[:-1])  # a broken stream
    assert r.returncode == 1 and b"beholder: " in r.stderr and not r.stdout
    r = _cli("hosts", str(path), "--dialect", "proto2")
    assert r.returncode == 2 and not r.stdout


def test_cli_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    path = tmp_path / "capture.bin"
    path.write_bytes(random_stream(1))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["hosts", str(path), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device gpu is not available" in out.err and "--device cpu" in out.err and not out.out


def test_a_stint_that_resumes():
    """a a b a: worker a has one media and two stints."""
    r = hosts_cpu(worker_stream([(b"m", b"a", 2, 1), (b"m", b"a", 2, 2), (b"m", b"b", 2, 3), (b"m", b"a", 2, 4)]))
    assert r.hosts == {"a": HostRow(3, {2: 3}, 2, 1, 1, 0), "b": HostRow(1, {2: 1}, 1, 1, 1, 0)}
    assert r.media_of("a") == 1 and r.media_of("b") == 1 and r.pairs == {("m", "a"): 3, ("m", "b"): 1}
    assert r.media == {"m": MediaEdge(4, (0, "a", 2, 1), (3, "a", 2, 4))}
    assert r.handovers == 2 and r.rewinds == 0
    assert r.holding() == {"a": {2: 1}} and r.starts() == {"a": 1}
    _check_laws(r)


def test_rewinds():
    # the progress falls under one status and one worker: a rewind
    r = hosts_cpu(worker_stream([(b"m", b"a", 2, 40), (b"m", b"a", 2, 39), (b"m", b"a", 2, 39), (b"m", b"a", 2, -1)]))
    assert r.rewinds == 2 and r.hosts["a"] == HostRow(4, {2: 4}, 1, 0, 0, 2)
    # none because the status changed, the unknown numbers included: the raw status counts, not its class
    r = hosts_cpu(worker_stream([(b"m", b"a", 2, 100), (b"m", b"a", 3, 0), (b"m", b"a", 6, -5), (b"m", b"a", 64, -9)]))
    assert r.rewinds == 0 and r.hosts["a"] == HostRow(4, {2: 1, 3: 1, UNKNOWN: 2}, 1, 0, 0, 0)
    # none across a handover
    r = hosts_cpu(worker_stream([(b"m", b"a", 2, 90), (b"m", b"b", 2, 10), (b"m", b"a", 2, 5)]))
    assert r.rewinds == 0 and r.handovers == 2 and r.hosts["a"].stints == 2
    # another media in between does not hide one
    r = hosts_cpu(worker_stream([(b"m", b"a", 2, 90), (b"n", b"a", 2, 10), (b"m", b"a", 2, 5)]))
    assert r.rewinds == 1 and r.hosts["a"] == HostRow(3, {2: 3}, 2, 0, 0, 1)


def test_hosts_that_are_no_utf8():
    data = worker_stream([(b"m", b"\xff", 2, 1), (b"m", b"\xfe", 2, 2), (b"m", None, 2, 3), (b"m", b"", 2, 4)])
    r = hosts_cpu(data, "protobufjs")
    assert r.hosts == {"�": HostRow(2, {2: 2}, 1, 0, 1, 0), "": HostRow(2, {2: 2}, 1, 1, 0, 0)}
    assert r.progress_decode_errors == 0 and r.handovers == 1
    r = hosts_cpu(data, "upb")
    assert r.hosts == {"": HostRow(2, {2: 2}, 1, 0, 0, 0)} and r.progress_decode_errors == 2
    assert r.media == {"m": MediaEdge(2, (2, "", 2, 3), (3, "", 2, 4))}


def test_other_frames_count_in_frames_only():
    data = frames([(STATUS_ID, body(b"m", 1)), (9, progress_body(b"m", 2, 5, b"a")), (PROGRESS_ID, b"\x2e"),
                   (PROGRESS_ID, progress_body(b"m", 2, 5, b"a"))])
    r = hosts_cpu(data)
    assert (r.frames, r.progress_events, r.progress_decode_errors) == (4, 1, 1)
    assert r.media == {"m": MediaEdge(1, (3, "a", 2, 5), (3, "a", 2, 5))}
    assert hosts_cpu(b"") == HostReport()
    with pytest.raises(ValueError):
        hosts_cpu(data[:-1])
    with pytest.raises(ValueError):
        hosts_cpu(data, "proto2")


def test_course_of_is_the_rule():
    names = replay.status_names()
    edge, rows, pairs = course_of([(3, "a", 2, 5), (7, "b", 9, 1), (8, "b", 9, 0)], names)
    assert edge == MediaEdge(3, (3, "a", 2, 5), (8, "b", 9, 0)) and pairs == {"a": 1, "b": 2}
    assert rows == {"a": HostRow(1, {class_of(2, names): 1}, 1, 0, 1, 0),
                    "b": HostRow(2, {class_of(9, names): 2}, 1, 1, 0, 1)}
    r = HostReport()
    r.add_course("m", edge, rows, pairs)
    r.add_course("n", *course_of([(1, "a", 2, 5)], names))
    r.add_course("m", None, rows, pairs, sign=-1)  # taken out again: what is left is n's
    assert r == HostReport(0, 1, 0, {"a": HostRow(1, {2: 1}, 1, 0, 0, 0)}, {("n", "a"): 1},
                           {"n": MediaEdge(1, (1, "a", 2, 5), (1, "a", 2, 5))})
