"""``shard`` on the CPU: the definition (beholder_amd/shard.py), its laws, what it means for the fold,
the coalesce and a ``Service`` run, and the command."""
from __future__ import annotations

import asyncio
import functools
import io
import json
import subprocess
import sys

import pytest

from beholder_amd import coalesce as co, ops, replay, shard as sh
from beholder_amd.bench.generator import Workload, bench_config
from beholder_amd.ops import frames
from beholder_amd.shard import DROP, Policy, Sharded, shard_cpu, shard_of
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames
from shard_cases import POLICIES, SHARD_COUNTS, corpus, mixed_stream, pairs_stream, policy_id
from telemetry_corpus import body as _body

FFFD = "\ufffd"
STREAMS = {"mixed": mixed_stream, "corpus": corpus}


@functools.lru_cache(maxsize=None)
def _fold(dialect: str) -> replay.Summary:
    return replay.fold_cpu(corpus(), dialect)


def _frame_list(data: bytes) -> list:
    return [ops.frame(topic, body) for topic, body in iter_frames(data)]


def _media(dialect: str):
    """``media(topic, body)``: the decoded id, or None for a frame that is no decoded event."""
    from beholder_amd.models import proto
    decoders = {STATUS_ID: ops.codec_for(proto.load("api.TelemetryStatus"), dialect).decode,
                PROGRESS_ID: ops.codec_for(proto.load("api.TelemetryProgress"), dialect).decode}

    def media(topic, body):
        try:
            return decoders[topic](body).mediaId if topic in decoders else None
        except proto.DecodeError:
            return None
    return media


# ---- the hash and the policy ------------------------------------------------------------------------

def test_shard_of_is_the_formula_over_the_folds_hash():
    np = pytest.importorskip("numpy")  # noqa: F841  gpu_fold imports it
    from beholder_amd.ops import gpu_fold
    ids = ["", "m", "m-1", "é", FFFD, "メディア", "x" * 300] + [m.id for m in Workload(n_media=50, seed=1).media]
    for mid in ids:
        h = gpu_fold.hash64(mid.encode("utf-8"))
        assert sh.hash64(mid.encode("utf-8")) == h
        for n in SHARD_COUNTS:
            assert shard_of(mid, n) == ((h >> 32) * n) >> 32 and 0 <= shard_of(mid, n) < n
    assert {shard_of(mid, 1) for mid in ids} == {0}
    assert len({shard_of(mid, 256) for mid in ids}) > 40


def test_shard_of_depends_on_the_string_and_the_count_only():
    """The same id gets the same shard from any capture, topic, dialect or chunk."""
    a = frames([(STATUS_ID, _body(b"m-1", 1)), (9, b"x"), (PROGRESS_ID, _body(b"m-2", 2))])
    b = frames([(PROGRESS_ID, _body(b"m-2", 5)), (PROGRESS_ID, _body(b"m-1", 0))])
    for n in (2, 7, 256):
        for dialect in ops.DIALECTS:
            route = sh.route_of(Policy(n), dialect)
            for data in (a, b, b + a):
                for topic, body in iter_frames(data):
                    if topic in (STATUS_ID, PROGRESS_ID):
                        assert route(topic, body) == shard_of(body[2:5].decode(), n)


def test_the_policy_is_validated():
    assert Policy(4) == Policy(shards=4, undecoded="first")
    for bad in (0, -1, 257, 1 << 40):
        with pytest.raises(ValueError):
            Policy(bad)
        with pytest.raises(ValueError):
            shard_of("m", bad)
    for bad in ("4", 4.0, None, True):
        with pytest.raises(TypeError):
            Policy(bad)
        with pytest.raises(TypeError):
            shard_of("m", bad)
    with pytest.raises(ValueError):
        Policy(4, "keep")
    with pytest.raises(ValueError):
        Policy(4, "")
    with pytest.raises(TypeError):
        Policy(4, None)
    with pytest.raises(TypeError):
        Policy(4, 0)
    assert Policy(1).shards == 1 and Policy(256, "drop").undecoded == "drop"


def test_route_of_by_hand():
    route = sh.route_of(Policy(8))
    assert route(STATUS_ID, _body(b"m-1", 3)) == route(PROGRESS_ID, _body(b"m-1", 64)) == shard_of("m-1", 8)
    assert route(STATUS_ID, b"") == shard_of("", 8)  # an absent id is the empty string
    assert route(STATUS_ID, _body(b"\xff", 1)) == route(PROGRESS_ID, _body(b"\xfe", 1)) == shard_of(FFFD, 8)
    assert route(STATUS_ID, b"\x2e") == route(9, _body(b"m-1", 3)) == route(0, b"") == 0
    drop = sh.route_of(Policy(8, "drop"))
    assert drop(STATUS_ID, b"\x2e") is drop(9, _body(b"m-1", 3)) is DROP
    assert drop(STATUS_ID, _body(b"m-1", 3)) == shard_of("m-1", 8)
    upb = sh.route_of(Policy(8, "drop"), "upb")  # upb raises on invalid UTF-8: an error
    assert upb(STATUS_ID, _body(b"\xff", 1)) is DROP and upb(STATUS_ID, _body("é".encode(), 1)) == shard_of("é", 8)


def test_bad_arguments_raise():
    data = frames([(STATUS_ID, _body(b"m", 1))])
    with pytest.raises(ValueError):
        shard_cpu(data, Policy(2), dialect="proto2")
    with pytest.raises(ValueError):
        sh.route_of(Policy(2), "proto2")
    with pytest.raises(TypeError):
        sh.route_of(2)
    with pytest.raises(TypeError):
        shard_cpu(data, 2)
    with pytest.raises(ValueError):
        sh.shard_file(io.BytesIO(data), [io.BytesIO(), io.BytesIO()], Policy(2), dialect="proto2")
    with pytest.raises(ValueError):
        sh.shard_file(io.BytesIO(data), [io.BytesIO()], Policy(2))  # one file per shard
    with pytest.raises(ValueError):
        sh.shard_file(io.BytesIO(data), [io.BytesIO(), io.BytesIO()], Policy(2), indices_outs=[io.StringIO()])
    for broken in (data[:-1], data + b"\x01\x00", data + b"\x00\x00\x00\x00"):
        with pytest.raises(ValueError):
            shard_cpu(broken, Policy(2))
    with pytest.raises(ValueError):
        Sharded(2).merge(Sharded(3))
    assert shard_cpu(b"", Policy(3)) == Sharded(3) == Sharded(3, [b""] * 3, [[], [], []], 0)


# ---- laws -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("stream", sorted(STREAMS))
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_shards_are_a_partition_in_order_by_media(policy, stream, dialect):
    data = STREAMS[stream]()
    whole = _frame_list(data)
    events = list(iter_frames(data))
    got = shard_cpu(data, policy, dialect)
    assert got.shards == policy.shards == len(got.data) == len(got.indices) and got.frames == len(whole)
    media = _media(dialect)
    placed = {}
    for s, (part, indices) in enumerate(zip(got.data, got.indices)):
        assert indices == sorted(set(indices))  # ascending
        assert _frame_list(part) == [whole[i] for i in indices]  # byte for byte
        for i in indices:
            assert i not in placed
            placed[i] = s
            mid = media(*events[i])
            assert s == (0 if mid is None else shard_of(mid, policy.shards)), (i, mid)
    undecoded = {i for i, e in enumerate(events) if media(*e) is None}
    assert undecoded and len(undecoded) < len(events)
    if policy.undecoded == "first":
        assert sorted(placed) == list(range(len(whole)))
        assert b"".join(whole[i] for i in sorted(placed)) == data  # merged by indices: the input again
    else:
        assert set(placed) == set(range(len(whole))) - undecoded  # exactly the non-decoded frames are missing


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_one_shard_taking_everything_is_the_identity(dialect):
    for data in (mixed_stream(), corpus()):
        got = shard_cpu(data, Policy(1), dialect)
        assert got.data == [data] and got.indices == [list(range(got.frames))]


@pytest.mark.parametrize("policy", [Policy(1), Policy(3), Policy(3, "drop"), Policy(256)], ids=policy_id)
def test_results_merge_at_every_frame_boundary(policy):
    data = mixed_stream()
    want = shard_cpu(data, policy)
    cut = 0
    for f in _frame_list(data):
        cut += len(f)
        assert shard_cpu(data[:cut], policy).merge(shard_cpu(data[cut:], policy)) == want
    assert Sharded(policy.shards).merge(want) == want == want.merge(Sharded(policy.shards))


def test_ids_that_differ_in_one_byte_spread_over_the_shards():
    got = shard_cpu(pairs_stream(), Policy(64))
    assert got.frames == 720 and sum(map(len, got.indices)) == 720
    assert sum(bool(i) for i in got.indices) > 40  # 120 ids over 64 shards
    for part in got.data:
        ids = {body[2:12] for _, body in iter_frames(part)}
        assert all(shard_of(mid.decode(), 64) == got.data.index(part) for mid in ids)


@pytest.mark.parametrize("chunk_bytes", [700, 1])
@pytest.mark.parametrize("policy", [Policy(3), Policy(7, "drop")], ids=policy_id)
def test_shard_file_in_small_chunks_equals_the_one_shot_result(policy, chunk_bytes):
    data = corpus() if chunk_bytes > 1 else mixed_stream()
    want = shard_cpu(data, policy)
    outs = [io.BytesIO() for _ in range(policy.shards)]
    indices = [io.StringIO() for _ in range(policy.shards)]
    counts = sh.shard_file(io.BytesIO(data), outs, policy, chunk_bytes=chunk_bytes, indices_outs=indices)
    assert [o.getvalue() for o in outs] == want.data
    assert [[int(line) for line in i.getvalue().split()] for i in indices] == want.indices
    assert counts == {"frames": want.frames, "kept": sum(map(len, want.indices)),
                      "kept_bytes": sum(map(len, want.data)), "host_frames": 0,
                      "per_shard": [{"frames": len(i), "bytes": len(d)} for i, d in zip(want.indices, want.data)]}
    assert counts["kept"] == want.frames if policy.undecoded == "first" else counts["kept"] < want.frames


def test_a_stream_that_ends_inside_a_frame_leaves_whole_frames_only():
    data = Workload(n_media=4, seed=5).framed(50)
    outs = [io.BytesIO() for _ in range(2)]
    with pytest.raises(ValueError, match="truncated"):
        sh.shard_file(io.BytesIO(data[:-3]), outs, Policy(2), chunk_bytes=700)
    want = shard_cpu(data, Policy(2))
    written = [o.getvalue() for o in outs]
    assert any(written) and all(w == d[:len(w)] for w, d in zip(written, want.data))
    for w in written:
        list(iter_frames(w))  # whole frames


# ---- against the fold, the coalesce and the service -------------------------------------------------

@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("shards", [1, 7, 256])
def test_against_the_fold(shards, dialect):
    fold = _fold(dialect)
    got = shard_cpu(corpus(), Policy(shards), dialect)
    subs = [replay.fold_cpu(part, dialect) for part in got.data]
    assert sum(len(sub.media) for sub in subs) == len(fold.media) > 60  # each media in exactly one shard
    for mid, want in fold.media.items():
        s = shard_of(mid, shards)
        mine = subs[s].media[mid]
        assert (mine.status_events, mine.progress_events, mine.progress_counted, mine.last_status) == \
            (want.status_events, want.progress_events, want.progress_counted, want.last_status), mid
        if want.last_status_index is None:
            assert mine.last_status_index is None
        else:
            assert got.indices[s][mine.last_status_index] == want.last_status_index, mid
    first = subs[0]
    assert (first.status_decode_errors, first.progress_decode_errors, first.other_topic) == \
        (fold.status_decode_errors, fold.progress_decode_errors, fold.other_topic)
    assert fold.status_decode_errors and fold.progress_decode_errors and fold.other_topic
    for sub in subs[1:]:
        assert (sub.status_decode_errors, sub.progress_decode_errors, sub.other_topic) == (0, 0, 0)
    assert sum(sub.frames for sub in subs) == fold.frames


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("shards", [2, 7, 64])
def test_coalescing_a_shard_is_that_shard_of_the_coalesce(shards, dialect):
    data = corpus()
    parts = shard_cpu(data, Policy(shards), dialect)
    of_the_cut = shard_cpu(co.coalesce_cpu(data, dialect=dialect).data, Policy(shards), dialect)
    for k in range(shards):
        assert co.coalesce_cpu(parts.data[k], dialect=dialect).data == of_the_cut.data[k], k
    assert sum(map(len, of_the_cut.indices)) < parts.frames


def test_the_service_ends_on_the_same_statuses_in_any_shard_order():
    """Set up like test_coalesce.test_the_service_ends_on_the_same_statuses: the store's status column
    after the shards, replayed one after another in either order, is what it is after the whole stream."""
    from beholder_amd.config import Config
    from beholder_amd.service import Service
    from beholder_amd.sinks import RecordingHttpClient
    from beholder_amd.store import MemoryStore
    from beholder_amd.transport.ingest import BytesSource
    from beholder_amd.utils.log import Logger, MemoryStream

    w = Workload(n_media=16, seed=3, unknown_media_fraction=0.1)
    data = w.framed(3000)
    parts = shard_cpu(data, Policy(4))
    assert parts.frames == 3000 and all(parts.indices)  # 16 media and some unknown ones: no shard is empty

    def run(streams: list) -> dict:
        store = MemoryStore(w.media)

        async def go(stream):
            svc = Service(Config.from_dict(bench_config()), source=BytesSource(stream), store=store,
                          http=RecordingHttpClient(), logger=Logger(stream=MemoryStream()), serve_metrics=False)
            await svc.init()
            await svc.run()
            await svc.close()
        for stream in streams:
            asyncio.run(go(stream))
        return {mid: row.status for mid, row in store.snapshot().items()}

    whole = run([data])
    assert run(parts.data) == whole
    assert run([parts.data[k] for k in (2, 0, 3, 1)]) == whole
    assert whole != {m.id: m.status for m in w.media}, "the stream changes statuses"


def test_the_shards_are_balanced():
    """9,971 distinct media over 8 shards: every shard holds within 10% of the mean (0.964-1.047 of
    it by the formula)."""
    data = Workload(n_media=10000, seed=9).framed(60000)
    got = shard_cpu(data, Policy(8))
    media = _media("protobufjs")
    per_shard = [len({media(topic, body) for topic, body in iter_frames(part)}) for part in got.data]
    mean = sum(per_shard) / 8
    assert sum(per_shard) > 9000
    assert all(0.9 * mean <= count <= 1.1 * mean for count in per_shard), per_shard


# ---- the command ------------------------------------------------------------------------------------

def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_cli_shard_writes_every_shard_and_the_chain_stays_closed(tmp_path):
    data = Workload(n_media=8, seed=5).framed(400)
    capture = tmp_path / "capture.bin"
    capture.write_bytes(data)
    r = _cli("shard", str(capture), "--shards", "3", "-o", str(tmp_path / "part-{}.bin"),
             "--indices", str(tmp_path / "part-{}.txt"), "--chunk-bytes", "700")
    assert r.returncode == 0 and not r.stdout, r.stderr
    want = shard_cpu(data, Policy(3))
    assert [(tmp_path / f"part-{k}.bin").read_bytes() for k in range(3)] == want.data
    assert [[int(line) for line in (tmp_path / f"part-{k}.txt").read_text().split()] for k in range(3)] == want.indices
    assert json.loads(r.stderr) == {
        "frames": 400, "kept": 400, "kept_bytes": len(data), "host_frames": 0,
        "per_shard": [{"frames": len(i), "bytes": len(d)} for i, d in zip(want.indices, want.data)]}
    whole = replay.fold_cpu(data)
    seen = {}
    for k in range(3):  # shard -> summarise
        r = _cli("summarise", str(tmp_path / f"part-{k}.bin"))
        assert r.returncode == 0, r.stderr
        sub = replay.Summary.from_json(json.loads(r.stdout)["summary"])
        assert not set(sub.media) & set(seen)
        seen.update({m: f.last_status for m, f in sub.media.items()})
    assert seen == {m: f.last_status for m, f in whole.media.items()}
    r = _cli("coalesce", str(tmp_path / "part-1.bin"), "-o", "-")  # shard -> coalesce
    assert r.returncode == 0 and r.stdout == co.coalesce_cpu(want.data[1]).data


def test_cli_shard_gives_an_empty_shard_an_empty_file(tmp_path):
    data = frames([(STATUS_ID, _body(b"m", k)) for k in range(5)])
    r = _cli("shard", "--shards", "16", "-o", str(tmp_path / "s{}"), "--undecoded", "drop", "--dialect", "upb",
             stdin=data)
    assert r.returncode == 0, r.stderr
    sizes = [(tmp_path / f"s{k}").stat().st_size for k in range(16)]
    assert sizes[shard_of("m", 16)] == len(data) and sum(sizes) == len(data)
    assert json.loads(r.stderr)["per_shard"][shard_of("m", 16)] == {"frames": 5, "bytes": len(data)}


def test_cli_shard_usage_errors_exit_2(tmp_path):
    data = Workload(n_media=4, seed=5).framed(20)
    assert _cli("shard", "--shards", "2", "-o", str(tmp_path / "out.bin"), stdin=data).returncode == 2  # no {}
    assert _cli("shard", "--shards", "2", "-o", "-", stdin=data).returncode == 2
    assert _cli("shard", "--shards", "2", "-o", str(tmp_path / "a{}"), "--indices", str(tmp_path / "i"),
                stdin=data).returncode == 2
    for bad in ("0", "257", "-1", "two"):
        assert _cli("shard", "--shards", bad, "-o", str(tmp_path / "b{}"), stdin=data).returncode == 2
    assert _cli("shard", "-o", str(tmp_path / "c{}"), stdin=data).returncode == 2  # --shards is required
    assert _cli("shard", "--shards", "2", "-o", str(tmp_path / "d{}"), "--undecoded", "keep", stdin=data).returncode == 2
    assert not list(tmp_path.iterdir())


def test_cli_shard_truncated_input_leaves_whole_frames_only(tmp_path):
    data = Workload(n_media=4, seed=5).framed(50)
    r = _cli("shard", "--shards", "2", "-o", str(tmp_path / "p{}"), "--chunk-bytes", "700", stdin=data[:-3])
    assert r.returncode == 1 and b"truncated" in r.stderr
    want = shard_cpu(data, Policy(2))
    for path in tmp_path.iterdir():
        written = path.read_bytes()
        assert written == want.data[int(path.name[1:])][:len(written)]
        list(iter_frames(written))
    # a run that fails before it writes leaves no file
    r = _cli("shard", "--shards", "2", "-o", str(tmp_path / "q{}"), stdin=data[:3])
    assert r.returncode == 1 and not list(tmp_path.glob("q*"))


def test_cli_shard_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    from beholder_amd.ops import hip_lib
    path, out = tmp_path / "capture.bin", tmp_path / "cut-{}.bin"
    path.write_bytes(Workload(n_media=2, seed=5).framed(10))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["shard", str(path), "--shards", "2", "-o", str(out), "--device", "gpu"]) != 0
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "no GPU" in err.err and not err.out and not list(tmp_path.glob("cut-*"))
    # and with a device but no library
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "libbeholder_hip.so"))
    monkeypatch.setattr(hip_lib, "_lib", None)
    assert cli.main(["shard", str(path), "--shards", "2", "-o", str(out), "--device", "gpu"]) != 0
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "missing" in err.err and not err.out and not list(tmp_path.glob("cut-*"))
