"""``dedupe`` on the CPU: the definition (beholder_amd/dedupe.py), its laws, what it means for the
coalesce, the fold and a ``Service`` run, and the command."""
from __future__ import annotations

import asyncio
import functools
import io
import json
import subprocess
import sys

import pytest

from beholder_amd import coalesce as co, dedupe as dd, ops, replay
from beholder_amd.bench.generator import Workload, bench_config
from beholder_amd.dedupe import Deduped, Policy, dedupe_cpu
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames
from dedupe_cases import POLICIES, aligned_stream, corpus, edge_stream, mixed_stream, policy_id, three_statuses
from telemetry_corpus import body as _body

STREAMS = {"mixed": mixed_stream, "corpus": corpus, "edge": edge_stream, "aligned": aligned_stream}


def _frame_list(data: bytes) -> list:
    return [ops.frame(topic, body) for topic, body in iter_frames(data)]


@functools.lru_cache(maxsize=None)
def _fold(data: bytes) -> dict:
    return {mid: f.last_status for mid, f in replay.fold_cpu(data).media.items()}


# ---- the policy and the arguments -------------------------------------------------------------------

def test_the_policy_is_validated():
    assert Policy() == Policy(keep="last", topics=None)
    assert Policy("first", {1, 2}) == Policy("first", frozenset({2, 1})) == Policy("first", [1, 2, 2])
    assert hash(Policy(topics={7})) == hash(Policy(topics=(7,)))
    for bad in ("", "all", "LAST", "newest"):
        with pytest.raises(ValueError):
            Policy(bad)
    for bad in (None, 0, b"last", True):
        with pytest.raises(TypeError):
            Policy(bad)
    for bad in ({-1}, {256}, {1, 1 << 40}):
        with pytest.raises(ValueError):
            Policy(topics=bad)
    for bad in (1, "status", b"\x01", {"1"}, {1.0}, {True}, {None}):
        with pytest.raises(TypeError):
            Policy(topics=bad)
    assert Policy(topics=set()).topics == frozenset()  # nothing takes part: the identity
    assert Policy(topics={0, 255}).takes_part(255) and not Policy(topics={0, 255}).takes_part(1)


def test_bad_arguments_raise():
    data = frames([(STATUS_ID, _body(b"m", 1))] * 2)
    with pytest.raises(TypeError):
        dedupe_cpu(data, "last")
    with pytest.raises(TypeError):
        dd.dedupe_file(io.BytesIO(data), io.BytesIO(), "last")
    with pytest.raises(ValueError):
        dd.dedupe_file(io.BytesIO(data), io.BytesIO(), Policy(), chunk_bytes=0)
    for broken in (data[:-1], data + b"\x01\x00", data + b"\x00\x00\x00\x00"):
        with pytest.raises(ValueError):
            dedupe_cpu(broken)
    for policy in POLICIES:
        assert dedupe_cpu(b"", policy) == Deduped(keep=policy.keep, topics=policy.topics)
        assert dedupe_cpu(b"", policy) == Deduped(b"", [], 0, policy.keep, policy.topics)


def test_by_hand():
    a, b, c = (STATUS_ID, b"a"), (STATUS_ID, b"b"), (PROGRESS_ID, b"a")
    data = frames([a, b, a, c, b, a, c])
    assert dedupe_cpu(data).indices == [4, 5, 6] and dedupe_cpu(data).data == frames([b, a, c])
    assert dedupe_cpu(data, Policy("first")).indices == [0, 1, 3]
    assert dedupe_cpu(data, Policy("first")).data == frames([a, b, c])
    assert dedupe_cpu(data, Policy(topics={PROGRESS_ID})).indices == [0, 1, 2, 4, 5, 6]
    assert dedupe_cpu(data, Policy("first", {PROGRESS_ID})).indices == [0, 1, 2, 3, 4, 5]
    assert dedupe_cpu(data, Policy(topics=set())).data == data
    # nothing is decoded: two encodings of one event are two contents
    one, other = b"\x0a\x01m\x10\x01", b"\x10\x01\x0a\x01m"
    assert dedupe_cpu(frames([(STATUS_ID, one), (STATUS_ID, other), (STATUS_ID, one)])).indices == [1, 2]


# ---- laws -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stream", sorted(STREAMS))
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_result_is_the_input_without_its_repeats(policy, stream):
    data = STREAMS[stream]()
    whole = _frame_list(data)
    got = dedupe_cpu(data, policy)
    assert got.frames == len(whole) and got.keep == policy.keep and got.topics == policy.topics
    assert got.indices == sorted(set(got.indices))  # ascending
    kept = _frame_list(got.data)
    assert kept == [whole[i] for i in got.indices]  # every kept frame is an input frame, in order, byte for byte
    taking_part = [f for f in kept if policy.takes_part(f[4])]
    assert len(taking_part) == len(set(taking_part))  # no two of them share a content
    assert set(kept) == set(whole)  # every content of the input is still there
    assert dedupe_cpu(got.data, policy).data == got.data  # idempotent
    assert dedupe_cpu(got.data, policy).indices == list(range(len(kept)))
    # the kept index of every content is its first or its last occurrence
    first, last = {}, {}
    for i, f in enumerate(whole):
        first.setdefault(f, i)
        last[f] = i
    where = last if policy.keep == "last" else first
    assert got.indices == [i for i, f in enumerate(whole) if not policy.takes_part(f[4]) or where[f] == i]
    repeats = len(whole) - len(got.indices)
    assert repeats == sum(policy.takes_part(f[4]) for f in whole) - len(taking_part)
    if policy.topics is None:
        assert repeats > 0


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_unselected_topics_pass_through_untouched(policy):
    """Undecodable frames and other topic bytes, each twice: those of a topic that is not selected
    all stay, in place."""
    events = [(STATUS_ID, b"\x2e"), (PROGRESS_ID, b"\x2e"), (9, _body(b"m", 1)), (0, b""), (255, b"\xff\xff"),
              (7, b"\x2e"), (STATUS_ID, _body(b"m", 1)), (PROGRESS_ID, _body(b"m", 1))] * 2
    data = frames(events)
    got = dedupe_cpu(data, policy)
    outside = [i for i, (topic, _) in enumerate(events) if not policy.takes_part(topic)]
    assert set(outside) <= set(got.indices)
    inside = len(events) - len(outside)
    assert len(got.indices) == len(outside) + inside // 2
    if policy.topics is None:
        assert got.indices == list(range(8, 16) if policy.keep == "last" else range(8))


@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_results_merge_at_every_frame_boundary(policy):
    data = mixed_stream()
    want = dedupe_cpu(data, policy)
    cut = 0
    for f in _frame_list(data):
        cut += len(f)
        assert dedupe_cpu(data[:cut], policy).merge(dedupe_cpu(data[cut:], policy)) == want
    empty = dedupe_cpu(b"", policy)
    assert empty.merge(want) == want == want.merge(empty)
    assert want.frames > 90
    if policy.topics != {7}:
        assert len(want.indices) < want.frames


def test_mismatched_merges_raise():
    data = mixed_stream()
    for a, b in ((Policy(), Policy("first")), (Policy(), Policy(topics={STATUS_ID})),
                 (Policy(topics={STATUS_ID}), Policy(topics={PROGRESS_ID})),
                 (Policy("first", {7}), Policy("last", {7}))):
        with pytest.raises(ValueError):
            dedupe_cpu(data, a).merge(dedupe_cpu(data, b))
        with pytest.raises(ValueError):
            dedupe_cpu(data, b).merge(dedupe_cpu(b"", a))


# ---- against the coalesce, the fold and the service -------------------------------------------------

@pytest.mark.parametrize("twice", [False, True], ids=["corpus", "corpus-twice"])
def test_last_keeps_what_the_coalesce_and_the_fold_need(twice):
    """The two laws that make ``last`` the default: coalescing the deduped stream gives what
    coalescing the input gives, and the fold ends on the same status for every media."""
    data = corpus() * 2 if twice else corpus()
    got = dedupe_cpu(data)
    assert (got.frames, len(got.indices)) == ((11422, 5008) if twice else (5711, 5008))
    policy = co.Policy(undecoded="drop")
    assert co.coalesce_cpu(got.data, policy).data == co.coalesce_cpu(data, policy).data
    assert _fold(got.data) == _fold(data) and len(_fold(data)) > 60


def test_first_breaks_both_laws_on_the_corpus():
    data = corpus()
    got = dedupe_cpu(data, Policy("first"))
    assert len(got.indices) == 5008
    policy = co.Policy(undecoded="drop")
    assert co.coalesce_cpu(got.data, policy).data != co.coalesce_cpu(data, policy).data
    assert _fold(got.data) != _fold(data)


def test_first_ends_queued_errored_queued_on_the_wrong_status():
    """The documented hazard, pinned: ``first`` turns QUEUED, ERRORED, QUEUED into QUEUED, ERRORED."""
    data = three_statuses()
    names = replay.status_names()
    first, last = dedupe_cpu(data, Policy("first")), dedupe_cpu(data)
    assert first.indices == [0, 1] and last.indices == [1, 2]
    assert names[_fold(data)["m-1"]] == names[_fold(last.data)["m-1"]] == "QUEUED"
    assert names[_fold(first.data)["m-1"]] == "ERRORED"


def test_the_service_ends_on_the_same_statuses():
    """Set up like test_shard.test_the_service_ends_on_the_same_statuses_in_any_shard_order: the
    store's status column after the deduped stream is what it is after the whole stream, which
    holds a redelivered stretch and is followed by a copy of itself."""
    from beholder_amd.config import Config
    from beholder_amd.service import Service
    from beholder_amd.sinks import RecordingHttpClient
    from beholder_amd.store import MemoryStore
    from beholder_amd.transport.ingest import BytesSource
    from beholder_amd.utils.log import Logger, MemoryStream

    w = Workload(n_media=16, seed=3, unknown_media_fraction=0.1)
    pieces = _frame_list(w.framed(1500))
    data = b"".join(pieces[:900] + pieces[600:] + pieces)  # a redelivery, then the dump published again
    got = dedupe_cpu(data)
    assert got.frames == 3300 and len(got.indices) <= 1500

    def run(stream: bytes) -> dict:
        store = MemoryStore(w.media)

        async def go():
            svc = Service(Config.from_dict(bench_config()), source=BytesSource(stream), store=store,
                          http=RecordingHttpClient(), logger=Logger(stream=MemoryStream()), serve_metrics=False)
            await svc.init()
            await svc.run()
            await svc.close()
        asyncio.run(go())
        return {mid: row.status for mid, row in store.snapshot().items()}

    whole = run(data)
    assert run(got.data) == whole
    assert whole != {m.id: m.status for m in w.media}, "the stream changes statuses"


# ---- dedupe_file ------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk_bytes", [700, 1])
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_dedupe_file_in_small_chunks_equals_the_one_shot_result(policy, chunk_bytes):
    data = corpus() + b"".join(_frame_list(corpus())[:1500]) if chunk_bytes > 1 else mixed_stream()
    want = dedupe_cpu(data, policy)
    for size in (chunk_bytes, 1 << 30):  # many chunks, and one
        out, indices = io.BytesIO(), io.StringIO()
        counts = dd.dedupe_file(io.BytesIO(data), out, policy, chunk_bytes=size, indices_out=indices)
        assert out.getvalue() == want.data
        assert [int(line) for line in indices.getvalue().split()] == want.indices
        assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                          "duplicates": want.frames - len(want.indices), "host_frames": 0}


def test_dedupe_file_of_one_chunk_builds_no_host_state(monkeypatch):
    def no_state(*a, **kw):
        raise AssertionError("one chunk needs no cross-chunk state")
    monkeypatch.setattr(dd, "_kept", no_state)
    data = corpus()
    for policy in (Policy(), Policy("first")):
        out = io.BytesIO()
        assert dd.dedupe_file(io.BytesIO(data), out, policy)["kept"] == 5008
        assert out.getvalue() == dedupe_cpu(data, policy).data
        with pytest.raises(AssertionError):
            dd.dedupe_file(io.BytesIO(data), io.BytesIO(), policy, chunk_bytes=30_000)


def test_the_cross_chunk_state_is_exact_when_its_numbers_collide(monkeypatch):
    """The 64-bit number only pre-filters: with every number equal, the bytes still decide."""
    kept = dd._kept
    monkeypatch.setattr(dd, "_kept",
                        lambda part, policy: ((f, i, None if n is None else 5) for f, i, n in kept(part, policy)))
    data = mixed_stream()
    for policy in POLICIES:
        out = io.BytesIO()
        dd.dedupe_file(io.BytesIO(data), out, policy, chunk_bytes=1)
        assert out.getvalue() == dedupe_cpu(data, policy).data


def test_many_repeats_across_chunks_keep_one_copy_per_content():
    """16 media repeated over and over: the tombstones are swept, and the state holds the distinct
    contents only."""
    data = Workload(n_media=16, seed=5).framed(600) * 12
    want = dedupe_cpu(data)
    out = io.BytesIO()
    counts = dd.dedupe_file(io.BytesIO(data), out, Policy(), chunk_bytes=2000)
    assert out.getvalue() == want.data and counts["kept"] == len(want.indices) <= 600 and counts["duplicates"] >= 6600


def test_a_stream_that_ends_inside_a_frame():
    data = Workload(n_media=4, seed=5).framed(50) * 2
    for chunk_bytes in (700, 1 << 30):
        out, indices = io.BytesIO(), io.StringIO()
        with pytest.raises(ValueError, match="truncated"):
            dd.dedupe_file(io.BytesIO(data[:-3]), out, Policy(), chunk_bytes=chunk_bytes, indices_out=indices)
        assert out.getvalue() == b"" and indices.getvalue() == ""  # last: nothing is written
    out = io.BytesIO()
    with pytest.raises(ValueError, match="truncated"):
        dd.dedupe_file(io.BytesIO(data[:-3]), out, Policy("first"), chunk_bytes=700)
    want = dedupe_cpu(data, Policy("first")).data
    written = out.getvalue()
    assert written and written == want[:len(written)]  # first: whole frames only
    list(iter_frames(written))


# ---- the command ------------------------------------------------------------------------------------

def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_cli_dedupe_from_stdin_to_stdout():
    data = corpus()
    r = _cli("dedupe", "-o", "-", stdin=data)
    want = dedupe_cpu(data)
    assert r.returncode == 0 and r.stdout == want.data
    assert json.loads(r.stderr) == {"frames": 5711, "kept": 5008, "kept_bytes": len(want.data), "duplicates": 703,
                                    "host_frames": 0}


def test_cli_dedupe_files_options_and_the_chain(tmp_path):
    data = Workload(n_media=8, seed=5).framed(400) * 2
    capture, out, indices = tmp_path / "capture.bin", tmp_path / "out.bin", tmp_path / "kept.txt"
    capture.write_bytes(data)
    r = _cli("dedupe", str(capture), "-o", str(out), "--keep", "first", "--topic", "status", "--topic", "7",
             "--indices", str(indices), "--chunk-bytes", "700")
    assert r.returncode == 0 and not r.stdout, r.stderr
    want = dedupe_cpu(data, Policy("first", {STATUS_ID, 7}))
    assert out.read_bytes() == want.data and [int(line) for line in indices.read_text().split()] == want.indices
    assert json.loads(r.stderr)["duplicates"] == want.frames - len(want.indices) > 0
    # extract -> dedupe -> coalesce: the chain stays closed
    r = _cli("dedupe", str(capture), "-o", str(out))
    assert r.returncode == 0
    r = _cli("coalesce", str(out), "-o", "-")
    assert r.returncode == 0 and r.stdout == co.coalesce_cpu(data).data


def test_cli_dedupe_usage_errors_exit_2(tmp_path):
    data = Workload(n_media=4, seed=5).framed(20)
    out = str(tmp_path / "out.bin")
    assert _cli("dedupe", stdin=data).returncode == 2  # -o is required
    assert _cli("dedupe", "-o", out, "--keep", "newest", stdin=data).returncode == 2
    assert _cli("dedupe", "-o", out, "--topic", "256", stdin=data).returncode == 2
    assert _cli("dedupe", "-o", out, "--topic", "media", stdin=data).returncode == 2
    assert _cli("dedupe", "-o", out, "--dialect", "upb", stdin=data).returncode == 2  # nothing is decoded
    assert not list(tmp_path.iterdir())


def test_cli_dedupe_truncated_input(tmp_path):
    data = Workload(n_media=4, seed=5).framed(50) * 2
    r = _cli("dedupe", "-o", str(tmp_path / "last.bin"), "--chunk-bytes", "700", stdin=data[:-3])
    assert r.returncode == 1 and b"truncated" in r.stderr and not list(tmp_path.iterdir())
    r = _cli("dedupe", "-o", str(tmp_path / "first.bin"), "--keep", "first", "--chunk-bytes", "700", stdin=data[:-3])
    assert r.returncode == 1 and b"truncated" in r.stderr
    written = (tmp_path / "first.bin").read_bytes()
    assert written and written == dedupe_cpu(data, Policy("first")).data[:len(written)]
    list(iter_frames(written))


def test_cli_dedupe_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    from beholder_amd.ops import hip_lib
    path, out = tmp_path / "capture.bin", tmp_path / "cut.bin"
    path.write_bytes(Workload(n_media=2, seed=5).framed(10))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["dedupe", str(path), "-o", str(out), "--device", "gpu"]) != 0
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "no GPU" in err.err and not err.out and not out.exists()
    # and with a device but no library
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "libbeholder_hip.so"))
    monkeypatch.setattr(hip_lib, "_lib", None)
    assert cli.main(["dedupe", str(path), "-o", str(out), "--device", "gpu"]) != 0
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "missing" in err.err and not err.out and not out.exists()
