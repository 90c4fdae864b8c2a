"""``thin`` on the CPU: the definition (beholder_amd/thin.py), its five laws, what it means for the
coalesce and the fold, ``thin_file`` and the command."""
from __future__ import annotations

import functools
import io
import json
import subprocess
import sys

import pytest

from beholder_amd import coalesce as co, ops, replay, thin as th
from beholder_amd.coalesce import _spans
from beholder_amd.ops import frames
from beholder_amd.thin import Policy, Thinned, thin_cpu
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames
from telemetry_corpus import body as _body
from thin_cases import (KEEPS, PERCENTAGES, POLICIES, STEPS, UNKNOWN_STATUSES, corpus, edge_stream, mixed_stream,
                        non_ascii_stream, policy_id, progress_body, progress_stream, random_stream, stitch_stream)

SEEDS = (1, 2, 3)
FFFD = "�"


def _frame_list(data: bytes) -> list:
    return [ops.frame(topic, body) for topic, body in iter_frames(data)]


@functools.lru_cache(maxsize=None)
def _fold(data: bytes, dialect: str) -> replay.Summary:
    return replay.fold_cpu(data, dialect)


def _streams() -> list:
    return [random_stream(seed) for seed in SEEDS] + \
        [edge_stream(), stitch_stream(), non_ascii_stream(), mixed_stream()]


# ---- the policy and the arguments -------------------------------------------------------------------

def test_the_policy_is_validated():
    assert Policy() == Policy(step=10, keep="last")
    assert Policy(1).step == 1 and Policy(2 ** 31 - 1).step == 2 ** 31 - 1
    for bad in (0, -1, -10, 2 ** 31, 2 ** 64):
        with pytest.raises(ValueError):
            Policy(bad)
    for bad in (True, False):
        with pytest.raises(TypeError):
            Policy(bad)
    for bad in (None, 10.0, "10", b"10", 2.5):
        with pytest.raises((TypeError, ValueError)):
            Policy(bad)
    for bad in ("", "all", "LAST", "newest"):
        with pytest.raises(ValueError):
            Policy(keep=bad)
    for bad in (None, 0, b"last", True):
        with pytest.raises(TypeError):
            Policy(keep=bad)
    assert hash(Policy(25, "first")) == hash(Policy(step=25, keep="first"))


def test_bad_arguments_raise():
    data = progress_stream([(b"m", 1, 5)] * 2)
    with pytest.raises(TypeError):
        thin_cpu(data, 10)
    with pytest.raises(TypeError):
        th.mark_of("last")
    with pytest.raises(ValueError):
        thin_cpu(data, Policy(), "proto2")
    with pytest.raises(TypeError):
        th.thin_file(io.BytesIO(data), io.BytesIO(), "last")
    with pytest.raises(ValueError):
        th.thin_file(io.BytesIO(data), io.BytesIO(), Policy(), dialect="proto2")
    with pytest.raises(ValueError):
        th.thin_file(io.BytesIO(data), io.BytesIO(), Policy(), chunk_bytes=0)
    for broken in (data[:-1], data + b"\x01\x00", data + b"\x00\x00\x00\x00"):
        with pytest.raises(ValueError):
            thin_cpu(broken)
    for policy in POLICIES:
        assert thin_cpu(b"", policy) == Thinned(b"", [], 0, policy.step, policy.keep, "protobufjs", 0)


def test_by_hand():
    events = [(b"m", 2, 0), (b"m", 2, 5), (b"n", 2, 5), (b"m", 2, 9), (b"m", 2, 10), (b"n", 2, 7), (b"m", 3, 10),
              (b"m", 3, 19), (b"m", 2, 19)]
    data = progress_stream(events)
    assert thin_cpu(data).indices == [3, 4, 5, 7, 8]              # 9 survives before 10, a stage's last before the next
    assert thin_cpu(data, Policy(keep="first")).indices == [0, 2, 4, 6, 8]
    assert thin_cpu(data, Policy(1)).indices == list(range(9))    # every event moves by a step of 1
    assert thin_cpu(data, Policy(2 ** 31 - 1)).indices == [4, 5, 7, 8]   # one bucket for 0..: the statuses still part
    assert thin_cpu(data).data == b"".join(_frame_list(data)[i] for i in (3, 4, 5, 7, 8))
    assert thin_cpu(data).frames == thin_cpu(data).progress_events == 9


def test_the_mark_floors_its_division():
    mark = th.mark_of(Policy(10))
    want = {-2 ** 31: -214748365, -11: -2, -10: -1, -1: -1, 0: 0, 9: 0, 10: 1, 99: 9, 100: 10, 101: 10,
            2 ** 31 - 1: 214748364}
    assert set(want) == set(PERCENTAGES)
    for p, bucket in want.items():
        assert mark(PROGRESS_ID, progress_body(b"m", 2, p)) == ("m", 2, bucket)
    assert th.mark_of(Policy(1))(PROGRESS_ID, progress_body(b"m", 2, -2 ** 31)) == ("m", 2, -2 ** 31)
    assert th.mark_of(Policy(2 ** 31 - 1))(PROGRESS_ID, progress_body(b"m", 2, -2 ** 31)) == ("m", 2, -2)
    assert th.mark_of(Policy(2 ** 31 - 1))(PROGRESS_ID, progress_body(b"m", 2, -1)) == ("m", 2, -1)
    assert th.mark_of(Policy(2 ** 31 - 1))(PROGRESS_ID, progress_body(b"m", 2, 2 ** 31 - 1)) == ("m", 2, 1)
    # -1 and 0 are neighbours on the number line and never in one bucket
    data = progress_stream([(b"m", 2, -1), (b"m", 2, 0)])
    for policy in POLICIES:
        assert thin_cpu(data, policy).indices == [0, 1]
    # no other frame has a mark
    for topic, payload in ((STATUS_ID, _body(b"m", 2)), (9, progress_body(b"m", 2, 5)), (PROGRESS_ID, b"\x2e")):
        assert mark(topic, payload) is None


def test_unknown_status_numbers_are_distinct_marks():
    events = [(b"m", s, 5) for s in UNKNOWN_STATUSES for _ in range(2)]
    data = progress_stream(events)
    assert thin_cpu(data).indices == [1, 3, 5] and thin_cpu(data, Policy(keep="first")).indices == [0, 2, 4]
    data = progress_stream([(b"m", s, 5) for s in UNKNOWN_STATUSES * 2])
    assert thin_cpu(data).indices == list(range(6))  # 6, 64, -1, 6, 64, -1: no neighbours share a status


def test_ids_that_are_no_utf8_are_one_media_under_protobufjs():
    data = progress_stream([(b"\xff", 2, 5), (b"\xfe", 2, 6), (b"\xff", 2, 7), (b"\xfe", 2, 15)])
    assert thin_cpu(data).indices == [2, 3] and thin_cpu(data, Policy(keep="first")).indices == [0, 3]
    assert th.mark_of()(PROGRESS_ID, progress_body(b"\xfe", 2, 6)) == (FFFD, 2, 0)
    got = thin_cpu(data, Policy(), "upb")  # upb raises on them: no events, everything kept
    assert got.indices == [0, 1, 2, 3] and got.progress_events == 0


def test_a_host_change_alone_does_not_keep_a_frame():
    bodies = [progress_body(b"m", 2, 5, b"node-a"), progress_body(b"m", 2, 6, b"node-b"), progress_body(b"m", 2, 7)]
    data = frames([(PROGRESS_ID, b) for b in bodies])
    assert thin_cpu(data).indices == [2] and thin_cpu(data, Policy(keep="first")).indices == [0]
    assert "host" in th.__doc__ and "host" in th.mark_of.__doc__.lower()


def test_other_frames_stay_where_they_are():
    events = [(STATUS_ID, _body(b"m", 1)), (PROGRESS_ID, b"\x2e"), (9, progress_body(b"m", 2, 5)), (0, b""),
              (PROGRESS_ID, progress_body(b"m", 2, 5)), (STATUS_ID, _body(b"m", 1)), (PROGRESS_ID, b"\x2e")] * 2
    data = frames(events)
    assert thin_cpu(data).indices == [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13]
    assert thin_cpu(data, Policy(keep="first")).indices == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13]


# ---- laws -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_result_is_the_definition_and_idempotent(policy, dialect):
    """Law 1, and the definition spelled out independently of thin_cpu's own loop."""
    mark = th.mark_of(policy, dialect)
    dropped_somewhere = False
    for data in _streams():
        whole = _frame_list(data)
        got = thin_cpu(data, policy, dialect)
        assert (got.frames, got.step, got.keep, got.dialect) == (len(whole), policy.step, policy.keep, dialect)
        marks = [mark(f[4], f[5:]) for f in whole]
        want = []
        for i, m in enumerate(marks):
            if m is not None:
                side = marks[i + 1:] if policy.keep == "last" else marks[:i][::-1]
                neighbour = next((o for o in side if o is not None and o[0] == m[0]), None)
                if neighbour == m:
                    continue
            want.append(i)
        assert got.indices == want and got.data == b"".join(whole[i] for i in want)
        assert got.progress_events == sum(m is not None for m in marks)
        again = thin_cpu(got.data, policy, dialect)
        assert again.data == got.data and again.indices == list(range(len(want)))
        dropped_somewhere |= len(want) < len(whole)
    assert dropped_somewhere


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("step", STEPS)
def test_first_has_a_sequential_form(step, dialect):
    """Law 2: keep a progress event iff its mark differs from the media's previous kept one."""
    mark = th.mark_of(Policy(step, "first"), dialect)
    for data in _streams():
        previous, want = {}, []
        for i, f in enumerate(_frame_list(data)):
            m = mark(f[4], f[5:])
            if m is not None:
                if previous.get(m[0]) == m:
                    continue
                previous[m[0]] = m
            want.append(i)
        assert thin_cpu(data, Policy(step, "first"), dialect).indices == want


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("step", STEPS)
def test_last_is_safe_before_the_coalesce(step, dialect):
    """Law 3."""
    for data in _streams() + [corpus()]:
        got = thin_cpu(data, Policy(step), dialect)
        for mode in ("last", "per-status"):
            policy = co.Policy(progress=mode)
            assert co.coalesce_cpu(got.data, policy, dialect).data == co.coalesce_cpu(data, policy, dialect).data


def test_first_is_not_safe_before_the_coalesce():
    data = progress_stream([(b"m", 2, 1), (b"m", 2, 2)])
    got = thin_cpu(data, Policy(keep="first"))
    assert co.coalesce_cpu(got.data).data != co.coalesce_cpu(data).data


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_the_fold_keeps_its_statuses_and_counters(policy, dialect):
    """Law 4."""
    for data in _streams() + [corpus()]:
        got = thin_cpu(data, policy, dialect)
        before, after = _fold(data, dialect), replay.fold_cpu(got.data, dialect)
        assert {mid: f.last_status for mid, f in after.media.items()} == \
            {mid: f.last_status for mid, f in before.media.items()}
        assert {mid: f.status_events for mid, f in after.media.items()} == \
            {mid: f.status_events for mid, f in before.media.items()}
        assert (after.status_decode_errors, after.progress_decode_errors, after.other_topic) == \
            (before.status_decode_errors, before.progress_decode_errors, before.other_topic)
        dropped = got.frames - len(got.indices)
        events = sum(f.progress_events for f in before.media.values())
        assert events == got.progress_events
        assert sum(f.progress_events for f in after.media.values()) == events - dropped
        assert after.frames == before.frames - dropped


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("policy", POLICIES, ids=policy_id)
def test_results_merge_at_every_frame_boundary(policy, dialect):
    """Law 5."""
    for data in (random_stream(1, 70), stitch_stream()):
        want = thin_cpu(data, policy, dialect)
        for _, cut in _spans(data):
            assert thin_cpu(data[:cut], policy, dialect).merge(thin_cpu(data[cut:], policy, dialect)) == want
        empty = thin_cpu(b"", policy, dialect)
        assert empty.merge(want) == want == want.merge(empty)


def test_mismatched_merges_raise():
    data = random_stream(1)
    for a, b in ((Policy(), Policy(keep="first")), (Policy(10), Policy(25)), (Policy(1, "first"), Policy(2, "last"))):
        with pytest.raises(ValueError):
            thin_cpu(data, a).merge(thin_cpu(data, b))
        with pytest.raises(ValueError):
            thin_cpu(data, b).merge(thin_cpu(b"", a))
    with pytest.raises(ValueError):
        thin_cpu(data, Policy(), "upb").merge(thin_cpu(data, Policy(), "protobufjs"))


def test_the_percentage_edges_depend_on_the_step():
    data = edge_stream()
    kept = {policy_id(p): len(thin_cpu(data, p).indices) for p in POLICIES}
    assert kept["1-last"] == kept["1-first"] > kept["10-last"] == kept["10-first"] > kept["25-last"] > \
        kept["2147483647-last"] == kept["2147483647-first"]


# ---- thin_file --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("keep", KEEPS)
def test_thin_file_in_small_chunks_equals_the_one_shot_result(keep, dialect):
    for data, chunk_bytes in ((corpus(), 30_000), (random_stream(2), 1), (stitch_stream(), 200)):
        policy = Policy(10, keep)
        want = thin_cpu(data, policy, dialect)
        assert len(data) > 3 * chunk_bytes
        for size in (chunk_bytes, 1 << 30):  # three chunks or more, and one
            out, indices = io.BytesIO(), io.StringIO()
            counts = th.thin_file(io.BytesIO(data), out, policy, dialect=dialect, chunk_bytes=size, indices_out=indices)
            assert out.getvalue() == want.data
            assert [int(line) for line in indices.getvalue().split()] == want.indices
            assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                              "progress_events": want.progress_events, "dropped": want.frames - len(want.indices),
                              "host_frames": 0}
            assert counts["dropped"] > 0


def test_thin_file_of_one_chunk_builds_no_host_state(monkeypatch):
    def no_state(*a, **kw):
        raise AssertionError("one chunk needs no cross-chunk state")
    monkeypatch.setattr(th, "_marks", no_state)
    data = corpus()
    for policy in (Policy(), Policy(keep="first")):
        out = io.BytesIO()
        assert th.thin_file(io.BytesIO(data), out, policy)["kept"] == len(thin_cpu(data, policy).indices)
        assert out.getvalue() == thin_cpu(data, policy).data
        with pytest.raises(AssertionError):
            th.thin_file(io.BytesIO(data), io.BytesIO(), policy, chunk_bytes=30_000)


def test_first_writes_each_chunk_before_it_reads_the_next():
    data = random_stream(3)
    want = thin_cpu(data, Policy(keep="first")).data

    class Watched(io.BytesIO):
        def read(self, size=-1):
            reads.append(len(out.getvalue()))
            return super().read(size)
    reads, out = [], io.BytesIO()
    th.thin_file(Watched(data), out, Policy(keep="first"), chunk_bytes=400)
    assert out.getvalue() == want and len(set(reads)) > 3  # the output grew between the reads
    reads, out = [], io.BytesIO()
    th.thin_file(Watched(data), out, Policy(), chunk_bytes=400)
    assert set(reads) == {0} and out.getvalue() == thin_cpu(data).data  # last: written once, at the end


def test_a_stream_that_ends_inside_a_frame():
    data = random_stream(2)
    for chunk_bytes in (400, 1 << 30):
        out, indices = io.BytesIO(), io.StringIO()
        with pytest.raises(ValueError, match="truncated"):
            th.thin_file(io.BytesIO(data[:-3]), out, Policy(), chunk_bytes=chunk_bytes, indices_out=indices)
        assert out.getvalue() == b"" and indices.getvalue() == ""  # last: nothing is written
    out = io.BytesIO()
    with pytest.raises(ValueError, match="truncated"):
        th.thin_file(io.BytesIO(data[:-3]), out, Policy(keep="first"), chunk_bytes=400)
    want = thin_cpu(data, Policy(keep="first")).data
    written = out.getvalue()
    assert written and written == want[:len(written)]  # first: whole frames only
    list(iter_frames(written))


# ---- the command ------------------------------------------------------------------------------------

def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_cli_thin_from_stdin_to_stdout():
    data = corpus()
    r = _cli("thin", "-o", "-", stdin=data)
    want = thin_cpu(data)
    assert r.returncode == 0 and r.stdout == want.data
    assert json.loads(r.stderr) == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                                    "progress_events": want.progress_events,
                                    "dropped": want.frames - len(want.indices), "host_frames": 0}
    assert want.frames > len(want.indices)


def test_cli_thin_files_options_and_the_chain(tmp_path):
    data = random_stream(3, 400)
    capture, out, indices = tmp_path / "capture.bin", tmp_path / "out.bin", tmp_path / "kept.txt"
    capture.write_bytes(data)
    r = _cli("thin", str(capture), "-o", str(out), "--step", "25", "--keep", "first", "--dialect", "upb",
             "--indices", str(indices), "--chunk-bytes", "700")
    assert r.returncode == 0 and not r.stdout, r.stderr
    want = thin_cpu(data, Policy(25, "first"), "upb")
    assert out.read_bytes() == want.data and [int(line) for line in indices.read_text().split()] == want.indices
    assert json.loads(r.stderr)["dropped"] == want.frames - len(want.indices) > 0
    # thin, then coalesce, is coalesce
    assert _cli("thin", str(capture), "-o", str(out)).returncode == 0
    r = _cli("coalesce", str(out), "-o", "-")
    assert r.returncode == 0 and r.stdout == co.coalesce_cpu(data).data


def test_cli_thin_usage_errors_exit_2(tmp_path):
    data = random_stream(1, 20)
    out = str(tmp_path / "out.bin")
    assert _cli("thin", stdin=data).returncode == 2  # -o is required
    assert _cli("thin", "-o", out, "--keep", "newest", stdin=data).returncode == 2
    assert _cli("thin", "-o", out, "--step", "0", stdin=data).returncode == 2
    assert _cli("thin", "-o", out, "--step", "-5", stdin=data).returncode == 2
    assert _cli("thin", "-o", out, "--step", str(2 ** 31), stdin=data).returncode == 2
    assert _cli("thin", "-o", out, "--step", "ten", stdin=data).returncode == 2
    assert _cli("thin", "-o", out, "--dialect", "proto2", stdin=data).returncode == 2
    assert not list(tmp_path.iterdir())


def test_cli_thin_truncated_input(tmp_path):
    data = random_stream(2)
    r = _cli("thin", "-o", str(tmp_path / "last.bin"), "--chunk-bytes", "400", stdin=data[:-3])
    assert r.returncode == 1 and b"truncated" in r.stderr and not list(tmp_path.iterdir())
    r = _cli("thin", "-o", str(tmp_path / "first.bin"), "--keep", "first", "--chunk-bytes", "400", stdin=data[:-3])
    assert r.returncode == 1 and b"truncated" in r.stderr
    written = (tmp_path / "first.bin").read_bytes()
    assert written and written == thin_cpu(data, Policy(keep="first")).data[:len(written)]
    list(iter_frames(written))


def test_cli_thin_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    from beholder_amd.ops import hip_lib
    path, out = tmp_path / "capture.bin", tmp_path / "cut.bin"
    path.write_bytes(random_stream(1, 10))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["thin", str(path), "-o", str(out), "--device", "gpu"]) != 0
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "no GPU" in err.err and not err.out and not out.exists()
    # and with a device but no library
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "libbeholder_hip.so"))
    monkeypatch.setattr(hip_lib, "_lib", None)
    assert cli.main(["thin", str(path), "-o", str(out), "--device", "gpu"]) != 0
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "missing" in err.err and not err.out and not out.exists()
    assert "thin " in cli.__doc__
