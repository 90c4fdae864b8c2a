"""``transitions`` (beholder_amd/transitions.py): the definition, ``transitions_cpu``, and its laws
against the fold, the shard and the coalesce; the merge, the JSON form, ``transitions_file`` and the
command on the CPU."""
from __future__ import annotations

import io
import json
import subprocess
import sys

import pytest

from beholder_amd import coalesce, ops, replay, shard
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transitions import UNKNOWN, MediaFlow, Transitions, class_of, transitions_cpu, transitions_file
from beholder_amd.transport.framing import iter_frames
from telemetry_corpus import body
from transitions_cases import UNKNOWN_NUMBERS, corpus, mixed_stream, shared_media_stream, three_statuses

NUMBERS = {name: number for number, name in replay.status_names().items()}
FFFD = "�"


def _boundaries(data: bytes) -> list:
    out, at = [0], 0
    for _, b in iter_frames(data):
        at += 5 + len(b)
        out.append(at)
    return out


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_merge_law_at_every_frame_boundary_of_the_mixed_stream(dialect):
    data = mixed_stream()
    whole = transitions_cpu(data, dialect)
    cuts = _boundaries(data)
    assert len(cuts) == 61 and whole.media and whole.matrix
    for cut in cuts:
        a, b = transitions_cpu(data[:cut], dialect), transitions_cpu(data[cut:], dialect)
        before = (Transitions.from_json(a.to_json(True)), Transitions.from_json(b.to_json(True)))
        assert a.merge(b) == whole, cut
        assert (a, b) == before  # neither operand changes


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_merge_law_on_the_fold_corpus(dialect):
    data = corpus()
    whole = transitions_cpu(data, dialect)
    cuts = _boundaries(data)
    for k in (0, 1, 7, len(cuts) // 3, len(cuts) // 2, len(cuts) - 2, len(cuts) - 1):
        assert transitions_cpu(data[:cuts[k]], dialect).merge(transitions_cpu(data[cuts[k]:], dialect)) == whole, k
    third = len(cuts) // 3
    parts = [transitions_cpu(data[cuts[a]:cuts[b]], dialect) for a, b in ((0, third), (third, 2 * third), (2 * third, -1))]
    assert parts[0].merge(parts[1]).merge(parts[2]) == whole == parts[0].merge(parts[1].merge(parts[2]))


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("stream", [corpus, mixed_stream, shared_media_stream], ids=lambda f: f.__name__)
def test_arithmetic_and_the_fold_law(stream, dialect):
    data = stream()
    t = transitions_cpu(data, dialect)
    fold = replay.fold_cpu(data, dialect)
    assert t.frames == fold.frames and t.status_decode_errors == fold.status_decode_errors
    assert t.transitions == sum(t.matrix.values()) == t.status_events - len(t.media)
    assert t.changes + t.repeats == t.transitions and all(t.matrix.values())
    assert t.changes == sum(flow.changes for flow in t.media.values())
    assert t.status_events == sum(flow.status_events for flow in t.media.values())
    assert sum(t.starts().values()) == sum(t.ends().values()) == len(t.media)
    with_status = {mid: f for mid, f in fold.media.items() if f.status_events}
    assert set(t.media) == set(with_status)
    for mid, flow in t.media.items():
        f = with_status[mid]
        assert (flow.status_events, flow.last_status, flow.last_index) == (f.status_events, f.last_status,
                                                                           f.last_status_index), mid
        assert flow.first_index <= flow.last_index and flow.changes <= flow.status_events - 1
        assert (flow.first_index == flow.last_index) == (flow.status_events == 1)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("shards", [1, 3, 64])
def test_the_shard_law(shards, dialect):
    data = corpus()
    whole = transitions_cpu(data, dialect)
    sharded = shard.shard_cpu(data, shard.Policy(shards), dialect)
    matrix, media = {}, {}
    for part, indices in zip(sharded.data, sharded.indices):
        t = transitions_cpu(part, dialect)
        for cell, count in t.matrix.items():
            matrix[cell] = matrix.get(cell, 0) + count
        for mid, flow in t.media.items():
            assert mid not in media  # a media lives in one shard
            media[mid] = MediaFlow(flow.status_events, flow.changes, flow.first_status, indices[flow.first_index],
                                   flow.last_status, indices[flow.last_index])
    assert matrix == whole.matrix and media == whole.media


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_coalesce_law(dialect):
    data = corpus()
    whole = transitions_cpu(data, dialect)
    cut = coalesce.coalesce_cpu(data, coalesce.Policy(status="last"), dialect)
    after = transitions_cpu(cut.data, dialect)
    assert after.matrix == {} and after.ends() == whole.ends() and set(after.media) == set(whole.media)
    assert all(flow.status_events == 1 for flow in after.media.values())


def test_unknown_numbers_are_one_class():
    names = replay.status_names()
    assert [class_of(s, names) for s in UNKNOWN_NUMBERS] == [UNKNOWN] * 5
    assert [class_of(s, names) for s in sorted(names)] == sorted(names)
    statuses = (0,) + UNKNOWN_NUMBERS + (4,)
    for dialect in ops.DIALECTS:
        t = transitions_cpu(frames([(STATUS_ID, body(b"m", s)) for s in statuses]), dialect)
        assert t.matrix == {(0, UNKNOWN): 1, (UNKNOWN, UNKNOWN): 4, (UNKNOWN, 4): 1}
        assert t.media == {"m": MediaFlow(7, 2, 0, 0, 4, 6)} and (t.changes, t.repeats) == (2, 4)


def test_redelivery_of_three_statuses():
    t = transitions_cpu(three_statuses())
    q, e = NUMBERS["QUEUED"], NUMBERS["ERRORED"]
    assert t.matrix == {(q, e): 1, (e, q): 1} and t.media == {"m-1": MediaFlow(3, 2, q, 0, q, 2)}
    assert t.to_json()["transitions"] == {"ERRORED": {"QUEUED": 1}, "QUEUED": {"ERRORED": 1}}
    storm = transitions_cpu(frames([(STATUS_ID, body(b"m-1", q))] * 5 + [(PROGRESS_ID, body(b"m-1", e))]))
    assert storm.matrix == {(q, q): 4} and (storm.changes, storm.repeats, storm.frames) == (0, 4, 6)


def test_identity_is_the_decoded_string():
    data = frames([(STATUS_ID, body(b"\xff", 1)), (STATUS_ID, body(b"\xfe", 2)), (STATUS_ID, b"\x10\x03")])
    t = transitions_cpu(data, "protobufjs")
    assert t.media == {FFFD: MediaFlow(2, 1, 1, 0, 2, 1), "": MediaFlow(1, 0, 3, 2, 3, 2)}
    assert t.matrix == {(1, 2): 1} and t.status_decode_errors == 0
    u = transitions_cpu(data, "upb")
    assert u.status_decode_errors == 2 and set(u.media) == {""} and u.matrix == {}


def test_other_frames_count_in_frames_only():
    data = frames([(PROGRESS_ID, body(b"m", 1)), (9, body(b"m", 2)), (STATUS_ID, b"\x2e"), (0, b"")])
    assert transitions_cpu(data) == Transitions(frames=4, status_decode_errors=1)
    assert transitions_cpu(b"") == Transitions()
    for broken in (data[:-1], data + b"\x01", data + b"\x00\x00\x00\x00"):
        with pytest.raises(ValueError):
            transitions_cpu(broken)
    with pytest.raises(ValueError):
        transitions_cpu(data, "proto2")


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_json_round_trip(dialect):
    t = transitions_cpu(corpus(), dialect)
    short, full = t.to_json(), t.to_json(per_media=True)
    assert json.loads(json.dumps(full)) == full
    assert Transitions.from_json(json.loads(json.dumps(full))) == t
    assert "media" not in short and {k: v for k, v in full.items() if k != "media"} == short
    names = set(NUMBERS) | {UNKNOWN}
    assert set(short["transitions"]) <= names and list(short["transitions"]) == sorted(short["transitions"])
    for row in short["transitions"].values():
        assert set(row) <= names and list(row) == sorted(row) and all(row.values())
    assert UNKNOWN in short["transitions"] and UNKNOWN in short["starts"]
    assert short["media_count"] == len(t.media) == sum(short["starts"].values()) == sum(short["ends"].values())
    assert short["changes"] + short["repeats"] == sum(sum(row.values()) for row in short["transitions"].values())
    assert (short["frames"], short["status_events"], short["status_decode_errors"]) == \
        (t.frames, t.status_events, t.status_decode_errors)
    with pytest.raises(ValueError):
        Transitions.from_json(short)  # no per-media rows: not a whole result


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_transitions_file_in_chunks_equals_the_whole(dialect, tmp_path):
    data = corpus()
    want = transitions_cpu(data, dialect)
    assert len(data) > 7 * 30_000
    assert transitions_file(io.BytesIO(data), dialect=dialect, chunk_bytes=30_000) == (want, 0)
    path = tmp_path / "capture.bin"
    path.write_bytes(data)
    assert transitions_file(str(path), "cpu", dialect) == (want, 0)
    assert transitions_file(io.BytesIO(b"")) == (Transitions(), 0)
    with pytest.raises(ValueError):
        transitions_file(io.BytesIO(data[:-1]), chunk_bytes=30_000)


def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_cli_on_the_cpu(tmp_path):
    data = mixed_stream()
    path = tmp_path / "capture.bin"
    path.write_bytes(data)
    want = transitions_cpu(data)
    r = _cli("transitions", str(path), "--device", "cpu", "--chunk-bytes", "200", "--per-media")
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out.pop("host_frames") == 0
    assert out == json.loads(json.dumps(want.to_json(per_media=True))) and Transitions.from_json(out) == want
    r = _cli("transitions", "--dialect", "upb", stdin=data)  # stdin, default device, no rows
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out.pop("host_frames") == 0 and "media" not in out
    assert out == json.loads(json.dumps(transitions_cpu(data, "upb").to_json()))
    r = _cli("transitions", stdin=data[:-1])  # a broken stream
    assert r.returncode == 1 and b"beholder: " in r.stderr and not r.stdout


def test_cli_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    path = tmp_path / "capture.bin"
    path.write_bytes(mixed_stream())
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["transitions", str(path), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device gpu is not available" in out.err and "--device cpu" in out.err and not out.out
