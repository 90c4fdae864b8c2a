"""``stages``: the definition (beholder_amd/stages.py) against its laws, the transitions and the fold,
its JSON form, its chunked file form, the command line and hand-written cases."""
from __future__ import annotations

import io
import json
import subprocess
import sys

import pytest

from beholder_amd import ops, replay
from beholder_amd.ops import frames
from beholder_amd.stages import (BUCKETS, PROGRESS, STATUS, MediaStand, StageReport, bucket_of, course_of, events_of,
                                 stages_cpu, stages_file)
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transitions import UNKNOWN, class_of, transitions_cpu
from beholder_amd.transport.framing import iter_frames
from stages_cases import P, S, bucket_edges, corpus, joined_stream, merge_stream, random_stream, stitch_stream
from telemetry_corpus import body
from thin_cases import PERCENTAGES, UNKNOWN_STATUSES, progress_body

SEEDS = (1, 2, 3)
# frames, status and progress events, their decode errors, media, lead events, agree, disagree, closed and open stages
CORPUS_NUMBERS = {"protobufjs": (5711, 1622, 2865, 656, 553, 353, 271, 682, 1912, 1276, 346),
                  "upb": (5711, 1314, 2452, 964, 966, 68, 121, 468, 1863, 1246, 68)}


def _boundaries(data: bytes):
    off = 0
    yield 0
    for _, b in iter_frames(data):
        off += 5 + len(b)
        yield off


def _courses(data: bytes, dialect: str) -> dict:
    events = ((i, topic, bytes(b)) for i, (topic, b) in enumerate(iter_frames(data)))
    return {mid: course_of(run) for mid, run in events_of(events, dialect)[0].items()}


def _check_laws(r: StageReport, data: bytes, dialect: str) -> None:
    opened = sum(1 for stand in r.media.values() if stand.open is not None)
    assert sum(r.entered.values()) == r.status_events == sum(r.closed.values()) + opened == \
        sum(r.closed.values()) + sum(r.open.values())
    assert sum(r.matrix.values()) + r.lead_events == r.progress_events == r.agree + r.disagree + r.lead_events
    assert all(r.entered.values()) and all(r.matrix.values()) and all(r.closed.values())
    assert {b for _, b in r.closed} | {b for _, b in r.open} <= set(BUCKETS)
    courses = _courses(data, dialect)
    assert set(courses) == set(r.media)
    stage_counts = 0
    for mid, course in courses.items():
        stand = r.media[mid]
        assert stand == course.stand
        counts = sum(count for _, count, _, _ in course.stages)
        assert stand.events == stand.lead_count + counts + len(course.stages)
        assert [closed for *_, closed in course.stages] == [True] * (len(course.stages) - 1) + [False] * bool(course.stages)
        assert (stand.lead_last is None) == (stand.lead_count == 0) and all(stand.lead.values())
        stage_counts += counts
    assert stage_counts + r.lead_events == r.progress_events
    assert sum(stand.events for stand in r.media.values()) == r.status_events + r.progress_events


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("seed", SEEDS)
def test_the_laws(seed, dialect):
    data = random_stream(seed)
    r = stages_cpu(data, dialect)
    assert r.status_events > 15 and r.progress_events > 60 and r.lead_events > 3 and r.disagree > 5 and r.agree > 5
    assert r.status_decode_errors and r.progress_decode_errors and sum(r.closed.values()) > 5
    _check_laws(r, data, dialect)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_fold_corpus_numbers(dialect):
    data = corpus()
    r = stages_cpu(data, dialect)
    _check_laws(r, data, dialect)
    got = (r.frames, r.status_events, r.progress_events, r.status_decode_errors, r.progress_decode_errors,
           len(r.media), r.lead_events, r.agree, r.disagree, sum(r.closed.values()), sum(r.open.values()))
    assert got == CORPUS_NUMBERS[dialect]
    assert r.lead_events and r.disagree and r.closed and r.open


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("stream", [lambda: random_stream(1), lambda: random_stream(3), corpus],
                         ids=["r1", "r3", "corpus"])
def test_against_the_transitions_and_the_fold(stream, dialect):
    data = stream()
    r, t, fold = stages_cpu(data, dialect), transitions_cpu(data, dialect), replay.fold_cpu(data, dialect)
    assert (r.frames, r.status_events, r.status_decode_errors) == (t.frames, t.status_events, t.status_decode_errors)
    assert r.progress_decode_errors == fold.progress_decode_errors
    assert r.progress_events == sum(m.progress_events for m in fold.media.values())
    # the open stage stands on the media's last status event
    assert {mid: (s.open[1], s.open[0]) for mid, s in r.media.items() if s.open is not None} == \
        {mid: (flow.last_status, flow.last_index) for mid, flow in t.media.items()}
    assert r.open and sum(r.open.values()) == len(t.media)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_merge_law_at_every_frame_boundary(dialect):
    data = merge_stream()
    whole = stages_cpu(data, dialect)
    cuts = list(_boundaries(data))
    assert 50 <= whole.frames <= 70 and len(cuts) == whole.frames + 1
    seen = set()
    for cut in cuts:
        a, b = stages_cpu(data[:cut], dialect), stages_cpu(data[cut:], dialect)
        before = (a.to_json(True), b.to_json(True))
        assert a.merge(b) == whole
        assert (a.to_json(True), b.to_json(True)) == before  # neither operand changes
        for mid in set(a.media) & set(b.media):
            theirs, mine = b.media[mid], a.media[mid]
            if theirs.lead:
                seen.add("a lead joins an open stage" if mine.open is not None else "a lead joins a lead")
            if theirs.open is not None and mine.open is not None:
                seen.add("a stage closed by the later operand")
        if set(a.media) ^ set(b.media):
            seen.add("a media present in one operand only")
    assert len(seen) == 4, seen


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("seed", SEEDS)
def test_the_merge_law_on_the_seeded_streams(seed, dialect):
    data = random_stream(seed, 120)
    whole = stages_cpu(data, dialect)
    for cut in _boundaries(data):
        assert stages_cpu(data[:cut], dialect).merge(stages_cpu(data[cut:], dialect)) == whole
    cuts = list(_boundaries(data))
    for i, j in ((10, 11), (40, 90), (1, len(cuts) - 2), (0, 50)):
        a, b, c = (stages_cpu(data[x:y], dialect) for x, y in ((0, cuts[i]), (cuts[i], cuts[j]), (cuts[j], len(data))))
        assert a.merge(b).merge(c) == a.merge(b.merge(c)) == whole
    assert StageReport().merge(whole) == whole == whole.merge(StageReport())


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_merge_law_on_the_stitch_stream_and_the_corpus(dialect):
    for data, every in ((stitch_stream(), 1), (bucket_edges(), 1), (corpus(), 701)):
        whole = stages_cpu(data, dialect)
        for cut in list(_boundaries(data))[::every]:
            assert stages_cpu(data[:cut], dialect).merge(stages_cpu(data[cut:], dialect)) == whole


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_stages_file_in_chunks_equals_the_whole(dialect, tmp_path):
    data = random_stream(3)
    want = stages_cpu(data, dialect)
    for chunk_bytes in (1, 64, 1000, 1 << 20):  # 1: one frame per chunk
        assert stages_file(io.BytesIO(data), dialect=dialect, chunk_bytes=chunk_bytes) == (want, 0)
    whole = corpus()
    assert len(whole) > 7 * 30_000
    assert stages_file(io.BytesIO(whole), dialect=dialect, chunk_bytes=30_000) == (stages_cpu(whole, dialect), 0)
    path = tmp_path / "capture.bin"
    path.write_bytes(data)
    assert stages_file(str(path), "cpu", dialect) == (want, 0)
    assert stages_file(io.BytesIO(b"")) == (StageReport(), 0)
    with pytest.raises(ValueError):
        stages_file(io.BytesIO(data[:-1]), chunk_bytes=64)
    with pytest.raises(ValueError):
        stages_file(io.BytesIO(data), dialect="proto2")


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_json_round_trip(dialect):
    for data in (random_stream(1), bucket_edges(), corpus(), b""):
        r = stages_cpu(data, dialect)
        full = json.loads(json.dumps(r.to_json(per_media=True)))
        assert StageReport.from_json(full) == r
        short = r.to_json()
        assert "media" not in short and {k: v for k, v in full.items() if k != "media"} == json.loads(json.dumps(short))
        assert (short["media_count"], short["lead_events"], short["agree"], short["disagree"]) == \
            (len(r.media), r.lead_events, r.agree, r.disagree)
        assert list(full["media"]) == sorted(r.media) and list(short["entered"]) == sorted(short["entered"])
        for table in ("closed", "open"):
            assert list(short[table]) == sorted(short[table])
            for row in short[table].values():
                assert list(row) == [b for b in BUCKETS if b in row]
        assert json.dumps(short) == json.dumps(stages_cpu(data, dialect).to_json())  # the key order is the same
        with pytest.raises(ValueError):
            StageReport.from_json(short)  # no per-media rows: not a whole result
    short = stages_cpu(random_stream(1), dialect).to_json()
    classes = set(short["entered"]) | set(short["matrix"]) | {k for row in short["matrix"].values() for k in row}
    assert "unknown" in classes and classes - {"unknown"} <= set(replay.status_names().values())
    for table, key in (("entered", None), ("closed", "no-such-bucket")):
        bad = stages_cpu(random_stream(1), dialect).to_json(True)
        if key is None:
            bad[table]["NO_SUCH"] = 1
        else:
            next(iter(bad[table].values()))[key] = 1
        with pytest.raises(ValueError):
            StageReport.from_json(bad)


def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_cli_on_the_cpu(tmp_path):
    data = random_stream(1)
    path = tmp_path / "capture.bin"
    path.write_bytes(data)
    want = stages_cpu(data)
    r = _cli("stages", str(path), "--device", "cpu", "--chunk-bytes", "200", "--per-media")
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out.pop("host_frames") == 0
    assert out == json.loads(json.dumps(want.to_json(per_media=True))) and StageReport.from_json(out) == want
    r = _cli("stages", "--dialect", "upb", stdin=data)  # stdin, default device, no rows
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out.pop("host_frames") == 0 and "media" not in out
    assert out == json.loads(json.dumps(stages_cpu(data, "upb").to_json()))
    r = _cli("stages", stdin=data[:-1])  # a broken stream
    assert r.returncode == 1 and b"beholder: " in r.stderr and not r.stdout
    r = _cli("stages", str(path), "--dialect", "proto2")
    assert r.returncode == 2 and not r.stdout
    r = _cli("stages", "--help")
    assert r.returncode == 0 and b"--per-media" in r.stdout and b"standing" in r.stdout


def test_cli_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    path = tmp_path / "capture.bin"
    path.write_bytes(random_stream(1))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["stages", str(path), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device gpu is not available" in out.err and "--device cpu" in out.err and not out.out


def test_broken_framing_raises():
    data = joined_stream([(S, b"m", 1), (P, b"m", 1, 5)])
    for cut in (1, 4, 5, len(data) - 1):
        with pytest.raises(ValueError):
            stages_cpu(data[:cut])
    with pytest.raises(ValueError):
        stages_cpu(data, "proto2")
    assert stages_cpu(b"") == StageReport()


def test_status_then_progress():
    r = stages_cpu(joined_stream([(S, b"m", 2), (P, b"m", 2, 10), (P, b"m", 3, 40)]))
    assert r == StageReport(3, 1, 2, 0, 0, {2: 1}, {(2, 2): 1, (2, 3): 1}, {}, {"m": MediaStand({}, None, 3, (0, 2, 2, 40))})
    assert (r.agree, r.disagree, r.lead_events, r.open) == (1, 1, 0, {(2, "4"): 1})
    assert r.stuck(2) == ["m"] and r.stuck(2, below=40) == [] and r.stuck(3) == []


def test_progress_then_status():
    r = stages_cpu(joined_stream([(P, b"m", 2, 10), (P, b"m", 6, 20), (P, b"m", 2, 30), (S, b"m", 3)]))
    assert r == StageReport(4, 1, 3, 0, 0, {3: 1}, {}, {}, {"m": MediaStand({2: 2, UNKNOWN: 1}, 30, 4, (3, 3, 0, None))})
    assert (r.lead_events, r.open, r.stuck(3)) == (3, {(3, "none"): 1}, ["m"])


def test_progress_only_and_status_only():
    r = stages_cpu(joined_stream([(P, b"p", 2, 100), (S, b"s", 4), (P, b"p", 2, 7), (S, b"s", 4)]))
    assert r.media == {"p": MediaStand({2: 2}, 7, 2, None), "s": MediaStand({}, None, 2, (3, 4, 0, None))}
    assert (r.entered, r.matrix, r.closed, r.open) == ({4: 2}, {}, {(4, "none"): 1}, {(4, "none"): 1})
    assert r.lead_events == 2 and r.stuck(4) == ["s"] and r.stuck(2) == []


def test_queued_errored_queued_with_progress_between():
    names = {name: number for number, name in replay.status_names().items()}
    q, e = names["QUEUED"], names["ERRORED"]
    r = stages_cpu(joined_stream([(S, b"m", q), (P, b"m", q, 100), (S, b"m", e), (P, b"m", q, 15), (P, b"m", e, 15),
                                  (S, b"m", q), (P, b"n", q, 1), (P, b"m", q, 0)]))
    assert r.entered == {q: 2, e: 1} and r.matrix == {(q, q): 2, (e, q): 1, (e, e): 1}
    assert r.closed == {(q, "full"): 1, (e, "1"): 1} and r.open == {(q, "0"): 1}
    assert r.media["m"] == MediaStand({}, None, 7, (5, q, 1, 0)) and r.media["n"] == MediaStand({q: 1}, 1, 1, None)
    assert (r.agree, r.disagree, r.lead_events) == (3, 1, 1)


def test_every_bucket_edge():
    want = dict(zip(PERCENTAGES, ("below", "below", "below", "below", "0", "0", "1", "9", "full", "over", "over")))
    for p, bucket in want.items():
        assert bucket_of(1, p) == bucket and bucket_of(0, p) == "none"
        r = stages_cpu(joined_stream([(S, b"m", 2), (P, b"m", 2, 50), (P, b"m", 2, p), (S, b"m", 3), (P, b"m", 3, p)]))
        assert r.closed == {(2, bucket): 1} and r.open == {(3, bucket): 1}
    assert bucket_of(0, None) == "none" and len(BUCKETS) == 14 and len(set(BUCKETS)) == 14
    assert [bucket_of(1, p) for p in (10, 19, 20, 89, 90)] == ["1", "1", "2", "8", "9"]
    data = bucket_edges()
    r = stages_cpu(data)
    assert {b for _, b in r.closed} == {"none", "below", "0", "1", "9", "full", "over"}
    _check_laws(r, data, "protobufjs")


def test_unknown_statuses_on_both_topics():
    a, b, c = UNKNOWN_STATUSES
    r = stages_cpu(joined_stream([(S, b"m", a), (P, b"m", b, 5), (P, b"m", 2, 5), (S, b"m", c), (P, b"m", c, 9)]))
    assert r.entered == {UNKNOWN: 2} and r.matrix == {(UNKNOWN, UNKNOWN): 2, (UNKNOWN, 2): 1}
    assert r.closed == {(UNKNOWN, "0"): 1} and r.media["m"].open == (3, c, 1, 9)  # the raw status stays
    assert r.stuck(UNKNOWN) == ["m"] and r.to_json()["open"] == {"unknown": {"0": 1}}
    assert class_of(a) == class_of(b) == class_of(c) == UNKNOWN


def test_other_frames_count_in_frames_only():
    data = frames([(STATUS_ID, body(b"m", 1)), (9, progress_body(b"m", 2, 5, b"a")), (PROGRESS_ID, b"\x2e"),
                   (STATUS_ID, b"\x2e"), (PROGRESS_ID, progress_body(b"m", 2, 5, b"a")), (0, b"x")])
    r = stages_cpu(data)
    assert (r.frames, r.status_events, r.progress_events, r.status_decode_errors, r.progress_decode_errors) == \
        (6, 1, 1, 1, 1)
    assert r.media == {"m": MediaStand({}, None, 2, (0, 1, 1, 5))}
    # the worker string takes no part
    assert stages_cpu(frames([(PROGRESS_ID, progress_body(b"m", 2, 5, b"a")), (PROGRESS_ID, progress_body(b"m", 2, 5))])) \
        .media == {"m": MediaStand({2: 2}, 5, 2, None)}


def test_course_of_is_the_rule():
    names = replay.status_names()
    course = course_of([(3, PROGRESS, 2, 5), (7, STATUS, 9, 0), (8, PROGRESS, 2, 100), (9, STATUS, 2, 0)], names)
    assert course.stand == MediaStand({2: 1}, 5, 4, (9, 2, 0, None))
    assert (course.entered, course.matrix, course.closed) == ({UNKNOWN: 1, 2: 1}, {(UNKNOWN, 2): 1}, {(UNKNOWN, "full"): 1})
    assert course.stages == [(UNKNOWN, 1, 100, True), (2, 0, None, False)]
    r = StageReport()
    r.add_course("m", course)
    r.add_course("n", course_of([(1, STATUS, 2, 0)], names))
    r.add_course("m", course, sign=-1)  # taken out again: what is left is n's
    assert r == StageReport(0, 1, 0, 0, 0, {2: 1}, {}, {}, {"n": MediaStand({}, None, 1, (1, 2, 0, None))})
