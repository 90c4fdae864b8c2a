"""The stream fold (beholder_amd/replay.py): ``fold_cpu`` is the definition of what a captured
stream does to the service's counters, comments and media rows. These tests pin it to the service
itself and to the service's codecs, check that summaries merge, and cover the host pieces of the
GPU path that need no device: ``frame_index``, the CLI, the HIP build stamp."""
from __future__ import annotations

import asyncio
import io
import json
import re
import struct
import subprocess
import sys

import pytest

from beholder_amd import _build, ops, replay
from beholder_amd.bench.generator import Workload, bench_config
from beholder_amd.models import proto
from beholder_amd.ops import frames, native
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

STATUS_T = proto.load("api.TelemetryStatus")
PROGRESS_T = proto.load("api.TelemetryProgress")
STATUS = ops.codec_for(STATUS_T)
PROGRESS = ops.codec_for(PROGRESS_T)


def _offsets(buf: bytes) -> list:
    out, i = [], 0
    for _, body in iter_frames(buf):
        out.append(i)
        i += 5 + len(body)
    return out + [i]


def _index(buf) -> tuple:
    n, raw = native.frame_index(buf)
    return n, list(memoryview(raw).cast("i"))


def test_the_fold_predicts_the_service():
    from beholder_amd.config import Config
    from beholder_amd.service import Service
    from beholder_amd.sinks import RecordingHttpClient
    from beholder_amd.store import MemoryStore
    from beholder_amd.transport.ingest import BytesSource
    from beholder_amd.utils.log import Logger, MemoryStream

    w = Workload(n_media=16, seed=3, unknown_media_fraction=0.1)
    data = w.framed(3000)
    summary = replay.fold_cpu(data)
    known = {m.id for m in w.media}
    unacked = sum(f.status_events for mid, f in summary.media.items() if mid not in known)
    store = MemoryStore(w.media)

    async def go():
        svc = Service(Config.from_dict(bench_config()), source=BytesSource(data), store=store,
                      http=RecordingHttpClient(), logger=Logger(stream=MemoryStream()), serve_metrics=False)
        await svc.init()
        # status events for unknown media are never acked (Q1): the run ends only while they fit the window
        assert 0 < unacked < svc.prefetch, (unacked, svc.prefetch)
        await svc.run()
        text = svc.registry.render()
        await svc.close()
        return text

    text = asyncio.run(go())
    counters = {m.group(1): int(float(m.group(2))) for m in
                re.finditer(r'^beholder_progress_updates_total\{status="([^"]*)"\} (\S+)$', text, re.M)}
    comments = int(float(re.search(r"^beholder_trello_comments (\S+)$", text, re.M).group(1)))
    prediction = summary.apply(w.media)
    assert prediction["progress_updates"] == counters and sum(counters.values()) > 2000
    assert prediction["trello_comments"] == comments and comments > 500
    assert prediction["statuses"] == {mid: row.status for mid, row in store.snapshot().items()}
    assert summary.frames == 3000 and not summary.status_decode_errors and not summary.progress_decode_errors


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("body", [b"\x1a\x02\x10\x04", b"\x22\x01"])
def test_status_frames_use_the_status_parser(body, dialect):
    """Fields 3 and 4 are unknown fields of a TelemetryStatus: each topic goes by its own codec."""
    s = replay.fold_cpu(frames([(STATUS_ID, body), (PROGRESS_ID, body)]), dialect)
    want = replay.Summary(frames=2)
    names = replay.status_names()
    for topic, ptype in ((STATUS_ID, STATUS_T), (PROGRESS_ID, PROGRESS_T)):
        try:
            m = ops.codec_for(ptype, dialect).decode(body)
        except proto.DecodeError:
            if topic == STATUS_ID:
                want.status_decode_errors += 1
            else:
                want.progress_decode_errors += 1
            continue
        fold = want.media.setdefault(m.mediaId, replay.MediaFold())
        if topic == STATUS_ID:
            fold.status_events, fold.last_status, fold.last_status_index = 1, m.status, 0
        else:
            fold.progress_events = fold.progress_counted = 1
            want.progress_updates[names[m.status].lower()] = 1
    assert s == want


def test_the_two_parsers_differ_where_the_issue_says():
    s = replay.fold_cpu(frames([(STATUS_ID, b"\x1a\x02\x10\x04"), (PROGRESS_ID, b"\x1a\x02\x10\x04"),
                                (STATUS_ID, b"\x22\x01"), (PROGRESS_ID, b"\x22\x01")]))
    assert s.media[""] == replay.MediaFold(status_events=1, progress_events=2, progress_counted=2,
                                           last_status=0, last_status_index=0)
    assert s.status_decode_errors == 1 and s.progress_decode_errors == 0
    assert s.progress_updates == {replay.status_names()[4].lower(): 1, replay.status_names()[0].lower(): 1}


def _merge_stream() -> list:
    """Media "both" has status events on both sides of the middle, "early" only before it, "late"
    only after it, "never" none at all."""
    ev = []
    for k in range(40):
        first = k < 20
        ev.append((PROGRESS_ID, PROGRESS.encode({"mediaId": "never", "status": k % 6, "progress": k})))
        ev.append((STATUS_ID, STATUS.encode({"mediaId": "both", "status": k % 5})))
        ev.append((STATUS_ID, STATUS.encode({"mediaId": "early" if first else "late", "status": (k + 1) % 5})))
        ev.append((PROGRESS_ID, PROGRESS.encode({"mediaId": "both", "status": 9, "progress": 1})))
        ev.append((7, b"x"))
        ev.append((STATUS_ID, b"\x22\x01"))
    return ev


def test_summaries_merge_at_any_frame_boundary():
    ev = _merge_stream() + Workload(n_media=8, seed=4).events(200)
    whole = replay.fold_cpu(frames(ev))
    assert whole.media["early"].last_status_index < 120 < whole.media["late"].last_status_index
    assert whole.media["never"].last_status is None and whole.other_topic == 40
    for cut in (0, 1, 2, 3, 119, 120, 121, 239, 240, 300, len(ev) - 1, len(ev)):
        a, b = replay.fold_cpu(frames(ev[:cut])), replay.fold_cpu(frames(ev[cut:]))
        assert a.merge(b) == whole, cut
        assert a.frames == cut and b.frames == len(ev) - cut
    thirds = [replay.fold_cpu(frames(ev[i:i + 150])) for i in range(0, len(ev), 150)]
    total = replay.Summary()
    for part in thirds:
        total = total.merge(part)
    assert total == whole


def test_fold_file_in_small_chunks_equals_the_one_shot_fold(tmp_path):
    data = Workload(n_media=32, seed=6, unknown_media_fraction=0.05).framed(3000)
    assert 120_000 < len(data) < 200_000
    path = tmp_path / "capture.bin"
    path.write_bytes(data)
    whole = replay.fold_cpu(data)
    assert replay.fold_file(str(path), chunk_bytes=4096) == whole
    assert replay.fold_file(io.BytesIO(data), chunk_bytes=1) == whole  # every frame a chunk of its own
    assert replay.fold_file(path) == whole
    chunks = list(replay.iter_chunks(io.BytesIO(data), 4096))
    assert b"".join(chunks) == data and len(chunks) > 30 and all(0 < len(c) <= 4096 for c in chunks)
    with pytest.raises(ValueError):
        replay.fold_file(io.BytesIO(data[:-1]), chunk_bytes=4096)
    with pytest.raises(ValueError):
        replay.fold_file(io.BytesIO(data + b"\x01\x00"), chunk_bytes=4096)


def test_frame_index_equals_the_python_splitter():
    data = Workload(n_media=8, seed=2).framed(500)
    n, offs = _index(data)
    assert n == 500 and offs == _offsets(data) and offs[-1] == len(data)
    assert _index(b"") == (0, [0])
    assert _index(bytearray(frames([(1, b"")]))) == (1, [0, 5])
    assert _index(memoryview(frames([(2, b"abc")]))) == (1, [0, 8])
    assert _index(frames([(2, b"abc")]) * 3) == (3, [0, 8, 16, 24])


@pytest.mark.parametrize("bad", [b"\x01\x00\x00", struct.pack("<I", 0), frames([(1, b"ab")])[:-1],
                                 frames([(1, b"ab")]) + b"\x02", frames([(1, b"ab")]) + struct.pack("<I", 0)])
def test_frame_index_raises_where_iter_frames_does(bad):
    with pytest.raises(ValueError):
        list(iter_frames(bad))
    with pytest.raises(ValueError):
        native.frame_index(bad)


def test_frame_index_partial_stops_at_the_last_whole_frame():
    two = frames([(1, b"ab"), (2, b"")])
    n, raw = native.frame_index(two + b"\x09\x00\x00\x00\x01abc", True)
    assert n == 2 and list(memoryview(raw).cast("i")) == [0, 7, 12]
    n, raw = native.frame_index(two + b"\x09", True)
    assert n == 2 and list(memoryview(raw).cast("i")) == [0, 7, 12]
    with pytest.raises(ValueError):
        native.frame_index(two + struct.pack("<I", 0), True)


def test_media_identity_is_the_decoded_string():
    def status(mid: bytes, st: int):
        return STATUS_ID, b"\x0a" + bytes([len(mid)]) + mid + bytes([0x10, st])
    s = replay.fold_cpu(frames([status(b"\xff", 1), status(b"\xfe", 2), status("é".encode(), 3),
                                (STATUS_ID, b"\x10\x04"), status(b"", 5)]))
    assert set(s.media) == {"�", "é", ""}
    assert s.media["�"] == replay.MediaFold(status_events=2, last_status=2, last_status_index=1)
    assert s.media["é"].status_events == 1
    assert s.media[""] == replay.MediaFold(status_events=2, last_status=5, last_status_index=4)


def test_apply_leaves_untouched_rows_and_counts_trello_comments_only():
    w = Workload(n_media=4, seed=1)
    trello = next(m for m in w.media if m.creator == 1)
    other = next(m for m in w.media if m.creator != 1)
    ev = [(PROGRESS_ID, PROGRESS.encode({"mediaId": trello.id, "status": 2, "progress": 5}))] * 3
    ev += [(PROGRESS_ID, PROGRESS.encode({"mediaId": trello.id, "status": 77}))]  # Q6: no count, no comment
    ev += [(PROGRESS_ID, PROGRESS.encode({"mediaId": other.id, "status": 2}))]
    ev += [(STATUS_ID, STATUS.encode({"mediaId": other.id, "status": 77}))]  # written as it is
    out = replay.fold_cpu(frames(ev)).apply(w.media)
    assert out["trello_comments"] == 3 and out["progress_updates"] == {"converting": 4}
    assert out["statuses"] == {m.id: 77 if m.id == other.id else m.status for m in w.media}


def test_json_round_trip_sorts_media():
    s = replay.fold_cpu(frames(_merge_stream()))
    obj = json.loads(json.dumps(s.to_json()))
    assert list(obj["media"]) == sorted(s.media) and replay.Summary.from_json(obj) == s


def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_cli_summarise_cpu_round_trips(tmp_path):
    w = Workload(n_media=8, seed=5)
    data = w.framed(400)
    path, fixture = tmp_path / "capture.bin", tmp_path / "media.json"
    path.write_bytes(data)
    fixture.write_text(json.dumps([m._asdict() for m in w.media]))
    r = _cli("summarise", str(path), "--device", "cpu", "--media-fixture", str(fixture), "--chunk-bytes", "5000")
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    want = replay.fold_cpu(data)
    assert replay.Summary.from_json(out["summary"]) == want
    assert out["prediction"] == json.loads(json.dumps(want.apply(w.media)))
    r = _cli("summarise", stdin=data)  # stdin, default device
    assert r.returncode == 0 and replay.Summary.from_json(json.loads(r.stdout)["summary"]) == want


def test_cli_summarise_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    from beholder_amd.ops import hip_lib
    path = tmp_path / "capture.bin"
    path.write_bytes(Workload(n_media=2, seed=5).framed(10))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["summarise", str(path), "--device", "gpu"]) != 0
    out = capsys.readouterr()
    assert "--device cpu" in out.err and "no GPU" in out.err and not out.out
    # and with a device but no library
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "libbeholder_hip.so"))
    monkeypatch.setattr(hip_lib, "_lib", None)
    assert cli.main(["summarise", str(path), "--device", "gpu"]) != 0
    out = capsys.readouterr()
    assert "--device cpu" in out.err and "missing" in out.err and not out.out


def test_hip_stamp_follows_the_headers(tmp_path):
    (tmp_path / "k.hip").write_text('#include "r.hpp"\n')
    (tmp_path / "r.hpp").write_text("// one\n")
    first = _build.hip_source_hash(str(tmp_path))
    assert first == _build.hip_source_hash(str(tmp_path))
    (tmp_path / "r.hpp").write_text("// two\n")
    second = _build.hip_source_hash(str(tmp_path))
    assert second != first
    (tmp_path / "k.hip").write_text('#include "r.hpp"\n\n')
    assert _build.hip_source_hash(str(tmp_path)) != second
    assert _build.hip_source_hash() == _build.hip_source_hash(_build.HIP_DIR)
