"""``extract`` on the CPU (beholder_amd/extract.py): the definition the device path is held to, its
laws (partition, concatenation, the fold of an extract) and the command. Every comparison is exact:
bytes and integers."""
from __future__ import annotations

import functools
import io
import json
import subprocess
import sys

import pytest

from beholder_amd import extract as ex, ops, replay
from beholder_amd.bench.generator import Workload
from beholder_amd.extract import Extract, Selector, extract_cpu
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames
from extract_cases import FFFD, FFFD3, KINDS, M3, M7
from telemetry_corpus import body as _body, fold_corpus as _corpus


@functools.lru_cache(maxsize=None)
def _fold(dialect: str) -> replay.Summary:
    return replay.fold_cpu(_corpus(), dialect)


def _frame_list(data: bytes) -> list:
    return [ops.frame(t, b) for t, b in iter_frames(data)]


def test_the_corpus_has_the_media_the_selectors_name():
    assert {"", FFFD3, M3, M7} <= set(_fold("protobufjs").media)


def test_the_empty_selector_keeps_everything_and_its_inverse_nothing():
    data = _corpus()
    n = _fold("protobufjs").frames
    assert extract_cpu(data, Selector()) == Extract(data, list(range(n)), n)
    assert extract_cpu(data, Selector(invert=True)) == Extract(b"", [], n)
    assert extract_cpu(b"", Selector()) == Extract() == extract_cpu(b"", Selector(invert=True))


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("kind", sorted(set(KINDS) - {"all"}))
def test_a_selector_and_its_inverse_partition_the_stream(kind, dialect):
    import dataclasses
    data = _corpus()
    yes = extract_cpu(data, KINDS[kind], dialect)
    no = extract_cpu(data, dataclasses.replace(KINDS[kind], invert=not KINDS[kind].invert), dialect)
    assert yes.frames == no.frames == _fold(dialect).frames
    assert yes.indices and no.indices, "the corpus exercises both sides of every kind"
    assert sorted(yes.indices) == yes.indices and sorted(no.indices) == no.indices
    assert not set(yes.indices) & set(no.indices)
    assert sorted(yes.indices + no.indices) == list(range(yes.frames))
    rebuilt = dict(zip(yes.indices, _frame_list(yes.data)))
    rebuilt.update(zip(no.indices, _frame_list(no.data)))
    assert b"".join(rebuilt[i] for i in range(yes.frames)) == data


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_counts_against_the_fold(dialect):
    data, fold = _corpus(), _fold(dialect)
    assert fold.status_decode_errors and fold.progress_decode_errors and fold.progress_unknown_status

    def count(**fields):
        return len(extract_cpu(data, Selector(**fields), dialect).indices)
    assert count(topics={STATUS_ID}, outcomes={"error"}) == fold.status_decode_errors
    assert count(topics={PROGRESS_ID}, outcomes={"error"}) == fold.progress_decode_errors
    assert count(outcomes={"other"}) == fold.other_topic == 15
    assert count(topics={PROGRESS_ID}, unknown_status=True) == fold.progress_unknown_status
    assert count(outcomes={"decoded"}) == sum(m.status_events + m.progress_events for m in fold.media.values())


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_fold_of_one_medias_extract_is_its_row_of_the_whole_fold(dialect):
    data, fold = _corpus(), _fold(dialect)
    busiest = max(fold.media, key=lambda m: fold.media[m].status_events + fold.media[m].progress_events)
    assert fold.media[busiest].status_events + fold.media[busiest].progress_events >= 20
    chosen = ["", busiest, M3] + ([FFFD3] if dialect == "protobufjs" else [])
    for mid in chosen:
        cut = extract_cpu(data, Selector(media={mid}), dialect)
        sub = replay.fold_cpu(cut.data, dialect)
        assert set(sub.media) == {mid} and sub.frames == len(cut.indices)
        assert not (sub.status_decode_errors or sub.progress_decode_errors or sub.other_topic)
        got, want = sub.media[mid], fold.media[mid]
        assert (got.status_events, got.progress_events, got.progress_counted, got.last_status) == \
            (want.status_events, want.progress_events, want.progress_counted, want.last_status), mid
        if want.last_status_index is None:
            assert got.last_status_index is None
        else:
            assert cut.indices[got.last_status_index] == want.last_status_index


def test_the_replacement_character_is_one_media_under_protobufjs_and_none_under_upb():
    data = frames([(STATUS_ID, _body(b"\xff", 1)), (PROGRESS_ID, _body(b"\xfe", 2)),
                   (PROGRESS_ID, _body("é".encode(), 3)), (STATUS_ID, _body(b"plain", 4))])
    assert extract_cpu(data, Selector(media={FFFD})).indices == [0, 1]
    assert extract_cpu(data, Selector(media={"é"})).indices == [2]
    assert extract_cpu(data, Selector(media={FFFD}), "upb").indices == []  # upb raises on invalid UTF-8
    assert extract_cpu(data, Selector(outcomes={"error"}), "upb").indices == [0, 1]


def test_status_selection_applies_to_either_topic_and_only_to_decoded_frames():
    data = frames([(STATUS_ID, _body(b"m", 3)), (PROGRESS_ID, _body(b"m", 3)), (PROGRESS_ID, _body(b"m", 64)),
                   (STATUS_ID, _body(b"m", -1)), (9, _body(b"m", 3)), (PROGRESS_ID, b"\x2e"), (STATUS_ID, b"")])
    assert 3 in replay.status_names() and 0 in replay.status_names()
    assert extract_cpu(data, Selector(statuses={3})).indices == [0, 1]
    assert extract_cpu(data, Selector(unknown_status=True)).indices == [2, 3]
    assert extract_cpu(data, Selector(statuses={3}, unknown_status=True)).indices == [0, 1, 2, 3]
    assert extract_cpu(data, Selector(statuses={0})).indices == [6]  # an empty message decodes to status 0
    assert extract_cpu(data, Selector(statuses=set())).indices == []
    assert extract_cpu(data, Selector(statuses={3}, invert=True)).indices == [2, 3, 4, 5, 6]


@pytest.mark.parametrize("kind", ["media", "outcome-error", "statuses-or-unknown"])
def test_extracts_concatenate_at_every_frame_boundary(kind):
    selector = KINDS[kind]
    pieces = _frame_list(_corpus())[:300]
    whole = extract_cpu(b"".join(pieces), selector)
    assert whole.frames == 300 and 0 < len(whole.indices) < 300
    for cut in range(301):
        a, b = b"".join(pieces[:cut]), b"".join(pieces[cut:])
        assert extract_cpu(a, selector) + extract_cpu(b, selector) == whole, cut


@pytest.mark.parametrize("chunk_bytes", [5000, 1])
def test_extract_file_in_chunks_equals_the_whole_buffer_call(chunk_bytes, tmp_path):
    data = _whole_prefix(_corpus()[:60_000]) if chunk_bytes == 1 else _corpus()  # one frame per chunk is slow
    selector = KINDS["media"]
    want = extract_cpu(data, selector)
    assert want.indices
    out, indices = io.BytesIO(), io.StringIO()
    counts = ex.extract_file(io.BytesIO(data), out, selector, chunk_bytes=chunk_bytes, indices_out=indices)
    assert out.getvalue() == want.data
    assert [int(line) for line in indices.getvalue().split()] == want.indices
    assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data), "host_frames": 0}
    path = tmp_path / "capture.bin"
    path.write_bytes(data)
    out = io.BytesIO()
    assert ex.extract_file(str(path), out, selector, chunk_bytes=chunk_bytes) == counts and out.getvalue() == want.data


def _whole_prefix(data: bytes) -> bytes:
    """``data`` cut back to its last whole frame."""
    i = 0
    while i + 4 <= len(data):
        end = i + 4 + int.from_bytes(data[i:i + 4], "little")
        if end > len(data):
            break
        i = end
    return data[:i]


def test_bad_arguments_raise():
    data = frames([(STATUS_ID, _body(b"m", 1))])
    with pytest.raises(ValueError):
        extract_cpu(data, Selector(statuses={64}))
    with pytest.raises(ValueError):
        extract_cpu(data, Selector(statuses={-1}))
    with pytest.raises(ValueError):
        extract_cpu(data, Selector(topics={256}))
    with pytest.raises(ValueError):
        extract_cpu(data, Selector(outcomes={"failed"}))
    with pytest.raises(ValueError):
        extract_cpu(data, Selector(), dialect="proto2")
    with pytest.raises(ValueError):
        ex.extract_file(io.BytesIO(data), io.BytesIO(), Selector(), dialect="proto2")
    with pytest.raises(ValueError):
        extract_cpu(data[:-1], Selector())
    with pytest.raises(ValueError):
        extract_cpu(data + b"\x01\x00", Selector())


# ---- the command ------------------------------------------------------------------------------------

def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_cli_extract_then_summarise_is_the_restricted_summary(tmp_path):
    data = Workload(n_media=8, seed=5).framed(400)
    whole = replay.fold_cpu(data)
    mid = sorted(whole.media)[2]
    capture, cut, indices = tmp_path / "capture.bin", tmp_path / "cut.bin", tmp_path / "indices.txt"
    capture.write_bytes(data)
    r = _cli("extract", str(capture), "--media", mid, "-o", str(cut), "--indices", str(indices), "--chunk-bytes", "5000")
    assert r.returncode == 0 and not r.stdout, r.stderr
    want = extract_cpu(data, Selector(media={mid}))
    assert cut.read_bytes() == want.data
    assert [int(line) for line in indices.read_text().split()] == want.indices
    assert json.loads(r.stderr) == {"frames": 400, "kept": len(want.indices), "kept_bytes": len(want.data),
                                    "host_frames": 0}
    r = _cli("summarise", str(cut))
    assert r.returncode == 0, r.stderr
    sub = replay.Summary.from_json(json.loads(r.stdout)["summary"])
    row = whole.media[mid]
    assert set(sub.media) == {mid} and sub.frames == row.status_events + row.progress_events
    got = sub.media[mid]
    assert (got.status_events, got.progress_events, got.progress_counted, got.last_status) == \
        (row.status_events, row.progress_events, row.progress_counted, row.last_status)
    assert want.indices[got.last_status_index] == row.last_status_index


def test_cli_extract_stdin_to_stdout_with_names_and_a_media_file(tmp_path):
    data = _corpus()
    names = replay.status_names()
    listed = tmp_path / "media.txt"
    listed.write_text(f"{M3}\n\n{M7}\n", encoding="utf-8")
    r = _cli("extract", "-o", "-", "--topic", "progress", "--status", names[2].lower(), "--status", "4",
             "--media-file", str(listed), "--media", FFFD3, stdin=data)
    assert r.returncode == 0, r.stderr
    want = extract_cpu(data, Selector(topics={PROGRESS_ID}, statuses={2, 4},
                                      media={M3, "", M7, FFFD3}))
    assert want.indices and r.stdout == want.data
    assert json.loads(r.stderr)["kept"] == len(want.indices)
    r = _cli("extract", "-o", "-", "--topic", "7", "--topic", "status", "--outcome", "error", "--outcome", "other",
             "--unknown-status", "--invert", "--dialect", "upb", stdin=data)
    assert r.returncode == 0, r.stderr
    assert r.stdout == extract_cpu(data, Selector(topics={7, STATUS_ID}, outcomes={"error", "other"},
                                                  unknown_status=True, invert=True), "upb").data
    assert _cli("extract", "-o", "-", "--status", "64", stdin=data).returncode == 2
    assert _cli("extract", "-o", "-", "--status", "nonsense", stdin=data).returncode == 2
    assert _cli("extract", "-o", "-", "--topic", "256", stdin=data).returncode == 2


def test_cli_extract_truncated_input_leaves_whole_frames(tmp_path):
    data = Workload(n_media=4, seed=5).framed(50)
    out = tmp_path / "cut.bin"
    r = _cli("extract", "-o", str(out), "--chunk-bytes", "700", stdin=data[:-3])
    assert r.returncode == 1 and b"truncated" in r.stderr
    written = out.read_bytes()
    assert written == _whole_prefix(data[:-3]) and len(list(iter_frames(written))) == 49


def test_cli_extract_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    from beholder_amd.ops import hip_lib
    path, out = tmp_path / "capture.bin", tmp_path / "cut.bin"
    path.write_bytes(Workload(n_media=2, seed=5).framed(10))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["extract", str(path), "-o", str(out), "--device", "gpu"]) != 0
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "no GPU" in err.err and not err.out and not out.exists()
    # and with a device but no library
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "libbeholder_hip.so"))
    monkeypatch.setattr(hip_lib, "_lib", None)
    assert cli.main(["extract", str(path), "-o", str(out), "--device", "gpu"]) != 0
    err = capsys.readouterr()
    assert "--device cpu" in err.err and "missing" in err.err and not err.out and not out.exists()
