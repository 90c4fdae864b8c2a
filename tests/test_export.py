"""``export`` (beholder_amd/export.py), the definition on the CPU: every row is valid JSON with its keys
in the spec's order; the rows are NDJSON input that gives back ``normalise``'s frames; the escapes are
``json.dumps``'s; results merge where the later base continues the earlier frames; ``export_file`` in
chunks equals one call; and the command line."""
from __future__ import annotations

import base64
import functools
import io
import json
import subprocess
import sys

import pytest

from beholder_amd import normalise as nm, ops, replay
from beholder_amd.coalesce import DROP, KEEP
from beholder_amd.export import Exported, Policy, export_cpu, export_file, row_of
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS, PROGRESS_ID, STATUS, STATUS_ID
from beholder_amd.transport.framing import iter_frames, ndjson_line_to_frame, ndjson_to_frames

import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus, varint  # noqa: E402

both = pytest.mark.parametrize("dialect", ops.DIALECTS)
OTHER = {"upb": "protobufjs", "protobufjs": "upb"}
TWO = {0x22: b'\\"', 0x5c: b"\\\\", 8: b"\\b", 9: b"\\t", 10: b"\\n", 12: b"\\f", 13: b"\\r"}  # the two-byte escapes
KEYS = {STATUS: ["mediaId", "status"], PROGRESS: ["mediaId", "status", "progress", "host"]}


@functools.lru_cache(maxsize=None)
def _stream(name: str) -> bytes:
    return fold_corpus() if name == "fold_corpus" else wire_edges.stream(6000)


def _str(field: int, value: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(value)) + value


def _rows(data: bytes) -> list:
    rows = data.split(b"\n")
    assert rows.pop() == b""  # every row ends in a newline, and none holds one
    return rows


@both
@pytest.mark.parametrize("name", ["fold_corpus", "wire_edges"])
def test_every_row_is_json_with_the_keys_in_order_and_gives_back_the_normalised_frame(name, dialect):
    data = _stream(name)
    events = list(iter_frames(data))
    got = export_cpu(data, Policy(), dialect)
    rows = _rows(got.data)
    assert got.frames == len(rows) == len(events) > 5000 and got.indices == list(range(len(events)))
    assert (got.base, got.dialect, got.undecoded) == (0, dialect, "keep")
    canon = nm.canon_of(nm.Policy("keep"), dialect)
    names = replay.status_names()
    decoded = 0
    two_topics = []
    for i, ((topic, body), row) in enumerate(zip(events, rows)):
        rec = json.loads(row)  # UTF-8
        assert rec["i"] == i
        if "json" in rec:
            decoded += 1
            assert list(rec) == ["i", "topic", "json", "name"] and rec["topic"] == {1: STATUS, 2: PROGRESS}[topic]
            assert list(rec["json"]) == KEYS[rec["topic"]]
            assert rec["name"] == names.get(rec["json"]["status"])
            assert canon(topic, body) is not KEEP
            want = (topic, canon(topic, body))
        else:
            assert list(rec) == ["i", "topic", "b64"]
            assert rec["topic"] == {1: STATUS, 2: PROGRESS}.get(topic, topic)
            assert base64.b64decode(rec["b64"], validate=True) == body
            assert canon(topic, body) is KEEP
            want = (topic, body)
        if topic in (STATUS_ID, PROGRESS_ID):  # the round-trip law: the row is NDJSON input to the service
            assert ndjson_line_to_frame(row.decode("utf-8")) == want
            two_topics.append((topic, body))
    assert got.events == decoded > 400
    sub = frames(two_topics)
    lines = export_cpu(sub, Policy(), dialect).data.decode("utf-8").splitlines()
    assert ndjson_to_frames(lines) == nm.normalise_cpu(sub, nm.Policy(), dialect).data
    dropped = export_cpu(data, Policy("drop"), dialect)
    assert _rows(dropped.data) == [row for row in rows if b'"json":{' in row[:64]]
    assert dropped.indices == [json.loads(r)["i"] for r in _rows(dropped.data)] and dropped.events == decoded
    assert (dropped.frames, dropped.undecoded) == (len(events), "drop")


@both
def test_the_escapes_are_json_dumps(dialect):
    row = row_of(Policy(), dialect)
    for c in range(0x80):
        s = chr(c)
        for topic, body, fields in ((PROGRESS_ID, _str(1, bytes([c])), {"mediaId": s, "status": 0, "progress": 0, "host": ""}),
                                    (PROGRESS_ID, _str(4, bytes([c])), {"mediaId": "", "status": 0, "progress": 0, "host": s}),
                                    (STATUS_ID, _str(1, bytes([c])), {"mediaId": s, "status": 0})):
            obj = {"i": 7, "topic": {1: STATUS, 2: PROGRESS}[topic], "json": fields, "name": "QUEUED"}
            want = json.dumps(obj, ensure_ascii=False, separators=(",", ":")).encode("utf-8") + b"\n"
            got = row(7, topic, body)
            assert got == want and json.loads(got) == obj
            key = b'"mediaId":"' if fields["mediaId"] else b'"host":"'
            assert key + TWO.get(c, b"\\u00%02x" % c if c < 0x20 else bytes([c])) + b'"' in got  # 0x7f as it is


def test_single_rows_written_out():
    row = row_of(Policy(), "protobufjs")
    assert row(0, STATUS_ID, b"") == b'{"i":0,"topic":"v1.telemetry.status","json":{"mediaId":"","status":0},"name":"QUEUED"}\n'
    assert row(12, PROGRESS_ID, b"\x0a\x01m\x10\x02\x18\x28\x22\x01h") == (
        b'{"i":12,"topic":"v1.telemetry.progress","json":{"mediaId":"m","status":2,"progress":40,"host":"h"},'
        b'"name":"CONVERTING"}\n')
    assert row(3, STATUS_ID, b"\x10\x06") == b'{"i":3,"topic":"v1.telemetry.status","json":{"mediaId":"","status":6},"name":null}\n'
    minus = b"\xff\xff\xff\xff\x0f"
    assert row(2 ** 53, PROGRESS_ID, b"\x10" + minus + b"\x18\x80\x80\x80\x80\x08") == (
        b'{"i":9007199254740992,"topic":"v1.telemetry.progress","json":{"mediaId":"","status":-1,'
        b'"progress":-2147483648,"host":""},"name":null}\n')
    assert row(1, STATUS_ID, b"\x2e") == b'{"i":1,"topic":"v1.telemetry.status","b64":"Lg=="}\n'
    assert row(1, PROGRESS_ID, b"\x2e\x00") == b'{"i":1,"topic":"v1.telemetry.progress","b64":"LgA="}\n'
    assert row(1, 9, b"\xfb\xff\xfe") == b'{"i":1,"topic":9,"b64":"+//+"}\n'
    assert row(1, 0, b"") == b'{"i":1,"topic":0,"b64":""}\n' and row(5, 255, b"abcd") == b'{"i":5,"topic":255,"b64":"YWJjZA=="}\n'
    assert row(1, PROGRESS_ID, b"\x0a\x02\xc3\xa9\x22\x02\xff\x41") == (
        '{"i":1,"topic":"v1.telemetry.progress","json":{"mediaId":"é","status":0,"progress":0,"host":"�A"},'
        '"name":"QUEUED"}\n').encode("utf-8")
    drop = row_of(Policy("drop"), "upb")
    assert drop(1, 9, b"x") is DROP and drop(1, STATUS_ID, b"\x2e") is DROP and drop(1, PROGRESS_ID, b"\x22\x01\xff") is DROP
    assert drop(1, STATUS_ID, b"") == row(1, STATUS_ID, b"")


def _forty() -> list:
    kinds = [(STATUS_ID, b"\x10\x00\x0a\x01m"), (PROGRESS_ID, b"\x18\x05\x10\x02\x0a\x01m"), (9, b"other"),
             (PROGRESS_ID, b"\x2e"), (STATUS_ID, b"\x0a\x03a\"b\x10\x03"), (STATUS_ID, b""), (PROGRESS_ID, b"\x0a\x02\xc3\xa9"),
             (PROGRESS_ID, b"\x10\xff\xff\xff\xff\x0f")]
    return kinds * 5


@both
@pytest.mark.parametrize("undecoded", ["keep", "drop"])
def test_merge_equals_the_whole_at_every_cut(dialect, undecoded):
    events = _forty()
    policy = Policy(undecoded)
    for base in (0, 95):  # the index takes a digit more inside the stream
        whole = export_cpu(frames(events), policy, dialect, base)
        assert whole.frames == 40 and whole.events == 30 and whole.base == base
        for cut in range(len(events) + 1):
            a = export_cpu(frames(events[:cut]), policy, dialect, base)
            b = export_cpu(frames(events[cut:]), policy, dialect, base + cut)
            before = (a.data, list(a.indices), b.data, list(b.indices))
            assert a.merge(b) == whole
            assert (a.data, a.indices, b.data, b.indices) == before
            if cut:
                with pytest.raises(ValueError, match="base"):
                    a.merge(export_cpu(frames(events[cut:]), policy, dialect, base))
                with pytest.raises(ValueError, match="base"):
                    a.merge(export_cpu(frames(events[cut:]), policy, dialect, base + cut + 1))
    with pytest.raises(ValueError):
        whole.merge(export_cpu(b"", policy, OTHER[dialect], whole.base + 40))
    with pytest.raises(ValueError):
        whole.merge(export_cpu(b"", Policy("drop" if undecoded == "keep" else "keep"), dialect, whole.base + 40))


@both
def test_export_file_in_chunks_equals_one_call(dialect):
    data = _stream("fold_corpus")
    assert len(data) > 7 * 30_000
    for undecoded in ("keep", "drop"):
        want = export_cpu(data, Policy(undecoded), dialect)
        for chunk_bytes in (30_000, 1 << 30):
            out, indices = io.BytesIO(), io.StringIO()
            counts = export_file(io.BytesIO(data), out, Policy(undecoded), "cpu", dialect, chunk_bytes, indices)
            assert out.getvalue() == want.data
            assert [int(line) for line in indices.getvalue().split()] == want.indices
            assert counts == {"frames": want.frames, "rows": len(want.indices), "out_bytes": len(want.data),
                              "in_bytes": len(data), "events": want.events, "undecoded": want.frames - want.events,
                              "host_frames": 0}


def test_each_chunk_is_written_before_the_next_is_read():
    data = frames(_forty() * 4)

    class Source(io.BytesIO):
        def read(self, size=-1):
            reads.append(out.tell())
            return super().read(size)
    reads, out = [], io.BytesIO()
    export_file(Source(data), out, chunk_bytes=64)
    assert len(reads) > 5 and reads[0] == 0 and reads == sorted(reads) and len(set(reads)) > 5


def test_a_truncated_tail_leaves_whole_rows_and_raises():
    events = _forty()
    data = frames(events)
    for lost in (1, 3, 9):
        out, indices = io.BytesIO(), io.StringIO()
        with pytest.raises(ValueError):
            export_file(io.BytesIO(data[:-lost]), out, chunk_bytes=16, indices_out=indices)
        assert out.getvalue() == export_cpu(frames(events[:-1])).data
        assert indices.getvalue().split() == [str(i) for i in range(len(events) - 1)]
    with pytest.raises(ValueError):
        export_cpu(data[:-1])
    with pytest.raises(ValueError):
        export_cpu(data + b"\0\0\0\0\x01")  # an empty frame


def test_argument_validation():
    for call in (lambda: row_of("keep"), lambda: export_cpu(b"", "keep"),
                 lambda: export_file(io.BytesIO(b""), io.BytesIO(), "drop")):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        export_cpu(b"", Policy(), "proto2")
    with pytest.raises(ValueError):
        export_file(io.BytesIO(b""), io.BytesIO(), Policy(), dialect="proto2")
    for base in (-1, 1.0, True, 2 ** 62 + 1):
        with pytest.raises(ValueError):
            export_cpu(b"", Policy(), "upb", base)
    assert export_cpu(b"") == Exported() and export_cpu(b"", Policy("drop"), "upb", 7) == Exported(
        base=7, dialect="upb", undecoded="drop")
    assert Policy is nm.Policy


def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", "export", *args], input=stdin, capture_output=True,
                          timeout=120)


def test_the_command_line_on_the_cpu(tmp_path):
    events = _forty()
    data = frames(events)
    source, out, indices = tmp_path / "in.bin", tmp_path / "out.ndjson", tmp_path / "indices.txt"
    source.write_bytes(data)
    for dialect in ops.DIALECTS:
        want = export_cpu(data, Policy("drop"), dialect)
        r = _cli(str(source), "-o", str(out), "--indices", str(indices), "--undecoded", "drop", "--dialect", dialect,
                 "--chunk-bytes", "50")
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == want.data and r.stdout == b""
        assert [int(line) for line in indices.read_text().split()] == want.indices
        counts = json.loads(r.stderr.decode().strip().splitlines()[-1])
        assert counts == {"frames": want.frames, "rows": len(want.indices), "out_bytes": len(want.data),
                          "in_bytes": len(data), "events": want.events, "undecoded": want.frames - want.events,
                          "host_frames": 0}
    r = _cli(stdin=data)  # stdin to stdout, the defaults
    assert r.returncode == 0 and r.stdout == export_cpu(data).data
    assert json.loads(r.stderr.decode().strip().splitlines()[-1])["rows"] == 40
    r = _cli("-o", str(out), stdin=data[:-2])  # whole rows only, and exit code 1
    assert r.returncode == 1 and out.read_bytes() == export_cpu(frames(events[:-1])).data
    assert b"truncated" in r.stderr
    assert _cli("--undecoded", "first", stdin=data).returncode == 2
    assert _cli("--device", "tpu", stdin=data).returncode == 2


def test_cli_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    from beholder_amd.ops import hip_lib
    path = tmp_path / "capture.bin"
    path.write_bytes(frames(_forty()))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["export", str(path), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device gpu is not available" in out.err and "--device cpu" in out.err and not out.out
    # and with a device but no library
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "libbeholder_hip.so"))
    monkeypatch.setattr(hip_lib, "_lib", None)
    assert cli.main(["export", str(path), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device cpu" in out.err and "missing" in out.err and not out.out


def test_the_default_chunk_leaves_room_for_the_rows():
    """The rows of the corpora take 3.1 and 5.2 times the input: a default chunk's rows stay below 2^31."""
    from beholder_amd import cli, export
    assert cli.build_parser().parse_args(["export"]).chunk_bytes == export.DEFAULT_CHUNK_BYTES == 64 << 20
    for name in ("fold_corpus", "wire_edges"):
        data = _stream(name)
        ratio = len(export_cpu(data).data) / len(data)
        assert 3.0 < ratio < 5.5 and ratio * export.DEFAULT_CHUNK_BYTES < 2 ** 31
