"""``import`` (beholder_amd/import_rows.py): NDJSON rows back into a framed stream, on the CPU. The
law that makes it the inverse of ``export``, agreement with the service's own line reader, the rows
one by one, the malformed ones, chunking and the command line."""
from __future__ import annotations

import io
import json
import subprocess
import sys

import pytest

from beholder_amd import import_rows as im, normalise as nm, ops
from beholder_amd.import_rows import Imported, MalformedRow, Policy, frame_of_row, import_cpu, import_file
from beholder_amd.normalise import frame_of
from beholder_amd.topics import PROGRESS, STATUS
from beholder_amd.transport.framing import ndjson_line_to_frame

import import_cases as cases  # noqa: E402

SKIP = Policy("skip")


def _frame(line: bytes) -> bytes:
    return frame_of_row()(line)


# ---- the law -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", cases.CORPORA)
def test_import_of_an_export_is_the_normalise(name, dialect):
    x = cases.corpus(name)
    for undecoded in ("keep", "drop"):
        e = cases.exported(name, dialect, undecoded)
        got = import_cpu(e.data)
        want = nm.normalise_cpu(x, nm.Policy(undecoded), dialect)
        assert got.data == want.data
        rows = len(e.indices)
        assert rows > 300 and got.lines == list(range(rows)) and got.line_count == rows and not got.skipped
        assert (got.events, got.carried) == (e.events, rows - e.events)
        assert import_cpu(e.data, SKIP, 5).data == want.data
    assert cases.exported(name, dialect).frames - cases.exported(name, dialect).events > 0  # other topics and errors came back


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", cases.CORPORA)
def test_agrees_with_the_services_reader_on_the_two_topics(name, dialect):
    frame = frame_of_row()
    seen = 0
    for line in cases.exported(name, dialect).data.split(b"\n")[:-1]:
        if isinstance(json.loads(line)["topic"], str):
            assert frame(line) == frame_of(*ndjson_line_to_frame(line.decode("utf-8")))
            seen += 1
    assert seen > 300


def test_agrees_with_the_services_reader_on_hand_written_rows():
    rows = ['{"topic": "v1.telemetry.progress", "json": {"mediaId": "m", "status": "DEPLOYED", "progress": 5}}',
            '{"topic": "v1.telemetry.status", "b64": "CgFt"}']
    for row in rows:
        assert _frame(row.encode()) == frame_of(*ndjson_line_to_frame(row))
    assert _frame(rows[0].encode()) == frame_of(2, b"\x0a\x01m\x10\x04\x18\x05")
    assert _frame(rows[1].encode()) == frame_of(1, b"\x0a\x01m")


# ---- row by row ----------------------------------------------------------------------------------

def test_numeric_topics():
    for topic in (0, 9, 255, 1, 2):
        assert _frame(cases.b64_row(topic, b"\x00\xffbody")) == frame_of(topic, b"\x00\xffbody")
    assert _frame(cases.b64_row(STATUS, b"x")) == frame_of(1, b"x") and _frame(cases.b64_row(PROGRESS, b"")) == frame_of(2, b"")
    assert _frame(cases.event_row(1, "m", 3)) == _frame(cases.event_row(STATUS, "m", 3)) == frame_of(1, b"\x0a\x01m\x10\x03")
    assert _frame(cases.event_row(2, "m", 3, 40, "h")) == frame_of(2, b"\x0a\x01m\x10\x03\x18\x28\x22\x01h")


def test_key_order_whitespace_and_ignored_keys():
    want = frame_of(2, b"\x0a\x03m-1\x10\x02\x18\x28\x22\x01h")
    assert _frame(b'{"name":"CONVERTING","json":{"host":"h","progress":40,"status":2,"mediaId":"m-1"},'
                  b'"topic":"v1.telemetry.progress","i":7}') == want
    assert _frame(b'{ "i" : 3 , "topic" :\t"v1.telemetry.progress" , "json" : { "mediaId" : "m-1" , "status" : 2 , '
                  b'"progress" : 40 , "host" : "h" } , "name" : null }') == want
    for i, name in (("[1,{}]", '{"x":true}'), ("1.5e3", "false"), ('"seven"', "7"), ("null", '"ERRORED"')):  # name is not checked
        row = ('{"i":%s,"topic":"v1.telemetry.progress","json":{"mediaId":"m-1","status":2,"progress":40,"host":"h"},'
               '"name":%s,"extra":[1.0]}' % (i, name)).encode()
        assert _frame(row) == want
    assert _frame(cases.event_row(PROGRESS, "m-1", 2, 40, "h", i=None, name=None)) == want


def test_lines_crlf_blank_lines_and_a_missing_final_newline():
    a, b = cases.event_row(STATUS, "m", 3), cases.b64_row(9, b"xyz")
    want = _frame(a) + _frame(b)
    assert import_cpu(a + b"\n" + b + b"\n") == Imported(want, [0, 1], 2, 1, 1)
    assert import_cpu(a + b"\n" + b) == Imported(want, [0, 1], 2, 1, 1)                    # no final newline
    assert import_cpu(a + b"\r\n" + b + b"\r\n") == Imported(want, [0, 1], 2, 1, 1)         # CRLF
    got = import_cpu(b"\n \t\r\n" + a + b"\n\n\n  " + b + b" \t\n\r\n", base=10)
    assert got == Imported(want, [12, 15], 7, 1, 1, [], 10)                               # blank lines count
    assert import_cpu(b"") == Imported() and import_cpu(b"\n") == Imported(line_count=1)
    assert import_cpu(b"\n\n \n", SKIP, 3) == Imported(line_count=3, base=3, malformed="skip")
    u2028 = '{"topic":"v1.telemetry.status","json":{"mediaId":"a\u2028b"}}'.encode()  # raw in the row: no line ends there
    assert b"\xe2\x80\xa8" in u2028 and import_cpu(u2028 + b"\n" + u2028) == Imported(
        frame_of(1, b"\x0a\x05a\xe2\x80\xa8b") * 2, [0, 1], 2, 2, 0)


def test_status_by_name_defaults_and_the_smallest_frame():
    assert _frame(b'{"topic":"v1.telemetry.status","json":{"mediaId":"m1","status":"dePLoyed"}}') == frame_of(1, b"\x0a\x02m1\x10\x04")
    assert _frame(b'{"topic":"v1.telemetry.status","json":{"mediaId":"m1","status":"queued"}}') == frame_of(1, b"\x0a\x02m1")
    assert _frame(cases.event_row(PROGRESS, None, None, 5, None)) == frame_of(2, b"\x18\x05")
    assert _frame(cases.event_row(PROGRESS, None, None, None, "h")) == frame_of(2, b"\x22\x01h")
    for row in (cases.event_row(PROGRESS, "", 0, 0, ""), cases.event_row(STATUS), b'{"topic":2,"json":{}}',
                cases.event_row(PROGRESS, None, "-0", "-0", None)):
        assert _frame(row) in (b"\x01\x00\x00\x00\x01", b"\x01\x00\x00\x00\x02") and len(_frame(row)) == 5


def test_int32_extremes():
    ten = b"\xff" * 9 + b"\x01"
    assert _frame(cases.event_row(PROGRESS, None, -1, -2 ** 31)) == frame_of(2, b"\x10" + ten + b"\x18\x80\x80\x80\x80\xf8" + b"\xff" * 4 + b"\x01")
    assert _frame(cases.event_row(STATUS, None, 2 ** 31 - 1)) == frame_of(1, b"\x10\xff\xff\xff\xff\x07")
    assert _frame(cases.event_row(STATUS, None, -2 ** 31 + 1)) == frame_of(1, b"\x10\x81\x80\x80\x80\xf8" + b"\xff" * 4 + b"\x01")


def test_escapes():
    row = cases.event_row(PROGRESS, '\\"\\\\\\/\\b\\f\\n\\r\\t', 1, 2, '\\u0041\\u000a\\u007f\\u0000x')
    assert _frame(row) == frame_of(2, b"\x0a\x08\"\\/\b\f\n\r\t\x10\x01\x18\x02\x22\x05A\n\x7f\x00x")
    assert _frame(cases.event_row(STATUS, "\\ud83d\\ude00", 0)) == frame_of(1, b"\x0a\x04" + "\U0001f600".encode())
    assert _frame(cases.event_row(STATUS, "\\u00e9\\u20AC", 0)) == frame_of(1, b"\x0a\x05" + "é€".encode())


def test_b64_wins_and_is_carried_verbatim():
    assert _frame(b'{"topic":"v1.telemetry.status","b64":"CgFt","json":{"mediaId":"other","status":3}}') == frame_of(1, b"\x0a\x01m")
    assert _frame(b'{"topic":9,"json":"not even an object","b64":""}') == frame_of(9, b"")
    assert _frame(b'{"topic":9,"b64":"QR=="}') == frame_of(9, b"A") and _frame(b'{"topic":9,"b64":"QUH="}') == frame_of(9, b"AA")
    not_canonical = b"\x22\x01h\x10\x00\x0a\x01m\x38\x01"  # a body that normalise would rewrite stays as it is
    got = import_cpu(cases.b64_row(PROGRESS, not_canonical))
    assert got.data == frame_of(2, not_canonical) and (got.events, got.carried) == (0, 1)


def test_every_valid_row_is_one_frame():
    rows = cases.valid_rows() + cases.relaxed_rows() + cases.base64_rows() + cases.escape_rows()
    got = import_cpu(cases.text_of(rows))
    assert got.lines == list(range(len(rows))) and got.events + got.carried == len(rows)
    assert got.data == b"".join(map(_frame, rows))
    for size in cases.B64_SIZES:
        assert _frame(cases.b64_row(9, bytes(range(size)))) == frame_of(9, bytes(range(size)))


# ---- malformed -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(cases.malformed_rows())))
def test_a_malformed_row(k):
    bad = cases.malformed_rows()[k]
    good = cases.event_row(STATUS, "m", 3)
    with pytest.raises(MalformedRow):
        _frame(bad.strip(im.BLANK))
    text = good + b"\n\n" + bad + b"\n" + good + b"\n" + bad
    with pytest.raises(ValueError, match=r"^line 102: malformed row: ") as e:
        import_cpu(text, Policy("fail"), 100)
    assert not isinstance(e.value, MalformedRow)
    assert import_cpu(text, SKIP, 100) == Imported(_frame(good) * 2, [100, 103], 5, 2, 0, [102, 104], 100, "skip")


def test_reasons():
    for row, reason in ((b"not json", "not JSON"), (b"[1]", "JSON object"), (b'{"topic":256,"b64":""}', "unknown topic 256"),
                        (b'{"topic":9}', "'b64' or 'json'"), (b'{"topic":9,"json":{}}', "topic 9"),
                        (b'{"topic":1,"json":{"progress":1}}', "unknown field 'progress'"),
                        (b'{"topic":2,"json":{"status":1.0}}', "int32"), (b'{"topic":2,"json":{"status":"FLYING"}}', "unknown status"),
                        (b'{"topic":2,"json":{"host":"\\ud800"}}', "surrogate"), (b'{"topic":9,"b64":"QQ="}', "base64"),
                        (b"\xff", "UTF-8")):
        with pytest.raises(MalformedRow, match=reason):
            _frame(row)


def test_policy_and_arguments():
    assert Policy() == Policy("fail") and Policy("skip").malformed == "skip"
    with pytest.raises(ValueError):
        Policy("drop")
    with pytest.raises(TypeError):
        Policy(1)
    with pytest.raises(dataclasses_error()):
        Policy().malformed = "skip"
    with pytest.raises(TypeError):
        import_cpu(b"", "skip")
    with pytest.raises(TypeError):
        frame_of_row("skip")
    for base in (-1, 1.0, True, 2 ** 62 + 1):
        with pytest.raises(ValueError):
            import_cpu(b"", Policy(), base)
    with pytest.raises(ValueError):
        import_file(io.BytesIO(b""), io.BytesIO(), Policy(), chunk_bytes=0)


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


# ---- chunking ------------------------------------------------------------------------------------

def test_merge_laws():
    rows = cases.valid_rows()[:30] + [b"", b"not a row", b"  "] + cases.base64_rows()[:10]
    whole = import_cpu(cases.text_of(rows), SKIP, 7)
    for cut in (0, 1, 17, 31, 32, len(rows)):
        first = import_cpu(cases.text_of(rows[:cut]), SKIP, 7)
        later = import_cpu(cases.text_of(rows[cut:]), SKIP, 7 + cut)
        assert first.merge(later) == whole
        assert first.line_count == cut
    a, b, c = (import_cpu(cases.text_of(rows[k:k + 10]), SKIP, 7 + k) for k in (0, 10, 20))
    assert a.merge(b).merge(c) == a.merge(b.merge(c))
    assert whole.merge(Imported(base=7 + len(rows), malformed="skip")) == whole
    with pytest.raises(ValueError, match="base=17"):
        a.merge(c)
    with pytest.raises(ValueError, match="malformed"):
        a.merge(import_cpu(b"", Policy("fail"), 17))


def test_import_file_in_chunks_is_the_whole():
    long_row = cases.b64_row(9, bytes(range(256)) * 40)  # longer than any chunk below
    assert len(long_row) > 12_000
    rows = cases.valid_rows() + [b"", long_row, b"junk", long_row] + cases.escape_rows()[:200] + [b" ", long_row]
    for final in (True, False):
        text = cases.text_of(rows, final=final)
        whole = import_cpu(text, SKIP)
        for chunk_bytes in (1, 700, 3000, 5000, 1 << 30):
            out, lines = io.BytesIO(), io.StringIO()
            counts = import_file(io.BytesIO(text), out, SKIP, chunk_bytes=chunk_bytes, lines_out=lines)
            assert out.getvalue() == whole.data
            assert [int(k) for k in lines.getvalue().split()] == whole.lines
            assert counts == {"lines": len(rows), "rows": len(rows) - 2, "frames": len(whole.lines), "events": whole.events,
                              "carried": whole.carried, "skipped": 1, "blank": 2, "in_bytes": len(text),
                              "out_bytes": len(whole.data), "host_rows": 0}


def test_iter_line_chunks_cuts_after_the_last_newline():
    text = b"aa\nbbbb\nc\n" + b"d" * 30 + b"\ne\nf"
    for chunk_bytes in (1, 2, 3, 4, 8, 9, 10, 11, 40, 100):
        chunks = list(im.iter_line_chunks(io.BytesIO(text), chunk_bytes))
        assert b"".join(chunks) == text and all(c.endswith(b"\n") for c in chunks[:-1])
        assert all(len(c) <= chunk_bytes or c.count(b"\n") <= 1 for c in chunks)
    assert list(im.iter_line_chunks(io.BytesIO(b""), 5)) == []


def test_fail_in_a_later_chunk_keeps_the_earlier_chunks_and_names_the_line(tmp_path):
    good = cases.event_row(STATUS, "m", 3)
    text = (good + b"\n") * 50 + b"\n" + b'{"topic":256,"b64":""}\n' + good + b"\n"
    out = io.BytesIO()
    with pytest.raises(ValueError, match=r"^line 51: malformed row: unknown topic 256"):
        import_file(io.BytesIO(text), out, Policy("fail"), chunk_bytes=10 * (len(good) + 1))
    assert out.getvalue() == _frame(good) * 50


# ---- the command line ----------------------------------------------------------------------------

def _cli(command, *args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", command, *args], input=stdin, capture_output=True,
                          timeout=120)


def test_the_command_line_round_trip(tmp_path):
    from test_export import _forty
    from beholder_amd.ops import frames
    data = frames(_forty())
    capture, rows, back, lines = (tmp_path / n for n in ("in.bin", "rows.ndjson", "back.bin", "lines.txt"))
    capture.write_bytes(data)
    want = nm.normalise_cpu(data).data
    assert _cli("export", str(capture), "-o", str(rows)).returncode == 0
    r = _cli("import", str(rows), "-o", str(back), "--lines", str(lines), "--chunk-bytes", "300")
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == want and r.stdout == b""
    whole = import_cpu(rows.read_bytes())
    assert [int(k) for k in lines.read_text().split()] == whole.lines == list(range(40))
    counts = json.loads(r.stderr.decode().strip().splitlines()[-1])
    assert counts == {"lines": 40, "rows": 40, "frames": 40, "events": whole.events, "carried": whole.carried, "skipped": 0,
                      "blank": 0, "in_bytes": len(rows.read_bytes()), "out_bytes": len(want), "host_rows": 0}
    r = _cli("import", stdin=_cli("export", stdin=data).stdout)  # stdin to stdout, the defaults
    assert r.returncode == 0 and r.stdout == want
    assert r.stdout == _cli("normalise", stdin=data).stdout


def test_the_command_line_on_a_malformed_row(tmp_path):
    good = cases.event_row(STATUS, "m", 3)
    text = good + b"\n" + good + b"\nnot a row\n" + good + b"\n"
    out = tmp_path / "out.bin"
    r = _cli("import", "-o", str(out), "--chunk-bytes", str(len(good) + 5), stdin=text)
    assert r.returncode == 1 and b"line 2: malformed row" in r.stderr and r.stdout == b""
    assert out.read_bytes() == _frame(good) * 2  # whole frames of the chunks before it
    r = _cli("import", "--malformed", "skip", stdin=text)
    assert r.returncode == 0 and r.stdout == _frame(good) * 3
    assert json.loads(r.stderr.decode().strip().splitlines()[-1])["skipped"] == 1
    assert _cli("import", "--malformed", "first", stdin=text).returncode == 2
    assert _cli("import", "--device", "tpu", stdin=text).returncode == 2
    r = _cli("import", "-o", str(tmp_path / "none.bin"), stdin=b"not a row\n")
    assert r.returncode == 1 and not (tmp_path / "none.bin").exists()


def test_cli_gpu_without_a_device_names_the_cpu_path(tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    from beholder_amd.ops import hip_lib
    path = tmp_path / "rows.ndjson"
    path.write_bytes(cases.event_row(STATUS, "m", 3) + b"\n")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["import", str(path), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device gpu is not available" in out.err and "--device cpu" in out.err and not out.out
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "libbeholder_hip.so"))
    monkeypatch.setattr(hip_lib, "_lib", None)
    assert cli.main(["import", str(path), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device cpu" in out.err and "missing" in out.err and not out.out
