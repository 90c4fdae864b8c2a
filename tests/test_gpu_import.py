"""``import`` on the GPU (ops/hip/telemetry_import.hip, ops/gpu_import.py) against its definition,
``import_rows.import_cpu``: every comparison is full ``Imported`` equality (the frames' bytes, the line
numbers, the counts, the skipped lines, the base), exact."""
from __future__ import annotations

import functools
import io

import pytest

from beholder_amd import ops
from beholder_amd.import_rows import Imported, Policy, import_cpu, import_file, import_gpu
from beholder_amd.topics import PROGRESS, STATUS

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_extract, gpu_import as gi, hip_lib  # noqa: E402
import import_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
FAIL, SKIP = Policy("fail"), Policy("skip")
HOST_SHARE_MAX = 0.10  # of the fold corpus's export, in either dialect
PLAIN = cases.event_row(PROGRESS, "m", 2, 5, "h")


@functools.lru_cache(maxsize=None)
def _want(text: bytes, policy: Policy, base: int):
    try:
        return import_cpu(text, policy, base)
    except ValueError as e:
        return str(e)


def _same(text: bytes, policy: Policy = SKIP, base: int = 0, public: bool = False) -> tuple:
    """Asserts the device result against the definition; returns ``(Imported, host_rows)``. Where the
    definition raises, the device raises the same words, and this returns ``(the words, None)``."""
    want = _want(text, policy, base)
    if isinstance(want, str):
        with pytest.raises(ValueError) as e:
            gi.import_rows(text, policy, DEVICE, base)
        assert str(e.value) == want
        return want, None
    got, host_rows = gi.import_rows(text, policy, DEVICE, base)
    assert (got.line_count, got.events, got.carried, got.base, got.malformed) == \
        (want.line_count, want.events, want.carried, want.base, want.malformed)
    assert got.lines == want.lines and got.skipped == want.skipped
    if got.data != want.data:  # name the first byte that differs, not a megabyte of frames
        k = next((k for k, (g, w) in enumerate(zip(got.data, want.data)) if g != w), min(len(got.data), len(want.data)))
        assert got.data[max(0, k - 40):k + 40] == want.data[max(0, k - 40):k + 40], (k, len(got.data), len(want.data))
    assert got == want
    if public:
        assert import_gpu(text, policy, DEVICE, base) == want  # the public call
    return want, host_rows


def _both(text: bytes, base: int = 0) -> tuple:
    """Under both policies, for a text without a malformed row."""
    assert _same(text, FAIL, base)[1] == _same(text, SKIP, base)[1]
    return _same(text, SKIP, base)


# ---- nothing to do -------------------------------------------------------------------------------

def test_empty_input_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty input must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for policy in (FAIL, SKIP):
        want = Imported(base=3, malformed=policy.malformed)
        assert import_gpu(b"", policy, DEVICE, 3) == want == import_cpu(b"", policy, 3)
        assert gi.import_rows(b"", policy, DEVICE, 3) == (want, 0)
    out = io.BytesIO()
    assert import_file(io.BytesIO(b""), out, FAIL, DEVICE)["lines"] == 0 and out.getvalue() == b""


def test_no_frame_launches_no_emit(monkeypatch):
    call = hip_lib.call

    def no_emit(name, *args):
        assert name != "bh_import_emit", "nothing to emit"
        return call(name, *args)
    monkeypatch.setattr(hip_lib, "call", no_emit)
    for text in (b"\n", b"\n \t\r\n\n", b" " * 5000, b"\r\n" * 300):
        want, host_rows = _both(text)
        assert want.lines == [] and want.data == b"" and host_rows == 0 and want.line_count >= 1
    text = cases.text_of(cases.malformed_rows())
    want, host_rows = _same(text, SKIP, 9)
    assert want.lines == [] and want.skipped == list(range(9, 9 + host_rows)) and host_rows == len(cases.malformed_rows())
    with pytest.raises(AssertionError, match="nothing to emit"):
        _same(PLAIN + b"\n")


# ---- the split -----------------------------------------------------------------------------------

@pytest.mark.parametrize("at", [15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192])
def test_a_newline_at_the_lanes_and_the_tiles_edges(at):
    rest = [PLAIN, b"", cases.b64_row(7, b"abc")]
    want, host_rows = _both(cases.edge_line(at) + b"\n" + cases.text_of(rest), base=5)
    assert want.lines == ([5, 6, 8] if at >= 20 else [6, 8]) and want.line_count == 4 and host_rows == 0


def test_the_lines_of_the_split():
    """The starts themselves, against Python's split."""
    text = cases.edge_line(4095) + b"\n" + b"\n" * 4100 + PLAIN + b"\r\n\n" + cases.edge_line(8190) + b"\n" + PLAIN + b"\n"
    lines = gi.split(gi.upload(text, DEVICE))
    starts = [0]
    for line in text.split(b"\n")[:-1]:
        starts.append(starts[-1] + len(line) + 1)
    assert lines.n == len(starts) - 1 and lines.starts.cpu().numpy().tolist() == starts
    assert gi.split(gi.upload(text + PLAIN, DEVICE)).starts.cpu().numpy().tolist() == starts + [starts[-1] + len(PLAIN) + 1]


def test_long_rows_many_newlines_crlf_and_no_final_newline():
    long_row = cases.b64_row(9, bytes(range(256)) * 36)  # longer than two tiles, no newline inside
    assert len(long_row) > 3 * 4096
    a = cases.event_row(STATUS, "m", 3)
    for text in (cases.text_of([long_row, a, long_row]), long_row, b"\n" * 4096, b"\n" * 4096 + a, b"\n" * 4097 + a + b"\n",
                 a + b"\n" + PLAIN, cases.text_of([a, PLAIN, b"", a], b"\r\n"), cases.text_of([a, PLAIN], b"\r\n", final=False),
                 b"\n \t\r\n" + a + b"\n\n\n  " + PLAIN + b" \t\n\r\n"):
        want, host_rows = _both(text, base=1)
        assert host_rows == 0 and len(want.lines) == text.count(a) + text.count(PLAIN) + text.count(long_row)


# ---- row counts and frame lengths ----------------------------------------------------------------

def test_single_row():
    for row in (PLAIN, cases.event_row(STATUS), cases.b64_row(9, b""), cases.b64_row(PROGRESS, b"\x2e"),
                cases.event_row(PROGRESS, None, -1, -2 ** 31)):
        want, host_rows = _both(row + b"\n")
        assert want.lines == [0] and host_rows == 0
        assert _both(row)[0].data == want.data
    want, _ = _same(PLAIN + b"\n", FAIL, 7, public=True)
    assert want == Imported(b"\x0b\x00\x00\x00\x02\x0a\x01m\x10\x02\x18\x05\x22\x01h", [7], 1, 1, 0, [], 7, "fail")


@pytest.mark.parametrize("count", [64, 65, gpu_extract.SCAN_BLOCK, gpu_extract.SCAN_BLOCK + 1])
def test_one_row_past_a_wave_and_past_a_block_of_the_scan(count):
    kinds = [cases.event_row(STATUS, "media-%d", 2), cases.event_row(PROGRESS, 'm\\"', 2, 50, "ho\\u0001st"),
             cases.b64_row(9, b"other"), b"", cases.event_row(STATUS), cases.event_row(PROGRESS, None, None, -7),
             b'{"topic":"v1.telemetry.status","json":{"status":"errored"}}', b"junk"]
    rows = [kinds[k % len(kinds)].replace(b"%d", b"%d" % k) for k in range(count)]
    want, host_rows = _same(cases.text_of(rows))
    assert want.line_count == count and host_rows == len(want.skipped) * 2 and 0 < want.carried < want.events < count
    assert isinstance(_same(cases.text_of(rows), FAIL)[0], str)
    for last in (kinds[1], kinds[2], kinds[6]):  # the last row alone in its wave or block
        want, _ = _both(cases.text_of([b""] * (count - 1) + [last]), base=3)
        assert want.lines == [3 + count - 1] and want.line_count == count


@pytest.mark.parametrize("length", [63, 64, 65, 128, 129])
def test_a_frame_of_exactly_this_length(length):
    """Where a lane's stride of 64 ends: the last lane, the first lane's second byte, and its third."""
    rows = cases.frame_length_rows(length)
    want, host_rows = _both(cases.text_of(rows * 3))
    assert host_rows == 0 and len(want.data) == 3 * len(rows) * length and want.carried == 6


# ---- escapes, base64 and numbers -----------------------------------------------------------------

def test_escapes_and_backslash_runs_across_the_pieces_of_64():
    rows = cases.escape_rows()
    want, host_rows = _both(cases.text_of(rows))
    assert host_rows == 0 and want.events == len(rows) > 500
    assert b"\x0a\xc8\x01" + b"\x01" * 200 in want.data and b"\x0a\xc8\x01" + b"\\" * 200 in want.data


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_ascii_byte_as_an_id_and_as_a_host(dialect):
    want, host_rows = _both(cases.ascii_byte_rows(dialect))
    assert host_rows == 0 and want.events == 3 * 128


def test_base64_bodies():
    rows = cases.base64_rows()
    want, host_rows = _both(cases.text_of(rows * 3))
    assert host_rows == 0 and want.carried == 3 * len(rows) and want.events == 0


def test_int32_extremes():
    rows = [cases.event_row(PROGRESS, "m", s, p, "h") for s in cases.INT32_EDGES for p in cases.INT32_EDGES]
    rows += [cases.event_row(STATUS, None, s) for s in cases.INT32_EDGES]
    want, host_rows = _both(cases.text_of(rows))
    assert host_rows == 0 and want.events == len(rows)
    assert b"\x10\x80\x80\x80\x80\xf8\xff\xff\xff\xff\x01\x18\xff\xff\xff\xff\x07" in want.data


# ---- the grammar ---------------------------------------------------------------------------------

def test_the_relaxed_grammar_stays_on_the_device():
    rows = cases.relaxed_rows()
    want, host_rows = _both(cases.text_of(rows))
    assert host_rows == 0 and want.lines == list(range(len(rows))) and want.events and want.carried


def test_hand_written_rows():
    rows = cases.valid_rows()
    want, host_rows = _both(cases.text_of(rows), base=2 ** 40)
    assert want.lines == list(range(2 ** 40, 2 ** 40 + len(rows))) and 0 < host_rows < len(rows) // 2


# ---- host rows -----------------------------------------------------------------------------------

def test_host_rows_first_last_and_neighbours():
    hosts = [b'{"topic":"v1.telemetry.status","json":{"mediaId":"m1","status":"dePLoyed"}}',
             '{"i":1,"topic":"v1.telemetry.progress","json":{"mediaId":"é","status":1,"progress":2,"host":"h"},"name":null}'.encode(),
             cases.event_row(PROGRESS, "\\u00fc" * 40, -1, 3, 'h\\"\\u0001'), b'{"topic":9,"b64":"QUJD","extra":[1,2]}']
    bad = [b"not a row", b'{"topic":256,"b64":""}', b'{"topic":9,"b64":"QQ="}']
    for layout, count in (([hosts[0], PLAIN, PLAIN], 1), ([PLAIN, PLAIN, hosts[1]], 1), ([PLAIN, hosts[0], hosts[1], PLAIN], 2),
                          ([hosts[2], hosts[1], hosts[0], hosts[3]], 4),
                          ([hosts[1]] + [PLAIN] * 70 + [hosts[2], hosts[0]] + [PLAIN] * 70 + [hosts[3]], 4)):
        want, host_rows = _both(cases.text_of(layout), base=98)
        assert host_rows == count and want.lines == list(range(98, 98 + len(layout)))
    for layout, first in (([bad[0], PLAIN, hosts[0]], 0), ([PLAIN, hosts[0], bad[1]], 2), ([hosts[1], bad[2], bad[0], PLAIN], 1),
                          ([PLAIN] * 70 + [bad[1]] + [PLAIN] * 70 + [hosts[2], bad[0]] + [PLAIN] * 200 + [bad[2]], 70),
                          ([PLAIN] * 300 + [bad[2], hosts[3], bad[1]], 300)):
        text = cases.text_of(layout)
        want, host_rows = _same(text, SKIP, 40)
        assert want.skipped == [40 + k for k, row in enumerate(layout) if row in bad] and host_rows == len(layout) - layout.count(PLAIN)
        words, _ = _same(text, FAIL, 40)
        assert words.startswith(f"line {40 + first}: malformed row: ")  # the smallest line number


# ---- the corpora ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", cases.CORPORA)
def test_the_exports_of_the_corpora(name, dialect):
    from beholder_amd import normalise as nm
    text = cases.exported(name, dialect).data
    want, host_rows = _both(text)
    _same(text, FAIL, 0, public=True)
    assert want.data == nm.normalise_cpu(cases.corpus(name), nm.Policy(), dialect).data and want.line_count > 5000
    assert host_rows == sum(max(line) >= 0x80 for line in text.split(b"\n")[:-1])
    if name == "fold_corpus":
        assert host_rows <= HOST_SHARE_MAX * want.line_count
        assert host_rows == (189 if dialect == "protobufjs" else 0)
    _both(cases.exported(name, dialect, "drop").data)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_import_file_on_the_device_in_chunks(dialect):
    """Twenty chunks or so, each through the device from the number its first line has."""
    text = cases.exported("fold_corpus", dialect).data
    assert len(text) > 20 * 30_000
    want = _want(text, FAIL, 0)
    for chunk_bytes in (30_000, 1 << 30):
        out, lines = io.BytesIO(), io.StringIO()
        counts = import_file(io.BytesIO(text), out, FAIL, DEVICE, chunk_bytes=chunk_bytes, lines_out=lines)
        assert out.getvalue() == want.data
        assert [int(k) for k in lines.getvalue().split()] == want.lines
        assert counts == {"lines": want.line_count, "rows": want.line_count, "frames": len(want.lines), "events": want.events,
                          "carried": want.carried, "skipped": 0, "blank": 0, "in_bytes": len(text), "out_bytes": len(want.data),
                          "host_rows": gi.import_rows(text, FAIL, DEVICE)[1]}
    bad = text[:100_000] + b"not a row\n" + text[100_000:]
    out = io.BytesIO()
    with pytest.raises(ValueError, match=f"^line {text[:100_000].count(10)}: malformed row"):
        import_file(io.BytesIO(bad), out, FAIL, DEVICE, chunk_bytes=30_000)
    assert 0 < len(out.getvalue()) < len(want.data) and want.data.startswith(out.getvalue())


# ---- determinism, checks and limits --------------------------------------------------------------

def test_import_is_deterministic():
    text = cases.exported("fold_corpus", "protobufjs").data
    first = import_gpu(text, SKIP, DEVICE)
    assert first == import_gpu(text, SKIP, DEVICE) == _want(text, SKIP, 0)


def test_the_size_check_comes_before_any_upload(monkeypatch):
    import torch
    assert gi.text_size(b"") == 0 and gi.text_size(b"a") == 2 and gi.text_size(b"a\n") == 2

    def no_upload(*args, **kwargs):
        raise AssertionError("the size check comes first")
    monkeypatch.setattr(gi, "upload", no_upload)
    monkeypatch.setattr(torch, "frombuffer", no_upload)
    for size in (2 ** 31, 2 ** 33):
        monkeypatch.setattr(gi, "text_size", lambda data, size=size: size)
        with pytest.raises(ValueError, match="2\\^31") as e:
            gi.import_rows(PLAIN + b"\n", FAIL, DEVICE)
        assert isinstance(e.value, gi.TooLarge)
        with pytest.raises(ValueError, match="--chunk-bytes"):
            import_file(io.BytesIO(PLAIN + b"\n"), io.BytesIO(), FAIL, DEVICE)
    monkeypatch.setattr(gi, "text_size", lambda data: 2 ** 31 - 1)  # fits: the upload is next
    with pytest.raises(AssertionError, match="the size check comes first"):
        gi.import_rows(PLAIN + b"\n", FAIL, DEVICE)


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    text = PLAIN + b"\n" + PLAIN + b"\n"
    buf = gi.upload(text, DEVICE)
    lines = gi.split(buf)
    tables = gi.allocate(buf, lines.starts, lines.n)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gi.allocate(buf, lines.starts.to(torch.int64), lines.n)  # wrong dtype
    with pytest.raises(ValueError):
        gi.allocate(buf.cpu(), lines.starts.cpu(), lines.n)  # host tensors
    with pytest.raises(ValueError):
        gi.allocate(buf, lines.starts, lines.n + 1)  # starts is not n + 1
    with pytest.raises(ValueError):
        gi.allocate(buf, lines.starts[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        gi.split(buf.cpu())
    with pytest.raises(ValueError):
        gi.split(buf[:0])
    with pytest.raises(ValueError):
        gi.split(buf[1:])  # not at a multiple of 16 bytes
    with pytest.raises(ValueError):
        gi.split(buf.to(torch.int32))
    for base in (-1, 2 ** 63, 1.5, True):
        with pytest.raises(ValueError):
            import_gpu(text, FAIL, DEVICE, base=base)
    bad = Policy()
    object.__setattr__(bad, "malformed", "first")  # a policy that got past its own check
    for call in (lambda: gi.import_rows(text, bad, DEVICE), lambda: gi.decide_on_host(tables, text, bad)):
        with pytest.raises(ValueError):
            call()
    for kept, kept_bytes in ((-1, 5), (lines.n + 1, 20), (1, 0), (0, 5), (1, len(text) + 1)):
        with pytest.raises(ValueError):
            gi.emit(tables, kept, kept_bytes)
    with pytest.raises(TypeError):
        gi.import_rows(text, "fail", DEVICE)
    with pytest.raises(TypeError):
        import_gpu(text, "skip", DEVICE)
    with pytest.raises(ValueError):
        import_gpu(text, FAIL, "cpu")
