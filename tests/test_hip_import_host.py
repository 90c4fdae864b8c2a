"""The gfx950 import kernels' per-line code (ops/hip/telemetry_import.hpp: the split's newline masks,
the row reader and its plan, the frame's length, every byte of the frame, the unescape in pieces of
64) on a CPU, under ASan and UBSan.

tests/native/import_host.cpp compiles the header for the host, finds the lines as the split kernels
do, plans every line from a heap block of exactly the line's size and builds every frame twice into
heap blocks of exactly the frame's length: one byte after the other, and piecewise as the emit kernel
does. The program itself fails where the two differ or miss ``out_len``; here its line starts are held
to Python's split and its frames to ``import_rows.frame_of_row``. A line it leaves to the host is
passed over in the comparison, and the tests say which lines may be: none in export's exact shape
that is ASCII, every line with a byte >= 0x80, every malformed one. Nothing is loaded into Python
under a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from beholder_amd import import_rows as im, ops
from beholder_amd.topics import PROGRESS, STATUS

import import_cases as cases  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
HOST_SHARE_MAX = 0.10  # of the fold corpus's export, in either dialect


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/test_hip_export_host.py."""
    out = str(tmp_path_factory.mktemp("import_host") / "import_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "import_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _run(program: str, text: bytes, tmp_path) -> list:
    """The program's output lines for ``text``; any sanitizer report fails."""
    path = tmp_path / "rows"
    path.write_bytes(text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.splitlines()


def _against_the_definition(program: str, text: bytes, tmp_path) -> dict:
    """Asserts the starts and every line; returns the line positions per kind of line."""
    got = _run(program, text, tmp_path)
    lines = im.split_lines(text)
    starts = [0]
    for line in lines:
        starts.append(starts[-1] + len(line) + 1)
    assert [int(w) for w in got[0].split()[1:]] == starts and got[0].startswith("starts")
    assert len(got) == 1 + len(lines)
    frame = im.decided_frame_of_row()
    kinds = {"blank": set(), "host": set(), "b64": set(), "status": set(), "progress": set()}
    bad = []
    for k, (line, said) in enumerate(zip(lines, got[1:])):
        word = said.split()
        kinds[word[0]].add(k)
        stripped = line.strip(im.BLANK)
        if not stripped:
            want = ["blank"]
        else:
            try:
                f, from_b64 = frame(stripped)
            except im.MalformedRow:
                want = ["host"]  # the device never decides that a row is malformed
            else:
                if word[0] == "host":
                    continue
                want = ["b64" if from_b64 else "status" if f[4] == 1 else "progress", f.hex()]
        if word != want:
            bad.append((k, line, said, want))
    assert not bad, (len(bad), bad[:5])
    assert all(k in kinds["host"] for k, line in enumerate(lines) if max(line, default=0) >= 0x80)
    return kinds


@pytest.mark.parametrize("undecoded", ("keep", "drop"))
@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", cases.CORPORA)
def test_every_row_of_the_exports(program, tmp_path, name, dialect, undecoded):
    text = cases.exported(name, dialect, undecoded).data
    kinds = _against_the_definition(program, text, tmp_path)
    lines = text.split(b"\n")[:-1]
    rows = len(lines)
    assert rows > 300 and kinds["status"] and kinds["progress"] and not kinds["blank"]
    assert bool(kinds["b64"]) == (undecoded == "keep")
    assert kinds["host"] == {k for k, line in enumerate(lines) if max(line) >= 0x80}  # no ASCII row of export's is the host's
    print(f"{name} {dialect} {undecoded}: {len(kinds['host'])} of {rows} rows left to the host")
    if name == "fold_corpus":
        assert len(kinds["host"]) <= HOST_SHARE_MAX * rows
        if dialect == "protobufjs" and undecoded == "keep":
            assert rows == 5711 and len(kinds["host"]) == 189
        if dialect == "upb":
            assert not kinds["host"]


def test_hand_written_rows(program, tmp_path):
    rows = cases.valid_rows()
    kinds = _against_the_definition(program, cases.text_of(rows), tmp_path)
    device = kinds["b64"] | kinds["status"] | kinds["progress"]
    assert len(device) > len(rows) // 2 and not kinds["blank"]
    by_name = [k for k, row in enumerate(rows) if b'"status":"' in row]
    assert by_name and set(by_name) <= kinds["host"]  # a status by name is the host's
    assert cases.text_of(rows).count(b"\n") == len(rows)


def test_the_relaxed_grammar_stays_on_the_device(program, tmp_path):
    rows = cases.relaxed_rows()
    kinds = _against_the_definition(program, cases.text_of(rows), tmp_path)
    assert not kinds["host"] and not kinds["blank"] and kinds["b64"] and kinds["status"] and kinds["progress"]


def test_malformed_rows_go_to_the_host(program, tmp_path):
    rows = cases.malformed_rows()
    kinds = _against_the_definition(program, cases.text_of(rows), tmp_path)
    assert kinds["host"] == set(range(len(rows)))


def test_lines_crlf_blank_lines_and_no_final_newline(program, tmp_path):
    a, b = cases.event_row(STATUS, "m", 3), cases.b64_row(9, b"xyz")
    for text in (a + b"\n" + b, a + b"\r\n" + b + b"\r\n", b"\n \t\r\n" + a + b"\n\n\n  " + b + b" \t\n\r\n", b"\n", b"",
                 b"\n" * 4096, b"\n" * 4097 + a, b" " * 5000 + a + b"\n" + b"\t" * 4090 + b"\n" + b):
        kinds = _against_the_definition(program, text, tmp_path)
        assert not kinds["host"]
        assert len(kinds["status"]) == text.count(a) and len(kinds["b64"]) == text.count(b)


@pytest.mark.parametrize("at", [15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192])
def test_a_newline_at_the_lanes_and_the_tiles_edges(program, tmp_path, at):
    """The first line's newline is at byte ``at``: the last byte of a lane or of a tile, the first of the
    next, and one on. The shortest row has 20 bytes, so below that the line is a blank one."""
    first = cases.edge_line(at)
    rest = [cases.event_row(PROGRESS, "m", 1, 2, "h"), b"", cases.b64_row(7, b"abc")]
    kinds = _against_the_definition(program, first + b"\n" + cases.text_of(rest), tmp_path)
    assert kinds["b64"] == ({0, 3} if at >= 20 else {3}) and kinds["progress"] == {1}
    assert kinds["blank"] == ({2} if at >= 20 else {0, 2})


def test_a_row_longer_than_two_tiles(program, tmp_path):
    long_row = cases.b64_row(9, bytes(range(256)) * 36)
    assert len(long_row) > 3 * 4096
    kinds = _against_the_definition(program, cases.text_of([long_row, cases.event_row(STATUS, "m"), long_row]), tmp_path)
    assert kinds["b64"] == {0, 2} and kinds["status"] == {1}


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_ascii_byte_as_an_id_and_as_a_host(program, tmp_path, dialect):
    """Through export and back: the escapes json.dumps writes, one by one."""
    text = cases.ascii_byte_rows(dialect)
    kinds = _against_the_definition(program, text, tmp_path)
    assert not kinds["host"] and not kinds["b64"] and len(kinds["progress"]) == 256 and len(kinds["status"]) == 128


def test_escapes_and_backslash_runs_across_the_pieces_of_64(program, tmp_path):
    rows = cases.escape_rows()
    assert len(rows) > 500
    kinds = _against_the_definition(program, cases.text_of(rows), tmp_path)
    assert not kinds["host"] and not kinds["b64"] and not kinds["blank"]


def test_base64_bodies(program, tmp_path):
    rows = cases.base64_rows()
    kinds = _against_the_definition(program, cases.text_of(rows), tmp_path)
    assert kinds["b64"] == set(range(len(rows)))


@pytest.mark.parametrize("length", [63, 64, 65, 128, 129])
def test_a_frame_of_exactly_this_length(program, tmp_path, length):
    rows = cases.frame_length_rows(length)
    frame = im.frame_of_row()
    assert all(len(frame(row)) == length for row in rows)
    kinds = _against_the_definition(program, cases.text_of(rows), tmp_path)
    assert not kinds["host"] and len(kinds["b64"]) == 2
