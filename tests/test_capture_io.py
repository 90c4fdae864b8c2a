"""What the capture commands share: the source opener of ``beholder_amd.capture_io``, and the
output closer and the ``--device gpu`` check of ``beholder_amd.cli``."""
import io
import sys

import pytest

from beholder_amd import capture_io, cli
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

CAPTURE = frames([(STATUS_ID, b"\x0a\x01m\x10\x02"), (PROGRESS_ID, b"\x0a\x01m\x10\x02\x18\x05\x22\x01h"),
                  (PROGRESS_ID, b"\x0a\x01m\x10\x02\x18\x07\x22\x01h")])
ROWS = (b'{"topic":"v1.telemetry.status","json":{"mediaId":"m","status":2}}\n'
        b'{"topic":"v1.telemetry.progress","json":{"mediaId":"m","status":2,"progress":5,"host":"h"}}\n'
        b'{"topic":9,"b64":"QUJD"}\n')


class Boom(Exception):
    pass


@pytest.mark.parametrize("as_type", [str, lambda p: str(p).encode(), lambda p: p], ids=["str", "bytes", "pathlike"])
@pytest.mark.parametrize("raises", [False, True])
def test_open_source_opens_and_closes_a_path(tmp_path, as_type, raises):
    path = tmp_path / "capture.bin"
    path.write_bytes(CAPTURE)
    seen = None
    try:
        with capture_io.open_source(as_type(path)) as f:
            seen = f
            assert f.read() == CAPTURE and not f.closed
            if raises:
                raise Boom
    except Boom:
        assert raises
    assert seen.closed


@pytest.mark.parametrize("raises", [False, True])
def test_open_source_leaves_a_file_object_open(raises):
    source = io.BytesIO(CAPTURE)
    try:
        with capture_io.open_source(source) as f:
            assert f is source
            if raises:
                raise Boom
    except Boom:
        assert raises
    assert not source.closed and source.read() == CAPTURE


def test_device_name_and_index_lines():
    assert [capture_io.torch_device(d) for d in ("gpu", "cpu", "cuda:1")] == ["cuda", "cpu", "cuda:1"]
    out = io.StringIO()
    capture_io.write_indices(out, [0, 2, 5])
    capture_io.write_indices(out, [1], base=10)
    capture_io.write_indices(out, [])
    assert out.getvalue() == "0\n2\n5\n11\n"
    assert list(capture_io.frame_spans(CAPTURE)) == [(0, 10), (10, 25), (25, 40)]
    with pytest.raises(ValueError, match="truncated"):
        list(capture_io.frame_spans(CAPTURE[:-1]))


def test_close_outputs_after_success_finishes_every_output(tmp_path):
    written, untouched = cli._LazyOutput(str(tmp_path / "a.bin")), cli._LazyOutput(str(tmp_path / "b.txt"), text=True)
    written.write(b"abc")
    cli._close_outputs([written, None, untouched])
    assert (tmp_path / "a.bin").read_bytes() == b"abc" and written.file.closed
    assert (tmp_path / "b.txt").read_text() == "" and untouched.file.closed


def test_close_outputs_after_failure_closes_only_what_was_opened(tmp_path):
    written, untouched = cli._LazyOutput(str(tmp_path / "a.bin")), cli._LazyOutput(str(tmp_path / "b.txt"), text=True)
    written.write(b"abc")
    cli._close_outputs([written, None, untouched], ValueError("truncated frame header"))
    assert (tmp_path / "a.bin").read_bytes() == b"abc" and written.file.closed
    assert not (tmp_path / "b.txt").exists() and untouched.file is None


@pytest.mark.parametrize("failed", [None, ValueError("truncated frame header")])
def test_close_outputs_flushes_stdout_and_leaves_it_open(monkeypatch, failed):
    class Stdout:
        def __init__(self):
            self.buffer = self
            self.data, self.flushes, self.closed = b"", 0, False

        def write(self, data):
            self.data += data
            return len(data)

        def flush(self):
            self.flushes += 1

        def close(self):
            self.closed = True
    fake = Stdout()
    monkeypatch.setattr(sys, "stdout", fake)
    out = cli._LazyOutput("-")
    out.write(b"abc")
    cli._close_outputs([out], failed)
    assert fake.data == b"abc" and fake.flushes == 1 and not fake.closed


GPU_COMMANDS = {
    "summarise": [], "transitions": [], "hosts": [], "stages": [],
    "extract": ["-o", "{out}"], "coalesce": ["-o", "{out}"], "dedupe": ["-o", "{out}"], "thin": ["-o", "{out}"],
    "normalise": ["-o", "{out}"], "anonymise": ["-o", "{out}"], "export": ["-o", "{out}"], "import": ["-o", "{out}"],
    "shard": ["--shards", "2", "-o", "{out}-{{}}"], "compare": ["{input}"],
}


@pytest.mark.parametrize("command", sorted(GPU_COMMANDS))
def test_device_gpu_without_a_device_names_the_cpu_path(command, tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    path, out = tmp_path / "input", tmp_path / "out"
    path.write_bytes(ROWS if command == "import" else CAPTURE)
    monkeypatch.setenv(cli.ANONYMISE_KEY_ENV, "00" * 16)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    extra = [x.format(out=out, input=path) for x in GPU_COMMANDS[command]]
    assert cli.main([command, str(path)] + extra + ["--device", "gpu"]) == 1
    said = capsys.readouterr()
    assert "--device gpu is not available" in said.err and "--device cpu" in said.err and not said.out
    assert command == "extract" or not list(tmp_path.glob("out*"))  # only extract opens its output at once
