"""The gfx950 kernels' readers (ops/hip/telemetry_readers.hpp) on a CPU, under ASan and UBSan.

tests/native/readers_host.cpp compiles the header for the host and reads every topic-1/2 frame of a
stream from a heap block of exactly the body's size: a reader that steps past its message is a
sanitizer report here. Its rows are compared with the service's own codecs
(``ops.codec_for(type, dialect).decode``) for both message types, in the protobufjs dialect and in
upb's STRICT form, and with ``gpu_decode.reference_table`` for the two forms the decode kernel uses.
Together that runs all six instantiations (protobufjs, upb, upb STRICT; status and progress)."""
from __future__ import annotations

import os
import random
import shutil
import subprocess

import pytest

from beholder_amd import ops
from beholder_amd.models import proto
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_decode as gd  # noqa: E402
import wire_edges  # noqa: E402
from telemetry_corpus import decode_corpus, fold_corpus  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
OK_ERROR, OK_DECODED, OK_HOST = 0, 1, 2  # Row::ok of telemetry_readers.hpp
MODES = {"protobufjs": "protobufjs", "upb": "upb-strict"}  # dialect -> the program's mode that follows its codec
TYPES = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}


@pytest.fixture(scope="module")
def program() -> str:
    b = subprocess.run(["make", "-s", "readers_host_asan"], cwd=HERE, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr  # the rule has -Wall -Wextra -Werror
    return os.path.join(HERE, "readers_host_asan")


def _rows(program: str, mode: str, stream: bytes, tmp_path):
    """The program's (k, 8) table for the topic-1/2 frames of ``stream``; any sanitizer report fails."""
    path = tmp_path / "stream.bin"
    path.write_bytes(stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, mode, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return np.array([line.split() for line in r.stdout.splitlines()], dtype=np.int64).reshape(-1, 8)


def _frames_12(stream: bytes) -> list:
    """(topic, body start, body end) of every topic-1/2 frame of a framed stream."""
    out, i = [], 0
    while i < len(stream):
        length = int.from_bytes(stream[i:i + 4], "little")
        if stream[i + 4] in TYPES:
            out.append((stream[i + 4], i + 5, i + 4 + length))
        i += 4 + length
    return out


def _high(b: bytes) -> bool:
    return any(c >= 0x80 for c in b)


def _against_codec(stream: bytes, rows, dialect: str, left: set = None):
    """Asserts the rows against the service's codec; returns (frames left out, compared frames the
    codec raises on). The indices of the frames left out are added to ``left`` where given."""
    index = _frames_12(stream)
    assert len(rows) == len(index)
    codecs = {t: ops.codec_for(p, dialect) for t, p in TYPES.items()}
    left_out = raised = 0
    bad = []
    for k, ((topic, start, end), row) in enumerate(zip(index, rows.tolist())):
        id_off, id_len, status, progress, host_off, host_len, ok, _ = row
        try:
            m = codecs[topic].decode(stream[start:end])
            want = (m.mediaId, m.status, getattr(m, "progress", 0), getattr(m, "host", ""))
        except proto.DecodeError:
            want = None
        mid, host = stream[id_off:id_off + id_len], stream[host_off:host_off + host_len]
        for off, n in ((id_off, id_len), (host_off, host_len)):
            assert n == 0 or start <= off and off + n <= end, (stream[start:end], row)
        # what the device hands to the host: the fold decodes these frames with the codec itself
        upb_host = dialect == "upb" and topic == PROGRESS_ID
        if ok == OK_HOST or ok == OK_DECODED and (_high(mid) or upb_host and _high(host)):
            left_out += 1
            if left is not None:
                left.add(k)
            continue
        raised += want is None
        # protobufjs decodes invalid UTF-8 to U+FFFD; upb strings that reach this line are ASCII
        got = None if ok == OK_ERROR else (mid.decode("utf-8", "replace"), status, progress,
                                           host.decode("utf-8", "replace"))
        if got != want:
            bad.append((topic, stream[start:end], row, want))
    assert not bad, (len(bad), bad[:5])
    return left_out, raised


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_readers_agree_with_the_service_codec_on_the_fold_corpus(program, tmp_path, dialect):
    stream = fold_corpus()
    rows = _rows(program, MODES[dialect], stream, tmp_path)
    left_out, raised = _against_codec(stream, rows, dialect)
    print(f"{dialect}: {len(rows)} topic-1/2 frames, {left_out} left to the host, the codec raises on {raised}")
    assert len(rows) > 5000
    assert left_out <= 0.05 * len(rows)  # the comparison covers what the device decides itself
    assert raised >= 1000                # and the corpus does reach the error branches


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_decode_kernel_readers_on_the_decode_corpus(program, tmp_path, dialect):
    """The two instantiations the decode kernel uses, MSG_PROGRESS in plain upb and in protobufjs:
    rows equal ``gpu_decode.reference_table`` exactly. The codec's form of the dialect is checked
    against the codec on the same bodies."""
    bodies = decode_corpus(random.Random(11))
    stream = frames([(PROGRESS_ID, b) for b in bodies])
    got = _rows(program, dialect, stream, tmp_path)
    # stream positions -> positions in the packed batch: body k starts 5 * (k + 1) bytes later in the stream
    shift = 5 * (np.arange(len(bodies)) + 1)
    got[:, 0] -= np.where(got[:, 7] & 1, shift, 0)
    got[:, 4] -= np.where(got[:, 7] & 8, shift, 0)
    want = gd.reference_table(bodies, dialect)
    diff = np.nonzero(np.any(got != want, axis=1))[0]
    assert len(diff) == 0, [(bodies[i], got[i].tolist(), want[i].tolist()) for i in diff[:5]]
    _against_codec(stream, _rows(program, MODES[dialect], stream, tmp_path), dialect)


def test_plain_upb_reads_both_message_types_in_bounds(program, tmp_path):
    """The one form no codec follows, plain upb as a TelemetryStatus, and the same as a progress: fields
    inside the message (and no sanitizer report), progress rows equal to the Python definition."""
    stream = fold_corpus()
    rows = _rows(program, "upb", stream, tmp_path)
    index = _frames_12(stream)
    assert len(rows) == len(index)
    for (topic, start, end), row in zip(index, rows.tolist()):
        if topic == PROGRESS_ID:
            assert row == gd.reference_decode(stream, start, end), stream[start:end]
        else:
            assert row[3] == 0 and row[5] == 0 and not row[7] & 12, (stream[start:end], row)
            assert row[1] == 0 or start <= row[0] and row[0] + row[1] <= end, (stream[start:end], row)


# ---- the systematic corpus (wire_edges.py) ------------------------------------------------------

@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_readers_agree_with_the_service_codec_on_the_wire_edges(program, tmp_path, dialect):
    """Both message types in the codec's form of each dialect over every body of the corpus. upb's
    STRICT reader hands the group families over by design; under protobufjs the frames left out are
    exactly those that decode to an id that is not ASCII."""
    stream = wire_edges.stream()
    rows = _rows(program, MODES[dialect], stream, tmp_path)
    left = set()
    left_out, raised = _against_codec(stream, rows, dialect, left)
    print(f"{dialect}: {len(rows)} topic-1/2 frames, {left_out} left to the host, the codec raises on {raised}")
    assert len(rows) == 2 * len(wire_edges.bodies())
    assert left_out <= wire_edges.HOST_CAP[dialect] * len(rows)
    if dialect == "protobufjs":
        want = wire_edges.expected(dialect)
        assert left == {k for k, v in enumerate(want) if v is not None and not v.media_id.isascii()}


def test_plain_upb_follows_its_definition_on_the_wire_edges(program, tmp_path):
    """The decode kernel's plain upb reader against ``gpu_decode.reference_decode``, exactly, on every
    body: as a progress the row itself, as a status the same walk with fields 3 and 4 unknown. A tag
    whose field number is 2^32 + k is an unknown field, not field k."""
    stream = wire_edges.stream()
    rows = _rows(program, "upb", stream, tmp_path)
    index = _frames_12(stream)
    assert len(rows) == len(index)
    bad = []
    for (topic, start, end), row in zip(index, rows.tolist()):
        want = gd.reference_decode(stream, start, end)
        if topic == STATUS_ID:
            want = want[:3] + [0, 0, 0, want[6], want[7] & 3]
        if row != want:
            bad.append((topic, stream[start:end], row, want))
    assert not bad, (len(bad), bad[:5])
    wide = [k for k, (_, start, end) in enumerate(index) if stream[start:end] == bytes.fromhex("8a808080800101 6d")]
    assert len(wide) == 2 and all(rows[k].tolist() == [0, 0, 0, 0, 0, 0, OK_DECODED, 0] for k in wide)
