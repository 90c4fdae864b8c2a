"""``normalise`` on the CPU (beholder_amd/normalise.py): the laws its docstring states, on the fold
corpus and the wire-edge stream in both dialects; merge, the file path, the command line; and single
frames against expected bytes written out here."""
from __future__ import annotations

import functools
import io
import json
import subprocess
import sys

import pytest

from beholder_amd import dedupe, hosts, normalise as nm, ops, replay, stages, transitions
from beholder_amd.coalesce import DROP, KEEP, _spans
from beholder_amd.normalise import Normalised, Policy, canon_of, normalise_cpu, normalise_file
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus  # noqa: E402

CORPORA = {"fold_corpus": fold_corpus, "wire_edges": lambda: wire_edges.stream(6000)}
OTHER = {"protobufjs": "upb", "upb": "protobufjs"}
# frames that dedupe keeps: of the stream, and of its normalised form per dialect
DEDUPE_KEPT = {"fold_corpus": (5008, {"protobufjs": 4435, "upb": 4452}),
               "wire_edges": (5920, {"protobufjs": 4812, "upb": 5515})}


@functools.lru_cache(maxsize=None)
def _stream(name: str) -> bytes:
    return CORPORA[name]()


@functools.lru_cache(maxsize=None)
def _normalised(name: str, undecoded: str, dialect: str) -> Normalised:
    return normalise_cpu(_stream(name), Policy(undecoded), dialect)


def _reports(data: bytes, dialect: str) -> dict:
    """What the four report commands print, as their JSON."""
    return {"summarise": replay.fold_cpu(data, dialect).to_json(),
            "transitions": transitions.transitions_cpu(data, dialect).to_json(per_media=True),
            "hosts": hosts.hosts_cpu(data, dialect).to_json(per_media=True),
            "stages": stages.stages_cpu(data, dialect).to_json(per_media=True)}


both = pytest.mark.parametrize("dialect", ops.DIALECTS)
corpora = pytest.mark.parametrize("name", sorted(CORPORA))


@corpora
@both
def test_idempotent(name, dialect):
    for undecoded in ("keep", "drop"):
        once = _normalised(name, undecoded, dialect)
        assert once.events > 400 and 0 < once.rewritten <= once.events and once.frames > 5000
        again = normalise_cpu(once.data, Policy(undecoded), dialect)
        assert again.data == once.data and again.rewritten == 0
        assert again.indices == list(range(len(once.indices))) and again.events == once.events


@corpora
@both
def test_the_reports_do_not_change(name, dialect):
    once = _normalised(name, "keep", dialect)
    assert once.indices == list(range(once.frames))
    before, after = _reports(_stream(name), dialect), _reports(once.data, dialect)
    for command in before:
        assert json.dumps(after[command], sort_keys=True) == json.dumps(before[command], sort_keys=True), command


@corpora
@both
def test_the_output_reads_the_same_in_either_dialect(name, dialect):
    once = _normalised(name, "drop", dialect)
    assert len(once.indices) == once.events < once.frames
    assert _reports(once.data, dialect) == _reports(once.data, OTHER[dialect])
    other = normalise_cpu(once.data, Policy("drop"), OTHER[dialect])  # a fixed point under the other dialect
    assert other.data == once.data and other.rewritten == 0 and other.events == once.events


@corpora
def test_dedupe_after_normalise_keeps_fewer_frames(name):
    alone, after = DEDUPE_KEPT[name]
    assert len(dedupe.dedupe_cpu(_stream(name)).indices) == alone
    for dialect in ops.DIALECTS:
        kept = len(dedupe.dedupe_cpu(_normalised(name, "keep", dialect).data).indices)
        assert kept == after[dialect] < alone


def test_a_frame_can_grow():
    """On the fold corpus under protobufjs: a negative int32 from a 5-byte varint, and U+FFFD."""
    once = _normalised("fold_corpus", "keep", "protobufjs")
    growth = [(b2 - a2) - (b - a) for (a, b), (a2, b2) in zip(_spans(_stream("fold_corpus")), _spans(once.data))]
    assert sum(g > 0 for g in growth) == 160 and max(growth) == 22


def _small() -> list:
    return [(STATUS_ID, b"\x10\x00\x0a\x01m"), (PROGRESS_ID, b"\x18\x05\x10\x02\x0a\x01m"), (9, b"other"),
            (PROGRESS_ID, b"\x2e"), (STATUS_ID, b"\x0a\x01m\x10\x03"), (STATUS_ID, b""), (PROGRESS_ID, b"\x0a\x02\xc3\xa9"),
            (PROGRESS_ID, b"\x10\xff\xff\xff\xff\x0f")]


@both
@pytest.mark.parametrize("undecoded", ["keep", "drop"])
def test_merge_equals_the_whole_at_every_cut(dialect, undecoded):
    events = _small()
    policy = Policy(undecoded)
    whole = normalise_cpu(frames(events), policy, dialect)
    assert whole.frames == len(events) and whole.events == 6 and whole.rewritten == 3
    for cut in range(len(events) + 1):
        a, b = normalise_cpu(frames(events[:cut]), policy, dialect), normalise_cpu(frames(events[cut:]), policy, dialect)
        before = (a.data, list(a.indices), b.data, list(b.indices))
        assert a.merge(b) == whole
        assert (a.data, a.indices, b.data, b.indices) == before
    with pytest.raises(ValueError):
        whole.merge(normalise_cpu(b"", policy, OTHER[dialect]))
    with pytest.raises(ValueError):
        whole.merge(normalise_cpu(b"", Policy("drop" if undecoded == "keep" else "keep"), dialect))


@both
def test_normalise_file_in_small_chunks_equals_one_call(dialect):
    whole = _stream("fold_corpus")
    data = whole[:max(end for _, end in _spans(whole) if end <= 40_000)]  # about 800 frames
    for undecoded in ("keep", "drop"):
        want = normalise_cpu(data, Policy(undecoded), dialect)
        for chunk_bytes in (300, 1 << 20):
            out, indices = io.BytesIO(), io.StringIO()
            counts = normalise_file(io.BytesIO(data), out, Policy(undecoded), "cpu", dialect, chunk_bytes, indices)
            assert out.getvalue() == want.data
            assert [int(line) for line in indices.getvalue().split()] == want.indices
            assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                              "in_bytes": len(data), "events": want.events, "rewritten": want.rewritten,
                              "undecoded": want.frames - want.events, "host_frames": 0}


def test_each_chunk_is_written_before_the_next_is_read():
    data = frames(_small() * 20)

    class Source(io.BytesIO):
        def read(self, size=-1):
            reads.append(out.tell())
            return super().read(size)
    reads, out = [], io.BytesIO()
    normalise_file(Source(data), out, chunk_bytes=64)
    assert len(reads) > 5 and reads[0] == 0 and reads == sorted(reads) and len(set(reads)) > 5


def test_a_truncated_tail_leaves_whole_frames_and_raises():
    events = _small()
    data = frames(events)
    for lost in (1, 3, 9):
        out, indices = io.BytesIO(), io.StringIO()
        with pytest.raises(ValueError):
            normalise_file(io.BytesIO(data[:-lost]), out, chunk_bytes=16, indices_out=indices)
        assert out.getvalue() == normalise_cpu(frames(events[:-1])).data
        assert indices.getvalue().split() == [str(i) for i in range(len(events) - 1)]
    with pytest.raises(ValueError):
        normalise_cpu(data[:-1])
    with pytest.raises(ValueError):
        normalise_cpu(data + b"\0\0\0\0\x01")  # an empty frame


def test_policy_validation():
    assert Policy().undecoded == "keep" and Policy("drop").undecoded == "drop"
    with pytest.raises(ValueError):
        Policy("first")
    with pytest.raises(TypeError):
        Policy(1)
    for call in (lambda: canon_of("keep"), lambda: normalise_cpu(b"", "keep"),
                 lambda: normalise_file(io.BytesIO(b""), io.BytesIO(), "drop")):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        normalise_cpu(b"", Policy(), "proto2")
    with pytest.raises(ValueError):
        normalise_file(io.BytesIO(b""), io.BytesIO(), Policy(), dialect="proto2")
    assert normalise_cpu(b"") == Normalised() and normalise_cpu(b"", Policy("drop"), "upb") == Normalised(
        dialect="upb", undecoded="drop")


def _cli(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "beholder_amd", "normalise", *args], input=stdin, capture_output=True,
                          timeout=120)


def test_the_command_line_on_the_cpu(tmp_path):
    data = frames(_small() * 3)
    source, out, indices = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "indices.txt"
    source.write_bytes(data)
    for dialect in ops.DIALECTS:
        want = normalise_cpu(data, Policy("drop"), dialect)
        r = _cli(str(source), "-o", str(out), "--indices", str(indices), "--undecoded", "drop", "--dialect", dialect,
                 "--chunk-bytes", "50")
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == want.data and r.stdout == b""
        assert [int(line) for line in indices.read_text().split()] == want.indices
        counts = json.loads(r.stderr.decode().strip().splitlines()[-1])
        assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                          "in_bytes": len(data), "events": want.events, "rewritten": want.rewritten,
                          "undecoded": want.frames - want.events, "host_frames": 0}
    r = _cli(stdin=data)  # stdin to stdout, the defaults
    assert r.returncode == 0 and r.stdout == normalise_cpu(data).data
    r = _cli("-o", str(out), stdin=data[:-2])  # whole frames only, and exit code 1
    assert r.returncode == 1 and out.read_bytes() == normalise_cpu(frames((_small() * 3)[:-1])).data
    assert b"truncated" in r.stderr
    assert _cli("--undecoded", "first", stdin=data).returncode == 2


# ---- single frames, against expected bytes written out here ------------------------------------------

M = b"\x0a\x01m"  # mediaId = "m"
MINUS_ONE = b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\x01"  # -1 sign-extended to 64 bits
SINGLE = [
    # (what, topic, body, canonical body per dialect or one for both)
    ("an explicit zero status", STATUS_ID, M + b"\x10\x00", M),
    ("an explicit zero progress and an empty host", PROGRESS_ID, M + b"\x10\x02\x18\x00\x22\x00", M + b"\x10\x02"),
    ("swapped field order", PROGRESS_ID, b"\x22\x01h\x18\x07\x10\x02" + M, M + b"\x10\x02\x18\x07\x22\x01h"),
    ("a repeated scalar: the last wins", STATUS_ID, M + b"\x10\x02\x10\x03", M + b"\x10\x03"),
    ("a repeated string: the last wins", STATUS_ID, b"\x0a\x01a" + M, M),
    ("an unknown field", STATUS_ID, M + b"\x38\x05\x10\x02\x42\x02xy", M + b"\x10\x02"),
    ("a status message with fields 3 and 4", STATUS_ID, M + b"\x10\x02\x18\x07\x22\x01h", M + b"\x10\x02"),
    ("an overlong varint", STATUS_ID, M + b"\x10\x82\x80\x00", M + b"\x10\x02"),
    ("an overlong length", STATUS_ID, b"\x0a\x81\x00m", M),
    ("a 5-byte minus one", STATUS_ID, M + b"\x10\xff\xff\xff\xff\x0f", M + b"\x10" + MINUS_ONE),
    ("negative status and progress", PROGRESS_ID, b"\x10" + MINUS_ONE + b"\x18\x80\x80\x80\x80\xf8\xff\xff\xff\xff\x01",
     b"\x10" + MINUS_ONE + b"\x18\x80\x80\x80\x80\xf8\xff\xff\xff\xff\x01"),
    ("INT_MIN from 5 bytes", PROGRESS_ID, b"\x18\x80\x80\x80\x80\x08", b"\x18\x80\x80\x80\x80\xf8\xff\xff\xff\xff\x01"),
    ("an all-default message", PROGRESS_ID, b"\x0a\x00\x10\x00\x18\x00\x22\x00", b""),
    ("an empty body", STATUS_ID, b"", b""),
    ("a clamped string", STATUS_ID, b"\x10\x02\x0a\x05abc", {"protobufjs": b"\x0a\x03abc\x10\x02", "upb": KEEP}),
    ("a clamped host", PROGRESS_ID, M + b"\x22\x7fh", {"protobufjs": M + b"\x22\x01h", "upb": KEEP}),
    ("invalid UTF-8", STATUS_ID, b"\x0a\x02\xffm", {"protobufjs": b"\x0a\x04\xef\xbf\xbdm", "upb": KEEP}),
    ("valid UTF-8", STATUS_ID, b"\x0a\x02\xc3\xa9\x10\x00", b"\x0a\x02\xc3\xa9"),
    ("a decode error", PROGRESS_ID, b"\x2e", KEEP),
    ("another topic", 9, M, KEEP),
]


@both
@pytest.mark.parametrize("case", SINGLE, ids=[c[0] for c in SINGLE])
def test_single_frames(case, dialect):
    _, topic, body, want = case
    if isinstance(want, dict):
        want = want[dialect]
    assert canon_of(Policy(), dialect)(topic, body) == want
    assert canon_of(Policy("drop"), dialect)(topic, body) == (DROP if want is KEEP else want)
    got = normalise_cpu(frames([(topic, body)]), Policy(), dialect)
    new = body if want is KEEP else want
    assert got == Normalised(nm.frame_of(topic, new), [0], 1, int(want is not KEEP),
                             int(want is not KEEP and want != body), dialect, "keep")
    if want == b"":
        assert got.data == b"\x01\0\0\0" + bytes([topic]) and len(got.data) == 5
    dropped = normalise_cpu(frames([(topic, body)]), Policy("drop"), dialect)
    assert dropped.indices == ([] if want is KEEP else [0]) and dropped.frames == 1
