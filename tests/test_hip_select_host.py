"""The gfx950 select kernels' predicate and media-table probe (ops/hip/telemetry_select.hpp) on a CPU,
under ASan and UBSan.

tests/native/select_host.cpp compiles the header for the host and decides every frame of a stream
from a heap block of exactly the frame's size, with the table and its id bytes in exact blocks too:
a read past any of them is a sanitizer report here. Its keep / drop lines are held to
``extract.predicate``, the definition, for every selector kind in both dialects; its host lines to
the rule that hands a frame to the host. The table is the one ``gpu_extract.build_media_table``
builds, so this also checks the Python builder against the C probe. Nothing is loaded into Python
under a sanitizer."""
from __future__ import annotations

import os
import random
import shutil
import subprocess

import pytest

from beholder_amd import extract as ex, ops
from beholder_amd.extract import Selector
from beholder_amd.models import proto
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_extract as gx, gpu_fold  # noqa: E402
import wire_edges  # noqa: E402
from extract_cases import KINDS, collision_pairs  # noqa: E402
from telemetry_corpus import body as _body, fold_corpus  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "beholder_amd", "ops", "hip")
TYPES = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}


@pytest.fixture(scope="module")
def program(tmp_path_factory) -> str:
    """The flags of tests/native/Makefile's readers_host_asan rule."""
    out = str(tmp_path_factory.mktemp("select_host") / "select_host_asan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", f"-I{HIP}", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "select_host.cpp"), "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return out


def _decisions(program: str, dialect: str, stream: bytes, selector: Selector, tmp_path, hash_mask=gpu_fold.ALL_ONES):
    """The program's line per frame of ``stream``; any sanitizer report fails."""
    ids = gx.ascii_ids(selector.media)
    table, blob = gx.build_media_table(ids, hash_mask)
    params = gx.select_params(selector, len(table), hash_mask)
    files = {"stream": stream, "params": bytes(params), "table": table.tobytes(), "blob": blob.tobytes()}
    for name, content in files.items():
        (tmp_path / name).write_bytes(content)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([program, dialect] + [str(tmp_path / name) for name in files], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-4000:]  # both sanitizers abort on a finding
    return r.stdout.split()


def _high(text: str) -> bool:
    return not text.isascii()


def _against_the_definition(stream: bytes, got: list, selector: Selector, dialect: str) -> int:
    """Asserts the decisions; returns how many frames went to the host."""
    keep = ex.predicate(selector, dialect)
    events = list(iter_frames(stream))
    assert len(got) == len(events)
    codecs = {t: ops.codec_for(p, dialect) for t, p in TYPES.items()}
    host, bad = 0, []
    for i, ((topic, body), word) in enumerate(zip(events, got)):
        if word == "host":
            host += 1
            assert topic in TYPES, (i, topic)
            if dialect == "protobufjs":  # the rule in full: it decodes, and its id is not ASCII
                assert _high(codecs[topic].decode(body).mediaId), (i, body)
            continue
        if dialect == "protobufjs" and topic in TYPES:
            try:
                assert not _high(codecs[topic].decode(body).mediaId), (i, body)  # ... and no other frame
            except proto.DecodeError:
                pass
        if word != ("keep" if keep(topic, body) else "drop"):
            bad.append((i, topic, body, word))
    assert not bad, (len(bad), bad[:5])
    return host


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_predicate_agrees_with_the_definition_on_the_fold_corpus(program, tmp_path, kind, dialect):
    stream = fold_corpus()
    got = _decisions(program, dialect, stream, KINDS[kind], tmp_path)
    host = _against_the_definition(stream, got, KINDS[kind], dialect)
    assert len(got) > 5000 and 0 < host <= 0.05 * len(got)  # the comparison covers what the device decides itself
    if kind not in ("all", "combined"):
        assert "keep" in got and "drop" in got


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_predicate_agrees_with_the_definition_on_the_wire_edges(program, tmp_path, dialect):
    """Under a selector that keeps by media and by status; ``_against_the_definition`` holds the host
    set to the rule in both directions under protobufjs."""
    stream, selector = wire_edges.stream(), wire_edges.selector()
    got = _decisions(program, dialect, stream, selector, tmp_path)
    host = _against_the_definition(stream, got, selector, dialect)
    print(f"{dialect}: {len(got)} frames, {host} left to the host")
    assert len(got) == 2 * len(wire_edges.bodies()) and got.count("keep") > 1000 and got.count("drop") > 1000
    assert host <= wire_edges.HOST_CAP[dialect] * len(got)


def test_the_host_set_does_not_depend_on_the_selector(program, tmp_path):
    stream = fold_corpus()
    for dialect in ops.DIALECTS:
        sets = {kind: [i for i, w in enumerate(_decisions(program, dialect, stream, KINDS[kind], tmp_path))
                       if w == "host"] for kind in ("all", "media", "combined-inverted")}
        assert sets["all"] == sets["media"] == sets["combined-inverted"]


@pytest.mark.parametrize("hash_mask", [0x3, 0])
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_forced_collisions_are_decided_by_the_bytes(program, tmp_path, dialect, hash_mask):
    """hash_mask 0x3 homes all 60 queried ids in four slots (0: in one), so every probe walks a chain
    of entries of its own length; each -y id differs from a queried -x id in its last byte only."""
    pairs = collision_pairs()
    rng = random.Random(5)
    events = [(rng.choice((STATUS_ID, PROGRESS_ID)), _body(mid, rng.randrange(6))) for pair in pairs for mid in pair]
    events += [(STATUS_ID, _body(b"", 1)), (PROGRESS_ID, _body(b"pair-000-", 1)), (PROGRESS_ID, _body(b"pair-000-xx", 1))]
    rng.shuffle(events)
    stream = frames(events)
    selector = Selector(media={x.decode() for x, _ in pairs})
    got = _decisions(program, dialect, stream, selector, tmp_path, hash_mask)
    assert _against_the_definition(stream, got, selector, dialect) == 0
    assert got.count("keep") == 60 and got.count("drop") == 63


def test_the_table_builder():
    ids = [b"", b"a", b"ab", b"a\0"] + [x for pair in collision_pairs() for x in pair]
    assert gx.hash64_many(ids).tolist() == [gpu_fold.hash64(b) for b in ids]
    assert gx.hash64_many([]).tolist() == []
    assert [gx.table_slots(k) for k in (0, 1, 2, 3, 60, 64, 65)] == [2, 2, 4, 8, 128, 128, 256]
    table, blob = gx.build_media_table(ids, 0x3)
    assert len(table) == 256 and (table["len"] >= 0).sum() == len(ids)
    stored = {bytes(blob[e["off"]:e["off"] + e["len"]]) for e in table if e["len"] >= 0}
    assert stored == set(ids)
    assert gx.ascii_ids({"b", "é", "a", "�"}) == [b"a", b"b"]
    empty, blob = gx.build_media_table([])
    assert len(empty) == 2 and (empty["len"] == -1).all() and len(blob) == 1
