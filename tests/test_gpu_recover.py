"""``recover`` on the GPU (ops/hip/telemetry_recover.hip, ops/gpu_recover.py) against its definition,
``recover.recover_cpu``: every comparison is full ``Recovered`` equality (the output bytes, the
offsets, the gaps, the counts, ``consumed`` and ``resync``), exact."""
from __future__ import annotations

import functools
import io
import json

import pytest

from beholder_amd import ops, recover as rc
from beholder_amd.recover import Policy, Recovered, recover_cpu, recover_file, recover_gpu

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_extract, gpu_recover as gr, hip_lib  # noqa: E402
import recover_cases as cases  # noqa: E402
from recover_cases import JUNK, MINIMAL  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
SMALL = Policy(64)
BLOCK = gr.BLOCK


@functools.lru_cache(maxsize=None)
def _want(data: bytes, policy: Policy, dialect: str, final: bool = True, resync: bool = False) -> Recovered:
    return recover_cpu(data, policy, dialect, final=final, resync=resync)


def _same(data: bytes, policy: Policy = SMALL, dialect: str = "protobufjs", final: bool = True, resync: bool = False):
    """Asserts the device result against the definition, field by field; returns
    ``(Recovered, host_offsets)``."""
    want = _want(data, policy, dialect, final, resync)
    got, host_offsets = gr.recover(data, policy, DEVICE, dialect, final=final, resync=resync)
    assert (got.consumed, got.resync, got.in_bytes) == (want.consumed, want.resync, want.in_bytes)
    assert got.gaps == want.gaps
    assert got.offsets == want.offsets
    assert (got.frames, got.anchors, got.dialect, got.max_frame, got.base) == \
        (want.frames, want.anchors, want.dialect, want.max_frame, want.base)
    assert got.data == want.data
    assert got == want
    return want, host_offsets


def _all(data: bytes, policy: Policy = SMALL) -> list:
    return [_same(data, policy, dialect) for dialect in ops.DIALECTS]


def test_empty_buffer_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty buffer must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for dialect in ops.DIALECTS:
        for resync in (False, True):
            want = recover_cpu(b"", SMALL, dialect, resync=resync)
            assert gr.recover(b"", SMALL, DEVICE, dialect, resync=resync) == (want, 0)
            assert recover_gpu(b"", SMALL, DEVICE, dialect, resync=resync) == want and want.resync == resync
    out = io.BytesIO()
    assert recover_file(io.BytesIO(b""), out, Policy(), DEVICE)["frames"] == 0 and out.getvalue() == b""


def test_buffers_of_1_to_9_bytes():
    status = cases.status(b"m", 2)  # 10 bytes
    for n in range(1, 10):
        for data in (MINIMAL[:n], (MINIMAL * 2)[:n], status[:n], b"\x00" * n, b"\xff" * n, (JUNK + MINIMAL)[-n:]):
            _all(data)
    assert _same(MINIMAL)[0].frames == 1 and _same(status, resync=True)[0].anchors == 1


@pytest.mark.parametrize("edge", [BLOCK, 2 * BLOCK])
def test_a_header_across_the_edge_of_a_candidate_block_and_its_halo(edge):
    """A frame whose header starts 0 to 6 bytes before the block's edge: its length bytes and its topic
    byte come from the halo. The anchor behind a gap does the same."""
    for back in range(0, 7):
        lead = edge - back - len(JUNK)
        prefix = MINIMAL * (lead // 5 - 1) + cases.frame(9, b"p" * (lead % 5))  # frames that are no anchor
        assert len(prefix) == lead
        tail = cases.status(b"m-1", 2) + cases.progress() + MINIMAL
        want, _ = _same(prefix + JUNK + tail)  # the anchor's header straddles the edge
        assert want.gaps == [(lead, 7)] and want.anchors == 1 and want.offsets[-3] == edge - back
        want, _ = _same(prefix + MINIMAL + b"\x01" + tail)  # in sync up to the edge, then one stray byte
        assert want.anchors == 1 and len(want.gaps) == 1


@pytest.mark.parametrize("at", [0, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 3 * BLOCK])
def test_an_anchor_at_the_first_and_the_last_offset_of_a_scan_block(at):
    """The one anchor of the buffer sits at ``at``; everything before it is a gap of noise in which no
    header fits, so ``next`` has to carry it across every block before it."""
    anchor = cases.status(b"m-1", 2)
    for tail in (b"", MINIMAL * 3, MINIMAL * 60):
        for resync in (False, True):
            want, _ = _same(b"\xff" * at + anchor + tail, resync=resync)
            assert want.offsets[0] == at and want.gaps == ([(0, at)] if at else [])
            assert want.anchors == (1 if at or resync else 0)  # in sync at 0 it is a frame like any other
    if at:
        want, _ = _same(b"\xff" * at + anchor + JUNK)  # followed by damage: no anchor after all
        assert want.frames == 0 and want.gaps == [(0, at + len(anchor) + 7)]


def test_no_anchor_anywhere():
    for data in (b"\xff" * 1000, bytes(1000), cases.damage_cases()["noise_only"], JUNK + MINIMAL * 300,
                 JUNK + cases.EMPTY_ID * 100):
        for resync in (False, True):
            for dialect in ops.DIALECTS:
                want, _ = _same(data, SMALL, dialect, resync=resync)
                assert want.frames == 0 and want.gaps == [(0, len(data))] and want.resync


def _counts():
    out = {1, 2, 3}
    for k in range(2, 13):
        out |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    return sorted(out)


def test_hop_counts_around_a_doubling_round():
    """Streams of minimal 5-byte frames: the longest walk a buffer of its size can hold."""
    for count in _counts():
        want, _ = _same(MINIMAL * count)
        assert want.frames == count and want.intact
    for count in (7, 8, 9, 1023, 1024, 1025):  # the same walks behind a gap, and torn
        want, _ = _same(JUNK + cases.status() + MINIMAL * count + b"\x01\x00")
        assert want.frames == count + 1 and len(want.gaps) == 2


def test_one_frame_that_spans_several_blocks():
    big = cases.frame(9, b"\x00" * 1000)
    status = cases.frame(1, b"\x0a\xe0\x07" + b"i" * 992 + b"\x10\x02")
    policy = Policy(1024)
    for data in (big, MINIMAL + big + MINIMAL, JUNK + status + big, big + JUNK + status, status[:-1], JUNK + status[:-1]):
        _all(data, policy)
    assert _same(JUNK + status + big, policy)[0].anchors == 1
    assert _same(big + MINIMAL, SMALL)[0].frames == 0  # above max_frame: no frame at all


@pytest.mark.parametrize("count", [gpu_extract.SCAN_BLOCK, gpu_extract.SCAN_BLOCK + 1])
def test_a_scan_block_of_frames_and_one_more(count):
    f = cases.five()
    data = b"".join(f[k % 5] for k in range(count))
    assert _same(data)[0].frames == count
    want, _ = _same(data[:400] + JUNK + data[400:])
    assert len(want.gaps) == 1 and want.frames >= count - 2


@pytest.mark.parametrize("max_frame", cases.MAX_FRAMES)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_every_damage_case(dialect, max_frame):
    asked = 0
    for name, data in cases.damage_cases().items():
        asked += _same(data, Policy(max_frame), dialect)[1]
    assert (asked > 0) == (dialect == "upb")


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_parts_that_are_not_the_last(dialect):
    h = rc.horizon(SMALL)
    d = cases.damage_cases()
    for name in ("damage_in_a_long_run", "gap_longer_than_two_chunks", "garbage_at_0", "long_intact_run", "one_frame",
                 "noise_only", "non_ascii_id"):
        for resync in (False, True):
            for data in (d[name], d[name][:2 * h], d[name][5:2 * h + 9], d[name][:h - 1], d[name][:h], d[name][:h + 1]):
                want, _ = _same(data, SMALL, dialect, final=False, resync=resync)
                assert want.consumed <= len(data) and (len(data) < h or want.consumed > len(data) - h)


def test_the_offsets_left_to_the_host_under_upb():
    f = cases.five()
    d = cases.damage_cases()
    for name, count in (("non_ascii_id", 2), ("group_behind_a_gap", 1), ("non_ascii_host", 2)):
        want, host_offsets = _same(d[name], SMALL, "upb")
        assert host_offsets == count and len(want.gaps) >= 1
        assert _same(d[name], SMALL, "protobufjs")[1] == 0
    # valid UTF-8 is an anchor under upb, invalid is none; protobufjs takes both
    bad = cases.status(b"\xff\xfe")
    data = f[0] + JUNK + bad + f[1]
    assert _same(data, SMALL, "upb")[0].offsets == [0, len(f[0]) + 7 + len(bad)]
    assert _same(data, SMALL, "protobufjs")[0].offsets == [0, len(f[0]) + 7, len(f[0]) + 7 + len(bad)]


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", cases.CORPORA)
def test_the_corpora_intact_and_damaged(name, dialect):
    data = cases.corpus(name)
    want, host_offsets = _same(data, Policy(), dialect)
    assert want.intact and want.data == data
    print(f"{name} {dialect} intact: {host_offsets} of {len(data)} offsets left to the host")
    assert dialect == "upb" or host_offsets == 0
    broken, _ = cases.damaged(name)
    want, host_offsets = _same(broken, Policy(), dialect)
    assert len(want.gaps) == 4
    print(f"{name} {dialect} damaged: {host_offsets} of {len(broken)} offsets left to the host")
    assert recover_gpu(broken, Policy(), DEVICE, dialect) == want  # the public call


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_recover_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device."""
    data, _ = cases.damaged("fold_corpus")
    policy = Policy(4096)
    chunk_bytes = 30_000
    assert len(data) > 7 * chunk_bytes and chunk_bytes >= 2 * rc.horizon(policy)
    want = _want(data, policy, dialect)
    for size in (chunk_bytes, 1 << 28):
        out, gaps, offsets = io.BytesIO(), io.StringIO(), io.StringIO()
        counts = recover_file(io.BytesIO(data), out, policy, DEVICE, dialect, chunk_bytes=size, gaps_out=gaps,
                              offsets_out=offsets)
        assert out.getvalue() == want.data
        assert [int(line) for line in offsets.getvalue().split()] == want.offsets
        rows = [json.loads(line) for line in gaps.getvalue().splitlines()]
        assert [(r["offset"], r["length"]) for r in rows] == want.gaps
        assert (counts["frames"], counts["anchors"], counts["gaps"], counts["in_bytes"], counts["intact"]) == \
            (want.frames, want.anchors, 4, len(data), False)
        assert (counts["host_offsets"] == 0) == (dialect == "protobufjs")


def test_recover_is_deterministic():
    data, _ = cases.damaged("fold_corpus")
    first = recover_gpu(data, Policy(), DEVICE, "upb")
    assert first == recover_gpu(data, Policy(), DEVICE, "upb") == _want(data, Policy(), "upb")


def test_the_size_check_raises_before_any_upload(monkeypatch):
    def no_upload(*a, **kw):
        raise AssertionError("the size check comes first")
    monkeypatch.setattr(gr, "upload", no_upload)
    monkeypatch.setattr(hip_lib, "lib", no_upload)

    class Huge(bytes):
        def __len__(self):
            return gr.LIMIT + 1
    with pytest.raises(ValueError, match="2684354") as e:
        gr.recover(Huge(), Policy(), DEVICE)
    assert isinstance(e.value, gr.TooLarge)
    gr.check_size(gr.LIMIT)
    with pytest.raises(gr.TooLarge):
        gr.check_size(gr.LIMIT + 1)
    assert gr.LIMIT == 2 ** 28


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = cases.five()[0] * 3
    buf = gr.upload(data, DEVICE)
    tables = gr.allocate(buf, len(data), SMALL)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gr.allocate(buf.to(torch.int32), len(data), SMALL)  # wrong dtype
    with pytest.raises(ValueError):
        gr.allocate(buf.cpu(), len(data), SMALL)  # a host tensor
    with pytest.raises(ValueError):
        gr.allocate(buf, 0, SMALL)  # n >= 1
    with pytest.raises(ValueError):
        gr.allocate(buf, buf.numel(), SMALL)  # no room for the halo
    with pytest.raises(ValueError):
        gr.allocate(buf[1:], len(data), SMALL)  # not upload()'s
    with pytest.raises(TypeError):
        gr.allocate(buf, len(data), 64)
    with pytest.raises(TypeError):
        gr.allocate(buf, len(data), SMALL, final=1)
    bad = Policy()
    object.__setattr__(bad, "max_frame", (16 << 20) + 1)  # a policy that got past its own check
    for call in (lambda: gr.allocate(buf, len(data), bad), lambda: gr.recover(data, bad, DEVICE)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        gr.candidates(tables, dialect="proto2")
    with pytest.raises(TypeError):
        gr.reach(tables, resync=1)
    with pytest.raises(TypeError):
        gr.recover(data, 64, DEVICE)
    with pytest.raises(ValueError):
        recover_gpu(data, SMALL, DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        recover_gpu(data, SMALL, "cpu")
    with pytest.raises(TypeError):
        recover_gpu(data, SMALL, DEVICE, final=1)
    with pytest.raises(ValueError):
        recover_gpu(data, SMALL, DEVICE, base=-1)
    with pytest.raises(ValueError, match="--chunk-bytes"):
        recover_file(io.BytesIO(data), io.BytesIO(), SMALL, DEVICE, chunk_bytes=100)
