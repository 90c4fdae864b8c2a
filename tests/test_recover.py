"""``recover`` on the CPU (beholder_amd/recover.py): the definition's laws, the damages one by one, and
``recover_file`` in chunks against the whole buffer."""
from __future__ import annotations

import io
import json
import struct

import pytest

from beholder_amd import ops, recover as rc
from beholder_amd.capture_io import frame_spans
from beholder_amd.recover import Policy, Recovered, recover_cpu, recover_file

import recover_cases as cases  # noqa: E402
from recover_cases import JUNK  # noqa: E402

SMALL = Policy(64)


def _laws(data: bytes, got: Recovered) -> None:
    """What holds for every final result."""
    assert got.in_bytes == got.consumed == len(data)
    assert got.resync == (bool(got.gaps) and sum(got.gaps[-1]) == len(data))  # a gap was open at the end
    assert got.frames == len(got.offsets) and got.intact == (not got.gaps)
    assert got.offsets == sorted(set(got.offsets))
    at = 0
    for offset, length in got.gaps:  # ascending, disjoint, never empty, and not touching
        assert length > 0 and (offset > at or (offset == 0 and at == 0))
        at = offset + length
    assert at <= len(data)
    assert got.in_bytes == len(got.data) + sum(length for _, length in got.gaps)
    keep, at = [], 0
    for offset, length in got.gaps:
        keep.append(data[at:offset])
        at = offset + length
    assert got.data == b"".join(keep) + data[at:]
    spans = list(frame_spans(got.data))  # the output always passes the framing walk
    assert len(spans) == got.frames
    shift, gaps = 0, list(got.gaps)
    for (a, b), o in zip(spans, got.offsets):  # and every output frame is the input's bytes at its offset
        while gaps and gaps[0][0] <= o - 0 and gaps[0][0] + gaps[0][1] <= o:
            shift += gaps.pop(0)[1]
        assert a + shift == o and got.data[a:b] == data[o:o + b - a]


def _recover(data: bytes, policy: Policy = SMALL, dialect: str = "protobufjs") -> Recovered:
    got = recover_cpu(data, policy, dialect)
    _laws(data, got)
    again = recover_cpu(got.data, policy, dialect)  # recover of its own output is the identity
    assert again.data == got.data and again.intact and again.frames == got.frames
    return got


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", cases.CORPORA)
def test_an_intact_capture_comes_back_byte_for_byte(name, dialect):
    data = cases.corpus(name)
    got = _recover(data, Policy(), dialect)
    assert got.data == data and got.gaps == [] and got.intact and got.anchors == 0
    assert got.offsets == [a for a, _ in frame_spans(data)]
    assert got.dialect == dialect and got.max_frame == 1 << 20


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("max_frame", cases.MAX_FRAMES)
def test_the_laws_on_every_damage_case(max_frame, dialect):
    for name, data in cases.damage_cases().items():
        _recover(data, Policy(max_frame), dialect)


def test_a_torn_tail_leaves_the_frames_before_it_and_one_gap():
    f = cases.five()
    whole, starts = b"".join(f), cases.starts(f)
    for k in list(range(1, len(f[4]))):  # inside the body, and with 1, 2 or 3 bytes of the header left
        got = _recover(whole[:-k])
        assert got.offsets == starts[:4] and got.gaps == [(starts[4], len(f[4]) - k)] and got.anchors == 0
        assert got.data == whole[:starts[4]]
    assert len(f[4]) - 3 in range(1, len(f[4]))  # the header cuts are among them
    assert _recover(whole).intact


def test_lengths_at_the_bounds():
    d = cases.damage_cases()
    f = cases.five()
    a = len(f[0])
    got = _recover(d["length_0"])
    assert got.gaps == [(a, 5)] and got.frames == 3 and got.anchors == 1
    got = _recover(d["length_max_frame_64"])
    assert got.intact and got.frames == 3
    got = _recover(d["length_max_frame_64_plus_1"])  # one byte above max_frame: skipped to the next anchor
    assert got.gaps == [(a, 69)] and got.offsets == [0, a + 69, a + 69 + len(f[1])]
    assert _recover(d["length_max_frame_64_plus_1"], Policy(65)).intact
    assert _recover(d["ends_exactly_at_n"]).intact
    got = _recover(d["would_end_at_n_plus_1"])
    assert got.frames == 5 and got.gaps == [(len(b"".join(f)), 67)]


def test_zeros_and_garbage():
    d = cases.damage_cases()
    f = cases.five()
    got = _recover(d["zeros"])
    assert got.gaps == [(len(f[0]), 40)] and got.frames == 3 and got.anchors == 1
    got = _recover(d["garbage_at_0"])
    assert got.gaps == [(0, len(JUNK))] and got.frames == 5 and got.anchors == 1 and got.data == b"".join(f)
    for name in ("garbage_only", "noise_only"):
        got = _recover(d[name])
        assert got.frames == 0 and got.gaps == [(0, len(d[name]))] and got.data == b""
    got = _recover(d["two_gaps_one_frame_between"])
    s = cases.starts([f[0], JUNK, f[1], f[2], JUNK * 2, f[3], f[4]])
    assert got.gaps == [(s[1], 7), (s[4], 14)] and got.offsets == [s[0], s[2], s[3], s[5], s[6]] and got.anchors == 2
    got = _recover(d["anchor_with_a_damaged_successor"])  # f[1] is followed by junk: no anchor; f[2] is taken
    s = cases.starts([f[0], JUNK, f[1], JUNK, f[2], f[3]])
    assert got.gaps == [(s[1], s[4] - s[1])] and got.offsets == [s[0], s[4], s[5]] and got.anchors == 1
    assert _recover(b"").intact and _recover(b"").frames == 0
    for n in range(1, 5):
        assert _recover(b"\x01" * n).gaps == [(0, n)]


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_frames_that_are_kept_in_sync_and_are_no_anchor(dialect):
    d = cases.damage_cases()
    f = cases.five()
    got = _recover(d["in_sync_frames_that_are_no_anchor"], SMALL, dialect)
    assert got.intact and got.frames == 6 and got.anchors == 0
    got = _recover(d["no_anchor_among_the_candidates"], SMALL, dialect)
    middle = len(JUNK) + len(cases.EMPTY_ID) + len(cases.OTHER_TOPIC) + len(cases.BROKEN)
    assert got.gaps == [(len(f[0]), middle)] and got.frames == 3 and got.anchors == 1


def test_a_damaged_length_that_still_fits_is_found_out_by_what_follows():
    """The frame before the gap is the one to distrust: it is made of the head of one frame and more."""
    d = cases.damage_cases()["a_damaged_length_that_still_fits"]
    got = _recover(d)
    f = cases.five()
    assert got.offsets[:2] == [0, len(f[0])] and len(got.gaps) == 1 and got.gaps[0][0] == len(f[0]) + 24
    assert "distrust" in rc.__doc__


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_damaged_fold_corpus(dialect):
    data, k = cases.damaged("fold_corpus")
    got = _recover(data, Policy(), dialect)
    print(f"fold_corpus {dialect}: {got.frames} of {k} frames, gaps {got.gaps}")
    assert len(got.gaps) == 4 and got.frames >= k - 6 and got.gaps[-1][0] + got.gaps[-1][1] == len(data)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_damaged_wire_edges(dialect):
    data, k = cases.damaged("wire_edges")
    got = _recover(data, Policy(), dialect)
    print(f"wire_edges {dialect}: {got.frames} of {k} frames, gaps {got.gaps}")
    assert len(got.gaps) == 4


def _file(data: bytes, policy: Policy, dialect: str, chunk_bytes: int):
    out, gaps, offsets = io.BytesIO(), io.StringIO(), io.StringIO()
    counts = recover_file(io.BytesIO(data), out, policy, "cpu", dialect, chunk_bytes, gaps_out=gaps, offsets_out=offsets)
    rows = [json.loads(line) for line in gaps.getvalue().splitlines()]
    return counts, out.getvalue(), rows, [int(line) for line in offsets.getvalue().split()]


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("max_frame", cases.MAX_FRAMES)
def test_recover_file_in_chunks_equals_the_whole_buffer(max_frame, dialect):
    """Damage that straddles a cut, a gap longer than two chunks, a cut in an intact run: all of them
    come with chunks of ``2 * H`` and a few bytes more over these buffers."""
    policy = Policy(max_frame)
    h = rc.horizon(policy)
    for name, data in cases.damage_cases().items():
        want = recover_cpu(data, policy, dialect)
        for chunk_bytes in (2 * h, 2 * h + 1, 2 * h + 7, 3 * h + 5, 1 << 20):
            counts, out, rows, offsets = _file(data, policy, dialect, chunk_bytes)
            assert out == want.data and offsets == want.offsets, (name, chunk_bytes)
            assert [(r["offset"], r["length"]) for r in rows] == want.gaps, (name, chunk_bytes)
            assert [r["after_frame"] for r in rows] == [sum(o < a for o in want.offsets) - 1 for a, _ in want.gaps]
            sizes = [length for _, length in want.gaps]
            assert counts == {"in_bytes": len(data), "kept_bytes": len(want.data), "frames": want.frames,
                              "anchors": want.anchors, "gaps": len(sizes), "gap_bytes": sum(sizes),
                              "largest_gap": max(sizes, default=0), "intact": want.intact, "host_offsets": 0}
    assert len(cases.damage_cases()["gap_longer_than_two_chunks"]) > 900 > 2 * 2 * rc.horizon(SMALL)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_parts_merge_to_the_whole(dialect):
    """The unit the file driver calls, by hand: parts with ``final=False`` and the carried ``resync``."""
    h = rc.horizon(SMALL)
    for name, data in cases.damage_cases().items():
        want = recover_cpu(data, SMALL, dialect)
        for size in (2 * h, 2 * h + 3):
            merged, at, resync = None, 0, False
            while True:
                piece = data[at:at + size]
                final = at + size >= len(data)
                part = recover_cpu(piece, SMALL, dialect, final=final, resync=resync)
                assert part.consumed <= len(piece) and (final or part.consumed > len(piece) - h)
                merged = part if merged is None else merged.merge(part)
                at, resync = at + part.consumed, part.resync
                if final:
                    break
            assert (merged.data, merged.offsets, merged.gaps, merged.anchors) == \
                (want.data, want.offsets, want.gaps, want.anchors), (name, size)
            assert merged == want
            based = recover_cpu(data[:size], SMALL, dialect, final=False, base=1000)
            plain = recover_cpu(data[:size], SMALL, dialect, final=False)
            assert based.offsets == [o + 1000 for o in plain.offsets] and based.data == plain.data


def test_a_part_that_is_not_the_last_decides_nothing_near_its_end():
    f = cases.five()
    h = rc.horizon(SMALL)
    data = b"".join(f) * 10
    part = recover_cpu(data, SMALL, final=False)
    assert len(data) - h < part.consumed <= len(data) and not part.resync and part.intact
    assert recover_cpu(data[:h - 1], SMALL, final=False) == Recovered(max_frame=64)  # nothing decided at all
    part = recover_cpu(data[:len(data) - h - 5] + JUNK * 30, SMALL, final=False)
    assert part.resync and part.consumed == len(part.data) + part.gaps[-1][1] == len(data) - h - 5 + 210 - h + 1
    entered = recover_cpu(JUNK + data, SMALL, final=True, resync=True)
    assert entered.gaps == [(0, 7)] and entered.anchors == 1 and entered.frames == 50
    entered = recover_cpu(data, SMALL, final=True, resync=True)  # offset 0 is a candidate itself
    assert entered.intact and entered.anchors == 1 and entered.frames == 50


def test_policy_and_argument_checks():
    for bad in (0, -1, (16 << 20) + 1):
        with pytest.raises(ValueError):
            Policy(bad)
    for bad in (True, 1.0, "64", None):
        with pytest.raises(TypeError):
            Policy(bad)
    assert Policy().max_frame == 1 << 20 and Policy(16 << 20).max_frame == 16 << 20 and Policy(1).max_frame == 1
    with pytest.raises(TypeError):
        recover_cpu(b"", 64)
    with pytest.raises(ValueError):
        recover_cpu(b"", Policy(), "proto2")
    with pytest.raises(TypeError):
        recover_cpu(b"", Policy(), final=1)
    with pytest.raises(ValueError):
        recover_cpu(b"", Policy(), base=-1)
    h = rc.horizon(SMALL)
    with pytest.raises(ValueError, match="--max-frame.*--chunk-bytes|--chunk-bytes.*--max-frame"):
        recover_file(io.BytesIO(b""), io.BytesIO(), SMALL, chunk_bytes=2 * h - 1)
    with pytest.raises(ValueError, match="--chunk-bytes"):
        recover_file(io.BytesIO(b""), io.BytesIO(), Policy(), chunk_bytes=1 << 20)
    assert recover_file(io.BytesIO(b""), io.BytesIO(), SMALL, chunk_bytes=2 * h)["intact"]
    with pytest.raises(ValueError):
        recover_file(io.BytesIO(b""), io.BytesIO(), SMALL, dialect="proto2")
    with pytest.raises(TypeError):
        recover_file(io.BytesIO(b""), io.BytesIO(), 64)
    a = recover_cpu(cases.five()[0], SMALL)
    with pytest.raises(ValueError, match="max_frame"):
        a.merge(recover_cpu(b"", Policy(65)))
    with pytest.raises(ValueError, match="dialect"):
        a.merge(recover_cpu(b"", SMALL, "upb"))
    assert struct.unpack("<I", a.data[:4])[0] == len(a.data) - 4
