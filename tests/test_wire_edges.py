"""The systematic wire-format corpus (wire_edges.py): that it reaches what it claims to reach, and the
plain-Python row definitions of ``ops/gpu_decode.py`` against the service's codecs on every body of
it. The readers compiled for the host run over it in test_hip_readers_host.py, the per-frame headers
in the other test_hip_*_host.py files, the device in test_gpu_wire_edges.py."""
from __future__ import annotations

import pytest

from beholder_amd import ops
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_decode as gd, gpu_fold  # noqa: E402
import wire_edges  # noqa: E402


def test_the_corpus_is_deterministic_sorted_and_small():
    bodies = wire_edges.bodies()
    assert list(bodies) == sorted(set(bodies))
    assert len(bodies) <= wire_edges.MAX_BODIES and sum(map(len, bodies)) <= wire_edges.MAX_BYTES
    wire_edges.bodies.cache_clear()
    assert wire_edges.bodies() == bodies
    print(f"{len(bodies)} bodies, {sum(map(len, bodies))} bytes")


def test_the_stream_frames_every_body_on_both_topics():
    bodies, events = wire_edges.bodies(), wire_edges.events()
    assert [b for t, b in events if t == STATUS_ID] == [b for t, b in events if t == PROGRESS_ID] == list(bodies)
    assert wire_edges.stream() == ops.frames(list(events))
    assert len(wire_edges.expected("upb")) == len(wire_edges.expected("protobufjs")) == len(events) == 2 * len(bodies)


@pytest.mark.parametrize("limit", [6000, 500])
def test_a_thinned_stream_keeps_every_family(limit):
    picked = wire_edges.picked(limit)
    assert limit // 4 < 2 * len(picked) <= limit and set(picked) <= set(wire_edges.bodies())
    assert len(wire_edges.events(limit)) == len(wire_edges.expected("upb", limit)) == 2 * len(picked)
    families = (wire_edges._varint_family, wire_edges._wide_tag_family, wire_edges._tag_family,
                wire_edges._string_family, wire_edges._group_family)
    if limit >= 6000:
        assert all(set(family()) & set(picked) for family in families)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_the_codec_raises_on_half_the_frames_and_decodes_thousands(dialect):
    want = wire_edges.expected(dialect)
    raised = sum(v is None for v in want)
    print(f"{dialect}: the codec raises on {raised} of {len(want)} frames")
    assert 2 * raised >= len(want) and len(want) - raised >= 5000
    ids = {v.media_id for v in want if v is not None}
    assert {"", "m", "abcdef"} <= ids and any(not mid.isascii() for mid in ids)
    assert wire_edges.id_hash(wire_edges.Values("m", 0, 0, "")) == gpu_fold.hash64(b"m")


def test_every_tag_of_wire_types_0_to_7_and_fields_0_to_6_starts_a_body():
    first = {b[0] for b in wire_edges.bodies() if b}
    assert all(field << 3 | wt in first for field in range(7) for wt in range(8))


def test_the_corpus_reaches_both_sides_of_the_protobufjs_fast_path(monkeypatch):
    """``PbjsReader::uint32`` reads unchecked while ``pos + 5 <= len`` and bounds-checked after. Every
    call is filed under (bytes left, capped at 10; leading bytes with the continuation bit among the
    first five present; how it ended). A varint whose first five bytes all continue takes the 64-bit
    tail: with exactly 5 bytes left it is the last call of the fast path, with 4 left (the 5th byte
    is past the end and reads as a continuation) the first of the checked one."""
    met = set()

    class Recording(gd._PbjsReader):
        def uint32(self):
            left = min(self.len - self.pos, 10)
            continued = 0
            while continued < min(left, 5) and self.at(self.pos + continued) >= 128:
                continued += 1
            try:
                value = super().uint32()
            except gd._PbjsOverrun:
                met.add((left, continued, "overrun"))
                raise
            met.add((left, continued, "read"))
            return value

    monkeypatch.setattr(gd, "_PbjsReader", Recording)
    for body in wire_edges.bodies():
        gd.reference_decode_pbjs(body, 0, len(body))
    # the 64-bit tail on the fast side: past the end with 5..9 bytes left, inside with 10
    assert {(left, 5, "overrun") for left in range(5, 10)} | {(10, 5, "read")} <= met
    # and on the checked side, where running over is certain
    assert {(left, left, "overrun") for left in range(1, 5)} <= met
    assert not any(left < 5 and continued == left and how == "read" for left, continued, how in met)
    # one to five bytes that end in the message, at every distance from the end on both sides
    assert {(left, continued, "read") for left in range(1, 11) for continued in range(min(left, 5))} <= met


def _codec_values(dialect: str) -> list:
    return [None if v is None else tuple(v) for v in wire_edges.expected(dialect)[1::2]]  # the progress frames


def test_pbjs_reference_row_matches_the_service_codec_on_the_wire_edges():
    """``reference_decode_pbjs`` gives what the protobufjs codec gives on every body, ok == 0 where it raises."""
    bodies = wire_edges.bodies()
    buf, _ = gd.pack(bodies)
    got = gd.materialise(buf, gd.reference_table(bodies, dialect="protobufjs"))
    want = _codec_values("protobufjs")
    diffs = [(bodies[i], got[i], want[i]) for i in range(len(bodies)) if got[i] != want[i]]
    assert not diffs, (len(diffs), diffs[:5])


def test_upb_reference_row_is_the_codec_where_both_decide():
    """``reference_decode`` is looser than the upb codec by design (10-byte tags, no UTF-8 check) and
    calls a group an error where the codec skips it; where it says ok and the codec decodes, the
    values are the codec's, and the codec never decodes a body without a group that it refuses."""
    bodies = wire_edges.bodies()
    buf, _ = gd.pack(bodies)
    table = gd.reference_table(bodies, "upb")
    got = gd.materialise(buf, table)
    want = _codec_values("upb")
    both = [i for i in range(len(bodies)) if got[i] is not None and want[i] is not None]
    diffs = [(bodies[i], got[i], want[i]) for i in both if got[i] != want[i]]
    assert not diffs and len(both) > 2000, (len(both), diffs[:5])
    lost = [bodies[i] for i in range(len(bodies)) if got[i] is None and want[i] is not None
            and not any(b & 7 == 3 for b in bodies[i])]
    assert not lost, lost[:5]
