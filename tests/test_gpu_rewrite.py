"""What the rewriting commands share on the host (ops/gpu_rewrite.py), as far as it runs without a
GPU: the splice of the host's parts into the stream that came back, against plain concatenation, and
the check in front of every emit, which must refuse what cannot be the scan's totals before anything
is allocated. The commands' own GPU tests (test_gpu_normalise.py, test_gpu_anonymise.py,
test_gpu_export.py, test_gpu_import.py) hold the rest to the CPU definitions."""
from __future__ import annotations

import sys
import types

import pytest

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_rewrite  # noqa: E402

FILL = 0xEE  # what the device left in a host part's span: anything


def _spliced(pieces):
    """``pieces`` are ``(bytes, from the host)`` in stream order: the stream as the device leaves it,
    spliced, and the stream by plain concatenation."""
    want = b"".join(piece for piece, _ in pieces)
    stream = np.frombuffer(b"".join(bytes([FILL]) * len(piece) if host else piece for piece, host in pieces),
                           dtype=np.uint8).copy()
    at, parts, start = [], [], 0
    for piece, host in pieces:
        if host:
            at.append(start)
            parts.append(piece)
        start += len(piece)
    gpu_rewrite.splice(stream, at, parts)
    return stream.tobytes(), want


@pytest.mark.parametrize("pieces", [
    [(b"host", True), (b"device bytes", False)],                          # at the stream's first byte
    [(b"device", False), (b"h", True), (b"more", False)],                 # in the middle
    [(b"device bytes", False), (b"host\n", True)],                        # at its last byte
    [(b"d", False), (b"one", True), (b"two!", True), (b"d", False)],      # adjacent
    [(b"a", True), (b"bc", True), (b"def", True)],                        # nothing but host parts
    [(b"x", True), (b"d" * 70, False), (b"y", True), (b"z", True), (b"d", False), (b"w" * 200, True)],
    [(b"only the device's", False)],                                      # none at all
    [],                                                                   # an empty stream
], ids=["first", "middle", "last", "adjacent", "all", "mixed", "none", "empty"])
def test_the_splice_is_plain_concatenation(pieces):
    got, want = _spliced(pieces)
    assert got == want


def test_the_splice_writes_nothing_outside_the_parts():
    stream = np.arange(16, dtype=np.uint8)
    gpu_rewrite.splice(stream, [3, 9], [b"\xff\xfe", b"\xfd"])
    assert stream.tolist() == [0, 1, 2, 0xFF, 0xFE, 5, 6, 7, 8, 0xFD, 10, 11, 12, 13, 14, 15]


class _Buf:
    """A stand-in for the device's input: its size, and a device that nobody may ask for before the
    check has passed."""

    def __init__(self, size: int):
        self.size = size

    def numel(self) -> int:
        return self.size

    @property
    def device(self):
        raise AssertionError("allocates")


def _tables(n: int, size: int) -> gpu_rewrite.Tables:
    return gpu_rewrite.Tables(n, _Buf(size), None, None, None, None, None, None)


def test_the_emit_front_refuses_what_is_not_the_scans_totals_before_any_allocation(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", types.SimpleNamespace(empty=None, uint8=None))  # nothing to allocate with
    n, size = 2, 100
    t = _tables(n, size)
    for kept, kept_bytes in ((-1, 5), (n + 1, 50), (n + 1, 20), (1, 0), (0, 5), (1, 2 ** 31), (1, -1)):
        with pytest.raises(ValueError, match="the scan's totals"):
            gpu_rewrite.emit_out(t, kept, kept_bytes)
    # the import's bound is its text's size: a frame is shorter than its row
    for kept, kept_bytes in ((1, size), (1, size + 1), (1, 2 ** 31), (-1, 5), (n + 1, 20), (1, 0), (0, 5)):
        with pytest.raises(ValueError, match="the scan's totals"):
            gpu_rewrite.emit_out(t, kept, kept_bytes, size)
    # what can be the scan's totals gets as far as the allocation
    whole = gpu_rewrite.LIMIT
    for kept, kept_bytes, limit in ((0, 0, whole), (1, 1, whole), (n, 2 ** 31 - 1, whole), (n, size - 1, size),
                                    (0, 0, size)):
        with pytest.raises(AssertionError, match="allocates"):
            gpu_rewrite.emit_out(t, kept, kept_bytes, limit)


def test_no_host_parts_scatter_nothing():
    frames = gpu_rewrite.scatter(None, [], [])  # touches no table
    assert frames.dtype == np.int64 and frames.size == 0
    none = gpu_rewrite.NO_HOST_PARTS
    assert (none.count, len(none.parts), none.events, none.rewritten, none.carried, list(none.skipped)) == \
        (0, 0, 0, 0, 0, [])
    assert none.frames.dtype == np.int64 and none.frames.size == 0
