"""``export`` on the GPU (ops/hip/telemetry_export.hip, ops/gpu_export.py) against its definition,
``export.export_cpu``: every comparison is full ``Exported`` equality (the rows' bytes, the indices,
the frame and event counts, the base), exact."""
from __future__ import annotations

import functools
import io

import pytest

from beholder_amd import ops
from beholder_amd.export import Exported, Policy, export_cpu, export_file, export_gpu
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_export as gx, gpu_extract, gpu_fold, hip_lib  # noqa: E402
import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus, varint  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
POLICIES = (Policy("keep"), Policy("drop"))
GROUP = b"\x2b\x08\x01\x2c"
ERROR = b"\x2e"  # field 5 with wire type 6: no event in either dialect
HOST_SHARE_MAX = 0.10  # of the fold corpus, in either dialect
LENGTHS = (63, 64, 65, 128, 129)


def _int(field: int, value: int) -> bytes:
    return varint(field << 3) + varint(value & 0xFFFFFFFFFFFFFFFF)


def _str(field: int, value: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(value)) + value


def _event(mid: bytes = b"m", status: int = 0, progress: int = 0, host: bytes = b"") -> bytes:
    """A body that is not canonical: host first, every field explicit, an unknown field last."""
    return _str(4, host) + _int(3, progress) + _int(2, status) + _str(1, mid) + b"\x38\x01"


@functools.lru_cache(maxsize=None)
def _corpus(name: str) -> bytes:
    return fold_corpus() if name == "fold_corpus" else wire_edges.stream(6000)


@functools.lru_cache(maxsize=None)
def _want(data: bytes, policy: Policy, dialect: str, base: int) -> Exported:
    return export_cpu(data, policy, dialect, base)


def _same(data: bytes, policy: Policy = Policy(), dialect: str = "protobufjs", base: int = 0, public: bool = False) -> tuple:
    """Asserts the device result against the definition; returns ``(Exported, host_frames)``."""
    want = _want(data, policy, dialect, base)
    got, host_frames = gx.export(data, policy, DEVICE, dialect, base)
    assert (got.frames, got.events, got.base, got.dialect, got.undecoded) == \
        (want.frames, want.events, want.base, want.dialect, want.undecoded)
    assert got.indices == want.indices
    if got.data != want.data:  # name the first row that differs, not a megabyte of text
        rows = list(zip(got.data.split(b"\n"), want.data.split(b"\n")))
        k = next((k for k, (g, w) in enumerate(rows) if g != w), len(rows))
        assert rows[k:k + 1] == [], (k, len(got.data), len(want.data))
    assert got == want
    if public:
        assert export_gpu(data, policy, DEVICE, dialect, base) == want  # the public call
    return want, host_frames


def _all(data: bytes, base: int = 0) -> list:
    """Both dialects and both policies; returns the ``(Exported, host_frames)`` pairs."""
    return [_same(data, policy, dialect, base) for dialect in ops.DIALECTS for policy in POLICIES]


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for dialect in ops.DIALECTS:
        for policy in POLICIES:
            want = Exported(b"", [], 0, 0, 3, dialect, policy.undecoded)
            assert export_gpu(b"", policy, DEVICE, dialect, 3) == want == export_cpu(b"", policy, dialect, 3)
            assert gx.export(b"", policy, DEVICE, dialect, 3) == (want, 0)
    out = io.BytesIO()
    assert export_file(io.BytesIO(b""), out, Policy(), DEVICE)["frames"] == 0 and out.getvalue() == b""


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (b"", ERROR, _event(b"m-1", 3, 40, b"h"), _int(2, -1) + _int(3, -2 ** 31)):
        for want, host_frames in _all(frames([(topic, body)])):
            assert want.frames == 1 and host_frames == 0
    want, _ = _same(frames([(topic, _event(b"m-1", 3, 40, b"h"))]), public=True)
    assert want.events == (topic != 9) and want.data.endswith(b"}\n")


@pytest.mark.parametrize("count", [64, 65, gpu_extract.SCAN_BLOCK, gpu_extract.SCAN_BLOCK + 1])
def test_one_frame_past_a_wave_and_past_a_block_of_the_scan(count):
    kinds = [(STATUS_ID, _event(b"media-%d", 2)), (PROGRESS_ID, _event(b"m\"", 2, 50, b"ho\x01st")), (9, b"other"),
             (PROGRESS_ID, ERROR), (STATUS_ID, b"\x0a\x01m\x10\x03"), (PROGRESS_ID, _int(3, -7))]
    events = [(t, b.replace(b"%d", b"%d" % k) if t == STATUS_ID else b) for k in range(count)
              for t, b in [kinds[k % len(kinds)]]]
    for want, host_frames in _all(frames(events)):
        assert want.frames == count and host_frames == 0 and 0 < want.events < count
    for want, _ in _all(frames([kinds[2]] * (count - 1) + [kinds[1]])):  # the last frame alone in its wave or block
        assert want.events == 1 and want.indices[-1] == count - 1


def _row_length(event: tuple, base: int = 0) -> int:
    return len(export_cpu(frames([event]), Policy(), "upb", base).data)


@pytest.mark.parametrize("length", LENGTHS)
def test_a_row_of_exactly_this_length(length):
    """Where a lane's stride of 64 ends: the last lane, the first lane's second byte, and its third. A
    decoded row has 87 bytes around its id, so the short ones are base64 rows: four bytes of text per
    three of the body, and the topic's and the index's digits make up the rest."""
    exact = [(event, base) for base in (0, 10, 100) for topic in (9, 10, 100) for size in range(0, 99, 3)
             for event in [(topic, b"\xfb" * size)] if _row_length(event, base) == length]
    fixed = _row_length((STATUS_ID, b""))
    assert fixed == 87
    if length > fixed:
        exact += [((STATUS_ID, _event(b"i" * (length - fixed))), 0),
                  ((PROGRESS_ID, _event(b"i" * (length - _row_length((PROGRESS_ID, _event(b"", 1, 2, b"h")))), 1, 2, b"h")), 0)]
    assert len(exact) >= 2
    for event, base in exact:
        for want, host_frames in _all(frames([event] * 3), base):
            assert host_frames == 0
        assert len(_want(frames([event] * 3), Policy(), "upb", base).data) == 3 * length


@pytest.mark.parametrize("length", LENGTHS)
def test_escapes_at_and_across_the_pieces_of_64(length):
    """A quote at 0, 63, 64 and last; a six-byte escape at 62, 63 and 64, whose bytes cross the piece's
    end; all six-byte and all two-byte. In the id, in the host, and in both."""
    strings = [b"\x01" * length, b"\\" * length, b"\n\x1f\"a" * (length // 4) + b"z" * (length % 4)]
    for at in sorted({0, 63, 64, length - 1} & set(range(length))):
        strings.append(b"a" * at + b'"' + b"b" * (length - at - 1))
    for at in sorted({62, 63, 64} & set(range(length))):
        strings.append(b"a" * at + b"\x01" + b"b" * (length - at - 1))
    events = []
    for s in strings:
        events += [(STATUS_ID, _event(s, 4)), (PROGRESS_ID, _event(b"plain", 1, 2, s)), (PROGRESS_ID, _event(s, 1, 2, s[::-1])),
                   (PROGRESS_ID, _event(s, 1, 2, b"plain"))]
    for want, host_frames in _all(frames(events)):
        assert want.events == len(events) and host_frames == 0
    assert b"\\u0001" * length in _want(frames(events), Policy(), "upb", 0).data


@pytest.mark.parametrize("size", [0, 1, 2, 3, 4, 62, 63, 64, 65])
def test_base64_bodies(size):
    """Bodies of exactly this size on another topic, and as decode errors on the two topics."""
    events = [(9, bytes(range(size))), (0, b"\xff" * size), (255, b"\xfb\xef\xbe" * size)]
    if size:  # an empty body is an event
        error = ERROR + bytes((200 + k) % 256 for k in range(size - 1))
        events += [(STATUS_ID, error), (PROGRESS_ID, error)]
    for want, host_frames in _all(frames(events * 3)):
        assert want.events == 0 and host_frames == 0
        assert len(want.indices) == (len(events) * 3 if want.undecoded == "keep" else 0)


@pytest.mark.parametrize("base", [0, 9, 10, 99, 10 ** 9 - 1, 2 ** 31, 2 ** 53])
def test_the_index_takes_a_digit_more_inside_the_chunk(base):
    events = [(STATUS_ID, _event(b"m", 2)), (9, b"abc"), (PROGRESS_ID, _event(b"a\tb", 3, 4, b"h"))] * 4
    for want, _ in _all(frames(events), base):
        assert want.base == base and want.frames == 12
    assert _want(frames(events), Policy(), "upb", base).indices == list(range(base, base + 12))


def test_status_and_progress_values():
    values = (0, 5, 6, -1, -2 ** 31, 2 ** 31 - 1, 10, 99, 100)
    events = [(PROGRESS_ID, _int(2, s) + _int(3, p)) for s in values for p in values]
    events += [(STATUS_ID, _int(2, s)) for s in values]
    for want, host_frames in _all(frames(events)):
        assert want.events == len(events) and host_frames == 0
    data = _want(frames(events), Policy(), "upb", 0).data
    assert b'"status":-2147483648,"progress":2147483647,' in data and b'"name":"ERRORED"' in data and b'"name":null' in data


def test_drop_over_errors_only_launches_no_emit(monkeypatch):
    call = hip_lib.call

    def no_emit(name, *args):
        assert name != "bh_export_emit", "nothing to emit"
        return call(name, *args)
    monkeypatch.setattr(hip_lib, "call", no_emit)
    data = frames([(PROGRESS_ID, ERROR), (9, b"other"), (STATUS_ID, b"\x0a\x05m")] * 30)
    want, host_frames = _same(data, Policy("drop"), "upb")
    assert want == Exported(b"", [], 90, 0, 0, "upb", "drop") and host_frames == 0
    with pytest.raises(AssertionError, match="nothing to emit"):
        _same(data, Policy("keep"), "upb")


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_host_frames_first_last_and_neighbours(dialect):
    plain = (PROGRESS_ID, _event(b"m", 2, 5, b"h"))
    hosts = [(STATUS_ID, _str(1, "é".encode())), (PROGRESS_ID, _str(1, b"\xff\xfe") + _int(2, 1)),
             (PROGRESS_ID, _event("ü".encode() * 40, -1, 3, b"h\"\x01"))]
    for layout, count in (([hosts[0], plain, plain], 1), ([plain, plain, hosts[1]], 1),
                          ([plain, hosts[0], hosts[1], plain], 2), ([hosts[2], hosts[1], hosts[0]], 3),
                          ([hosts[1]] + [plain] * 70 + [hosts[2], hosts[0]] + [plain] * 70 + [hosts[1]], 4)):
        for policy in POLICIES:
            want, host_frames = _same(frames(layout), policy, dialect, base=98)
            assert host_frames == count
    # invalid UTF-8 is U+FFFD twice under protobufjs and no event under upb
    want, _ = _same(frames([hosts[1]]), Policy(), dialect)
    assert want.events == (dialect == "protobufjs") and ("��".encode() in want.data) == bool(want.events)


def test_a_non_ascii_host_goes_to_the_host_in_either_dialect():
    data = frames([(PROGRESS_ID, _event(b"m", 2, 5, "hôte".encode())), (PROGRESS_ID, _event(b"m", 2, 5, b"h\xff")),
                   (STATUS_ID, _event(b"m", 2, 5, b"h\xff"))])  # field 4 of a status message is an unknown field
    for dialect in ops.DIALECTS:
        for policy in POLICIES:
            want, host_frames = _same(data, policy, dialect)
            assert host_frames == 2 and want.events == (3 if dialect == "protobufjs" else 2)


def test_a_group_goes_to_the_host_under_upb():
    body = _str(1, b"m") + GROUP + _int(2, 3)
    data = frames([(STATUS_ID, body), (PROGRESS_ID, body), (PROGRESS_ID, _event())])
    assert _same(data, Policy(), "upb")[1] == 2 and _same(data, Policy("drop"), "upb")[1] == 2
    want, host_frames = _same(data, Policy(), "protobufjs")
    assert host_frames == 0 and want.events == 3


@pytest.mark.parametrize("policy", POLICIES, ids=lambda p: p.undecoded)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", ["fold_corpus", "wire_edges"])
def test_the_corpora(name, dialect, policy):
    want, host_frames = _same(_corpus(name), policy, dialect, public=policy.undecoded == "keep")
    assert want.frames > 5000 and want.events > 400
    if name == "fold_corpus":
        assert host_frames <= HOST_SHARE_MAX * want.frames
        if dialect == "protobufjs":
            assert host_frames > 0


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_export_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device from the index its first frame has."""
    data = _corpus("fold_corpus")
    assert len(data) > 7 * 30_000
    for policy in POLICIES:
        want = _want(data, policy, dialect, 0)
        for chunk_bytes in (30_000, 1 << 30):
            out, indices = io.BytesIO(), io.StringIO()
            counts = export_file(io.BytesIO(data), out, policy, DEVICE, dialect, chunk_bytes=chunk_bytes,
                                 indices_out=indices)
            assert out.getvalue() == want.data
            assert [int(line) for line in indices.getvalue().split()] == want.indices
            assert counts == {"frames": want.frames, "rows": len(want.indices), "out_bytes": len(want.data),
                              "in_bytes": len(data), "events": want.events, "undecoded": want.frames - want.events,
                              "host_frames": gx.export(data, policy, DEVICE, dialect)[1]}


def test_export_is_deterministic():
    data = _corpus("fold_corpus")
    first = export_gpu(data, Policy(), DEVICE)
    assert first == export_gpu(data, Policy(), DEVICE) == _want(data, Policy(), "protobufjs", 0)


def test_the_size_check_raises_before_the_scan_and_any_emit(monkeypatch):
    call = hip_lib.call

    def classify_only(name, *args):
        assert name == "bh_export_classify", "the size check comes first"
        return call(name, *args)
    data = frames([(PROGRESS_ID, _event())] * 4)
    monkeypatch.setattr(hip_lib, "call", classify_only)
    for size in (2 ** 31, 2 ** 33):
        monkeypatch.setattr(gx, "keep_len_sum", lambda t, size=size: size)
        with pytest.raises(ValueError, match="2\\^31") as e:
            gx.export(data, Policy(), DEVICE)
        assert isinstance(e.value, gx.TooLarge)
        with pytest.raises(ValueError, match="--chunk-bytes"):
            export_file(io.BytesIO(data), io.BytesIO(), Policy(), DEVICE)
    monkeypatch.setattr(gx, "keep_len_sum", lambda t: 2 ** 31 - 1)  # fits: the scan is next
    with pytest.raises(AssertionError, match="the size check comes first"):
        gx.export(data, Policy(), DEVICE)


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = frames([(PROGRESS_ID, _event())] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gx.allocate(buf, offs_dev, n)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gx.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gx.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gx.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gx.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    for base in (-1, 2 ** 63, 1.5):
        with pytest.raises(ValueError):
            gx.allocate(buf, offs_dev, n, base)
        with pytest.raises(ValueError):
            export_gpu(data, Policy(), DEVICE, base=base)
    with pytest.raises(ValueError):
        gx.classify(tables, Policy(), dialect="proto2")
    with pytest.raises(TypeError):
        gx.classify(tables, "keep")
    bad = Policy()
    object.__setattr__(bad, "undecoded", "first")  # a policy that got past its own check
    for call in (lambda: gx.classify(tables, bad), lambda: gx.export(data, bad, DEVICE)):
        with pytest.raises(ValueError):
            call()
    for kept, kept_bytes in ((-1, 5), (n + 1, 50), (1, 0), (0, 5), (1, 2 ** 31)):
        with pytest.raises(ValueError):
            gx.emit(tables, kept, kept_bytes)
    with pytest.raises(TypeError):
        gx.export(data, "keep", DEVICE)
    with pytest.raises(ValueError):
        export_gpu(data, Policy(), DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        export_gpu(data, Policy(), "cpu")
    with pytest.raises(ValueError):
        export_gpu(data[:-1], Policy(), DEVICE)  # broken framing never reaches the device
    with pytest.raises(ValueError):
        export_file(io.BytesIO(data), io.BytesIO(), Policy(), DEVICE, dialect="proto2")
