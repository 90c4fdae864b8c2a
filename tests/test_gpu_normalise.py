"""``normalise`` on the GPU (ops/hip/telemetry_normalise.hip, ops/gpu_normalise.py) against its
definition, ``normalise.normalise_cpu``: every comparison is full ``Normalised`` equality (the output
bytes, the indices, the frame, event and rewritten counts), exact."""
from __future__ import annotations

import functools
import io

import pytest

from beholder_amd import ops
from beholder_amd.normalise import Normalised, Policy, normalise_cpu, normalise_file, normalise_gpu
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_extract, gpu_fold, gpu_normalise as gn, hip_lib  # noqa: E402
import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus, varint  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
POLICIES = (Policy("keep"), Policy("drop"))
MINUS = b"\xff\xff\xff\xff\x0f"  # 0xffffffff in 5 bytes: -1 as an int32, 10 bytes when written
GROUP = b"\x2b\x08\x01\x2c"
HOST_SHARE_MAX = 0.10  # of the fold corpus, in either dialect


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
def _want(data: bytes, policy: Policy, dialect: str) -> Normalised:
    return normalise_cpu(data, policy, dialect)


def _same(data: bytes, policy: Policy = Policy(), dialect: str = "protobufjs", public: bool = False) -> tuple:
    """Asserts the device result against the definition; returns ``(Normalised, host_frames)``."""
    want = _want(data, policy, dialect)
    got, host_frames = gn.normalise(data, policy, DEVICE, dialect)
    assert (got.frames, got.events, got.rewritten, got.dialect, got.undecoded) == \
        (want.frames, want.events, want.rewritten, want.dialect, want.undecoded)
    assert got.indices == want.indices
    assert got.data == want.data
    assert got == want
    if public:
        assert normalise_gpu(data, policy, DEVICE, dialect) == want  # the public call
    return want, host_frames


def _all(data: bytes) -> list:
    """Both dialects and both policies; returns the ``(Normalised, host_frames)`` pairs."""
    return [_same(data, policy, dialect) for dialect in ops.DIALECTS for policy in POLICIES]


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for dialect in ops.DIALECTS:
        for policy in POLICIES:
            want = Normalised(b"", [], 0, 0, 0, dialect, policy.undecoded)
            assert normalise_gpu(b"", policy, DEVICE, dialect) == want == normalise_cpu(b"", policy, dialect)
            assert gn.normalise(b"", policy, DEVICE, dialect) == (want, 0)
    out = io.BytesIO()
    assert normalise_file(io.BytesIO(b""), out, Policy(), DEVICE)["frames"] == 0 and out.getvalue() == b""


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (_event(b"m-1", 3, 40, b"h"), b"", b"\x2e", _int(2, -1) + _int(3, -2 ** 31), b"\x10" + MINUS):
        for want, host_frames in _all(frames([(topic, body)])):
            assert want.frames == 1 and host_frames == 0
    want, _ = _same(frames([(topic, _event(b"m-1", 3, 40, b"h"))]), public=True)
    assert want.rewritten == (topic != 9)


@pytest.mark.parametrize("count", [64, 65, gpu_extract.SCAN_BLOCK, gpu_extract.SCAN_BLOCK + 1])
def test_one_frame_past_a_wave_and_past_a_block_of_the_scan(count):
    kinds = [(STATUS_ID, _event(b"media-%d", 2)), (PROGRESS_ID, _event(b"m", 2, 50, b"host")), (9, b"other"),
             (PROGRESS_ID, b"\x2e"), (STATUS_ID, b"\x0a\x01m\x10\x03"), (PROGRESS_ID, b"\x18" + MINUS)]
    events = [(t, b.replace(b"%d", b"%d" % k) if t == STATUS_ID else b) for k in range(count)
              for t, b in [kinds[k % len(kinds)]]]
    for want, host_frames in _all(frames(events)):
        assert want.frames == count and host_frames == 0 and 0 < want.rewritten < want.events
    for want, _ in _all(frames([kinds[1]] * (count - 1) + [kinds[0]])):  # the last frame alone in its wave or block
        assert want.indices == list(range(count)) and want.rewritten == count


@pytest.mark.parametrize("length", [5, 64, 65, 129])
def test_a_canonical_frame_of_exactly_this_length(length):
    """Where a lane's stride of 64 ends: the last lane, the first lane's second byte, and its third."""
    body = b"" if length == 5 else _event(b"i" * (length - 7))  # 5 | 0x0a | one length byte | the id
    for topic in (STATUS_ID, PROGRESS_ID):
        for want, host_frames in _all(frames([(topic, body)] * 3)):
            assert len(want.data) == 3 * length and host_frames == 0 and want.rewritten == (0 if length == 5 else 3)


@pytest.mark.parametrize("length", [127, 128, 16383, 16384])
def test_string_lengths_where_the_length_varint_steps(length):
    events = [(PROGRESS_ID, _event(b"i" * length, 1, 2, b"h" * length)), (STATUS_ID, _event(b"i" * length)),
              (PROGRESS_ID, _str(1, b"i" * length)), (PROGRESS_ID, _str(4, b"h" * length)),  # canonical already
              (PROGRESS_ID, b"\x0a" + varint(length) + b"i" * (length - 1))]  # clamped under protobufjs
    for want, host_frames in _all(frames(events)):
        assert host_frames == 0
        assert want.rewritten == (3 if want.dialect == "protobufjs" else 2)


def test_negative_status_and_progress():
    values = (-1, -2 ** 31, -2 ** 31 + 1, 2 ** 31 - 1, 1, 127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 28)
    events = [(PROGRESS_ID, _int(2, s) + _int(3, p)) for s in values for p in values]
    events += [(STATUS_ID, _int(2, s)) for s in values]
    for want, host_frames in _all(frames(events)):
        assert want.events == len(events) and want.rewritten == 0 and host_frames == 0  # 10 bytes already
    events = [(t, b"\x10" + MINUS + b"\x18\x80\x80\x80\x80\x08") for t in (STATUS_ID, PROGRESS_ID)]
    for want, _ in _all(frames(events * 40)):
        assert want.rewritten == 80


def test_every_frame_grows_and_every_frame_shrinks():
    grow = frames([(PROGRESS_ID, b"\x10" + MINUS + b"\x18" + MINUS), (STATUS_ID, b"\x0a\x01m\x10" + MINUS)] * 100)
    for want, _ in _all(grow):
        assert len(want.data) == len(grow) + 100 * (gn.NM_GROWTH_MAX + 5) and want.rewritten == 200
    shrink = frames([(PROGRESS_ID, _event(b"m", 2, 5, b"h")), (STATUS_ID, _event(b"m", 0, 7, b"host"))] * 100)
    for want, _ in _all(shrink):
        assert len(want.data) < len(shrink) - 200 * 2 and want.rewritten == 200
    same = frames([(PROGRESS_ID, b"\x18\x05\x10\x02\x0a\x01m"), (PROGRESS_ID, b"\x0a\x01m\x10\x02\x18\x05")] * 50)
    for want, _ in _all(same):  # the same length, other bytes: the ballot decides
        assert len(want.data) == len(same) and want.rewritten == 50


@pytest.mark.parametrize("total", [15, 16, 17, 31, 32, 33])
def test_output_byte_totals_around_a_multiple_of_16(total):
    sizes = {15: (5, 5, 5), 16: (7, 9), 17: (5, 5, 7), 31: (7, 7, 7, 5, 5), 32: (9, 9, 7, 7), 33: (9, 9, 5, 5, 5)}[total]
    body = {5: b"\x10\x00", 7: b"\x10\x02\x0a\x00", 9: b"\x10\x00\x0a\x02ab"}
    data = frames([(STATUS_ID if k % 2 else PROGRESS_ID, body[size]) for k, size in enumerate(sizes)])
    for want, _ in _all(data):
        assert len(want.data) == total


def test_drop_over_errors_only_launches_no_emit(monkeypatch):
    call = hip_lib.call

    def no_emit(name, *args):
        assert name != "bh_normalise_emit", "nothing to emit"
        return call(name, *args)
    monkeypatch.setattr(hip_lib, "call", no_emit)
    data = frames([(PROGRESS_ID, b"\x2e"), (9, b"other"), (STATUS_ID, b"\x0a\x05m")] * 30)
    want, host_frames = _same(data, Policy("drop"), "upb")
    assert want == Normalised(b"", [], 90, 0, 0, "upb", "drop") and host_frames == 0
    with pytest.raises(AssertionError, match="nothing to emit"):
        _same(data, Policy("keep"), "upb")


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_host_frames_first_last_and_neighbours(dialect):
    plain = (PROGRESS_ID, _event(b"m", 2, 5, b"h"))
    hosts = [(STATUS_ID, _str(1, "é".encode())), (PROGRESS_ID, _str(1, b"\xff\xfe") + _int(2, 1)),
             (PROGRESS_ID, _event("ü".encode() * 40, -1, 3, b"h"))]
    for layout, count in (([hosts[0], plain, plain], 1), ([plain, plain, hosts[1]], 1),
                          ([plain, hosts[0], hosts[1], plain], 2), ([hosts[2], hosts[1], hosts[0]], 3),
                          ([hosts[1]] + [plain] * 70 + [hosts[2], hosts[0]] + [plain] * 70 + [hosts[1]], 4)):
        for policy in POLICIES:
            want, host_frames = _same(frames(layout), policy, dialect)
            assert host_frames == count
    # invalid UTF-8 grows under protobufjs (U+FFFD, three bytes each) and is no event under upb
    want, _ = _same(frames([hosts[1]]), Policy(), dialect)
    assert len(want.data) - len(frames([hosts[1]])) == (4 if dialect == "protobufjs" else 0)


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
    assert host_frames == 0 and want.rewritten == 3


@pytest.mark.parametrize("policy", POLICIES, ids=lambda p: p.undecoded)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", ["fold_corpus", "wire_edges"])
def test_the_corpora(name, dialect, policy):
    want, host_frames = _same(_corpus(name), policy, dialect, public=policy.undecoded == "keep")
    assert want.frames > 5000 and want.events > 400 and 0 < want.rewritten < want.events
    if name == "fold_corpus":
        assert 0 < host_frames <= HOST_SHARE_MAX * want.frames


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_normalise_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device."""
    data = _corpus("fold_corpus")
    assert len(data) > 7 * 30_000
    for policy in POLICIES:
        want = _want(data, policy, dialect)
        for chunk_bytes in (30_000, 1 << 30):
            out, indices = io.BytesIO(), io.StringIO()
            counts = normalise_file(io.BytesIO(data), out, policy, DEVICE, dialect, chunk_bytes=chunk_bytes,
                                    indices_out=indices)
            assert out.getvalue() == want.data
            assert [int(line) for line in indices.getvalue().split()] == want.indices
            assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                              "in_bytes": len(data), "events": want.events, "rewritten": want.rewritten,
                              "undecoded": want.frames - want.events,
                              "host_frames": gn.normalise(data, policy, DEVICE, dialect)[1]}
            assert counts["host_frames"] > 0


def test_normalise_is_deterministic():
    data = _corpus("fold_corpus")
    first = normalise_gpu(data, Policy(), DEVICE)
    assert first == normalise_gpu(data, Policy(), DEVICE) == _want(data, Policy(), "protobufjs")


def test_the_size_check_raises_before_any_upload(monkeypatch):
    def no_upload(*a, **kw):
        raise AssertionError("the size check comes first")
    data = frames([(PROGRESS_ID, _event())] * 4)
    monkeypatch.setattr(gpu_fold, "upload", no_upload)
    monkeypatch.setattr(hip_lib, "lib", no_upload)
    monkeypatch.setattr(gpu_fold, "index", lambda d: (2 ** 28, None))  # 10 bytes more per frame pass 2^31
    with pytest.raises(ValueError, match="2\\^31") as e:
        gn.normalise(data, Policy(), DEVICE)
    assert isinstance(e.value, gn.TooLarge)
    with pytest.raises(ValueError, match="--chunk-bytes"):
        normalise_file(io.BytesIO(data), io.BytesIO(), Policy(), DEVICE)
    gn.check_size(2 ** 31 - 1 - gn.NM_GROWTH_MAX, 1)
    for size, n, extra in ((2 ** 31 - gn.NM_GROWTH_MAX, 1, 0), (2 ** 31 - 1 - gn.NM_GROWTH_MAX, 1, 1), (5, 2 ** 28, 0)):
        with pytest.raises(gn.TooLarge):
            gn.check_size(size, n, extra)


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = frames([(PROGRESS_ID, _event())] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = gn.allocate(buf, offs_dev, n)

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gn.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        gn.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        gn.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        gn.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        gn.classify(tables, Policy(), dialect="proto2")
    with pytest.raises(TypeError):
        gn.classify(tables, "keep")
    bad = Policy()
    object.__setattr__(bad, "undecoded", "first")  # a policy that got past its own check
    for call in (lambda: gn.classify(tables, bad), lambda: gn.normalise(data, bad, DEVICE)):
        with pytest.raises(ValueError):
            call()
    for kept, kept_bytes in ((-1, 5), (n + 1, 50), (1, 0), (0, 5), (1, 2 ** 31)):
        with pytest.raises(ValueError):
            gn.emit(tables, kept, kept_bytes)
    with pytest.raises(TypeError):
        gn.normalise(data, "keep", DEVICE)
    with pytest.raises(ValueError):
        normalise_gpu(data, Policy(), DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        normalise_gpu(data, Policy(), "cpu")
    with pytest.raises(ValueError):
        normalise_gpu(data[:-1], Policy(), DEVICE)  # broken framing never reaches the device
    with pytest.raises(ValueError):
        normalise_file(io.BytesIO(data), io.BytesIO(), Policy(), DEVICE, dialect="proto2")
