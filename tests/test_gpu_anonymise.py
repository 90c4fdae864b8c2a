"""``anonymise`` on the GPU (ops/hip/telemetry_anonymise.hip, ops/gpu_anonymise.py) against its
definition, ``anonymise.anonymise_cpu``: every comparison is full ``Anonymised`` equality (the output
bytes, the indices, the frame and event counts, the settings), exact."""
from __future__ import annotations

import functools
import io

import pytest

from beholder_amd import ops
from beholder_amd.anonymise import (FIELDS, Anonymised, Policy, anonymise_cpu, anonymise_file, anonymise_gpu,
                                    pseudonym_of)
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_anonymise as ga, gpu_extract, gpu_fold, hip_lib  # noqa: E402
import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus, varint  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
KEY = bytes(range(32))
ONLY_MEDIA, ONLY_HOST = frozenset({"mediaId"}), frozenset({"host"})
POLICIES = (Policy(KEY, "keep"), Policy(KEY, "drop"))
MINUS = b"\xff\xff\xff\xff\x0f"  # 0xffffffff in 5 bytes: -1 as an int32, 10 bytes when written
GROUP = b"\x2b\x08\x01\x2c"
HOST_SHARE_MAX = 0.10  # of the fold corpus, in either dialect: what the normalise tests hold it to


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
def _want(data: bytes, policy: Policy, dialect: str) -> Anonymised:
    return anonymise_cpu(data, policy, dialect)


def _same(data: bytes, policy: Policy = POLICIES[1], dialect: str = "protobufjs", public: bool = False) -> tuple:
    """Asserts the device result against the definition; returns ``(Anonymised, host_frames)``."""
    want = _want(data, policy, dialect)
    got, host_frames = ga.anonymise(data, policy, DEVICE, dialect)
    assert (got.frames, got.events, got.dialect, got.undecoded, got.fields, got.key_id) == \
        (want.frames, want.events, want.dialect, want.undecoded, want.fields, want.key_id)
    assert got.indices == want.indices
    assert got.data == want.data
    assert got == want
    if public:
        assert anonymise_gpu(data, policy, DEVICE, dialect) == want  # the public call
    return want, host_frames


def _all(data: bytes, fields: frozenset = FIELDS, key: bytes = KEY) -> list:
    """Both dialects and both policies; returns the ``(Anonymised, host_frames)`` pairs."""
    return [_same(data, Policy(key, undecoded, fields), dialect) for dialect in ops.DIALECTS
            for undecoded in ("keep", "drop")]


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for dialect in ops.DIALECTS:
        for policy in POLICIES:
            want = Anonymised(b"", [], 0, 0, dialect, policy.undecoded, FIELDS, policy.key_id)
            assert anonymise_gpu(b"", policy, DEVICE, dialect) == want == anonymise_cpu(b"", policy, dialect)
            assert ga.anonymise(b"", policy, DEVICE, dialect) == (want, 0)
    out = io.BytesIO()
    assert anonymise_file(io.BytesIO(b""), out, POLICIES[0], DEVICE)["frames"] == 0 and out.getvalue() == b""


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame(topic):
    for body in (_event(b"m-1", 3, 40, b"h"), b"", b"\x2e", _int(2, -1) + _int(3, -2 ** 31), b"\x10" + MINUS,
                 _str(1, b"media"), _str(4, b"worker-0")):
        for fields in (FIELDS, ONLY_MEDIA, ONLY_HOST):
            for want, host_frames in _all(frames([(topic, body)]), fields):
                assert want.frames == 1 and host_frames == 0
    want, _ = _same(frames([(topic, _event(b"m-1", 3, 40, b"h"))]), public=True)
    if topic == PROGRESS_ID:
        assert pseudonym_of(KEY, "mediaId", "m-1").encode() in want.data
        assert pseudonym_of(KEY, "host", "h").encode() in want.data
    assert len(want.data) == {STATUS_ID: 5 + 34 + 2, PROGRESS_ID: 5 + 34 + 2 + 2 + 34, 9: 0}[topic]


@pytest.mark.parametrize("count", [64, 65, gpu_extract.SCAN_BLOCK, gpu_extract.SCAN_BLOCK + 1])
def test_one_frame_past_a_wave_and_past_a_block_of_the_scan(count):
    kinds = [(STATUS_ID, _event(b"media-%d", 2)), (PROGRESS_ID, _event(b"m", 2, 50, b"host")), (9, b"other"),
             (PROGRESS_ID, b"\x2e"), (STATUS_ID, b"\x0a\x01m\x10\x03"), (PROGRESS_ID, b"\x18" + MINUS)]
    events = [(t, b.replace(b"%d", b"%d" % k) if t == STATUS_ID else b) for k in range(count)
              for t, b in [kinds[k % len(kinds)]]]
    for want, host_frames in _all(frames(events)):
        assert want.frames == count and host_frames == 0 and 0 < want.events < count
    for want, _ in _all(frames([kinds[1]] * (count - 1) + [kinds[0]])):  # the last frame alone in its wave or block
        assert want.indices == list(range(count)) and want.events == count


@pytest.mark.parametrize("length", [1, 55, 56, 63, 64, 65, 127, 128, 129, 4096, 4097])
def test_string_lengths_at_the_block_edges_of_the_hash_and_at_the_host_limit(length):
    """55 and 56 would be SHA-2's padding edge, 64 and 128 end on a full final block; 4,097 is the
    first length the device leaves to the host."""
    i, h = bytes(0x21 + k % 94 for k in range(length)), bytes(0x7e - k % 94 for k in range(length))
    events = [(PROGRESS_ID, _event(i, 1, 2, h)), (STATUS_ID, _event(i, 3)), (PROGRESS_ID, _str(1, i)),
              (PROGRESS_ID, _str(4, h)), (PROGRESS_ID, _str(1, b"m") + _str(4, h)), (STATUS_ID, _str(4, h))]
    over = length > ga.AN_STRING_MAX
    for fields, host_want in ((FIELDS, 5), (ONLY_MEDIA, 3), (ONLY_HOST, 3)):
        for want, host_frames in _all(frames(events), fields):
            assert want.events == len(events)
            assert host_frames == (host_want if over else 0)
    want, _ = _same(frames(events))
    assert pseudonym_of(KEY, "mediaId", i.decode()).encode() in want.data
    assert pseudonym_of(KEY, "host", h.decode()).encode() in want.data


@pytest.mark.parametrize("length", [64, 65, 129])
def test_an_output_frame_of_exactly_this_length(length):
    """Where a lane's stride of 64 ends: the last lane, the first lane's second byte, and its third.
    One string is a pseudonym (5 + 34 bytes with the header), the other is in clear and sets the
    length: 0x22 or 0x0a, one length byte, the string."""
    clear = b"c" * (length - 5 - 34 - 2)
    for fields, body in ((ONLY_MEDIA, _event(b"media", 0, 0, clear)), (ONLY_HOST, _event(clear, 0, 0, b"worker-0"))):
        for want, host_frames in _all(frames([(PROGRESS_ID, body)] * 3), fields):
            assert len(want.data) == 3 * length and host_frames == 0 and clear in want.data


@pytest.mark.parametrize("key", [bytes(range(9, 9 + n)) for n in (16, 17, 31, 32)], ids=lambda k: str(len(k)))
def test_key_lengths(key):
    data = frames([(PROGRESS_ID, _event(b"media-1", 2, 5, b"worker-0")), (STATUS_ID, _event(b"m" * 70, 2))] * 40)
    for fields in (FIELDS, ONLY_MEDIA, ONLY_HOST):
        for want, _ in _all(data, fields, key):
            assert want.events == 80 and want.key_id == Policy(key).key_id
    assert _want(data, Policy(key), "upb").data != _want(data, Policy(KEY), "upb").data


def test_every_frame_grows_by_the_most():
    grow = frames([(PROGRESS_ID, b"\x0a\x01m\x10" + MINUS + b"\x18" + MINUS + b"\x22\x01h")] * 100)
    for want, _ in _all(grow):
        assert len(want.data) == len(grow) + 100 * ga.AN_GROWTH_MAX and ga.AN_GROWTH_MAX == 72
    status = frames([(STATUS_ID, b"\x0a\x01m\x10" + MINUS)] * 100)
    for want, _ in _all(status):
        assert len(want.data) == len(status) + 100 * 36
    shrink = frames([(PROGRESS_ID, _event(b"m" * 60, 2, 5, b"h" * 50))] * 100)
    for want, _ in _all(shrink):
        assert len(want.data) == 100 * (5 + 34 + 2 + 2 + 34) < len(shrink)


@pytest.mark.parametrize("total", [47, 48, 49, 79, 80, 81])
def test_output_byte_totals_around_a_multiple_of_16(total):
    """5: an empty event; 7: a status number; 39: a pseudonym; 41: both."""
    sizes = {47: (7,) * 6 + (5,), 48: (41, 7), 49: (39, 5, 5), 79: (39,) + (7,) * 5 + (5,), 80: (39, 41),
             81: (39,) + (7,) * 6}[total]
    body = {5: b"\x10\x00", 7: b"\x10\x02\x0a\x00", 39: b"\x10\x00\x0a\x02ab", 41: b"\x10\x03\x0a\x02ab"}
    data = frames([(STATUS_ID if k % 2 else PROGRESS_ID, body[size]) for k, size in enumerate(sizes)])
    for want, _ in _all(data):
        assert len(want.data) == total


def test_drop_over_errors_only_launches_no_emit(monkeypatch):
    call = hip_lib.call

    def no_emit(name, *args):
        assert name != "bh_anonymise_emit", "nothing to emit"
        return call(name, *args)
    monkeypatch.setattr(hip_lib, "call", no_emit)
    data = frames([(PROGRESS_ID, b"\x2e"), (9, b"other"), (STATUS_ID, b"\x0a\x05m")] * 30)
    want, host_frames = _same(data, Policy(KEY, "drop"), "upb")
    assert want == Anonymised(b"", [], 90, 0, "upb", "drop", FIELDS, Policy(KEY).key_id) and host_frames == 0
    with pytest.raises(AssertionError, match="nothing to emit"):
        _same(data, Policy(KEY, "keep"), "upb")


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_host_frames_first_last_and_neighbours(dialect):
    plain = (PROGRESS_ID, _event(b"m", 2, 5, b"h"))
    hosts = [(STATUS_ID, _str(1, "é".encode())), (PROGRESS_ID, _str(1, b"\xff\xfe") + _int(2, 1)),
             (PROGRESS_ID, _event("ü".encode() * 40, -1, 3, b"h")), (PROGRESS_ID, _event(b"m", 2, 5, b"h" * 4097))]
    for layout, count in (([hosts[0], plain, plain], 1), ([plain, plain, hosts[1]], 1),
                          ([plain, hosts[0], hosts[3], plain], 2), ([hosts[2], hosts[1], hosts[0]], 3),
                          ([hosts[1]] + [plain] * 70 + [hosts[2], hosts[3]] + [plain] * 70 + [hosts[1]], 4)):
        for policy in POLICIES:
            want, host_frames = _same(frames(layout), policy, dialect)
            assert host_frames == count
    # a long host in clear stays on the device
    assert _same(frames([hosts[3], plain]), Policy(KEY, fields=ONLY_MEDIA), dialect)[1] == 0


def test_a_group_goes_to_the_host_under_upb():
    body = _str(1, b"m") + GROUP + _int(2, 3)
    data = frames([(STATUS_ID, body), (PROGRESS_ID, body), (PROGRESS_ID, _event())])
    assert _same(data, POLICIES[0], "upb")[1] == 2 and _same(data, POLICIES[1], "upb")[1] == 2
    want, host_frames = _same(data, POLICIES[0], "protobufjs")
    assert host_frames == 0 and want.events == 3


@pytest.mark.parametrize("policy", POLICIES, ids=lambda p: p.undecoded)
@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("name", ["fold_corpus", "wire_edges"])
def test_the_corpora(name, dialect, policy):
    want, host_frames = _same(_corpus(name), policy, dialect, public=policy.undecoded == "keep")
    assert want.frames > 5000 and want.events > 400
    if name == "fold_corpus":
        assert 0 < host_frames <= HOST_SHARE_MAX * want.frames
    for fields in (ONLY_MEDIA, ONLY_HOST):
        assert _same(_corpus(name), Policy(KEY, policy.undecoded, fields), dialect)[1] == host_frames


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_anonymise_file_on_the_device_in_chunks(dialect):
    """Eight chunks or so, each through the device."""
    data = _corpus("fold_corpus")
    assert len(data) > 7 * 30_000
    for policy in POLICIES:
        want = _want(data, policy, dialect)
        for chunk_bytes in (30_000, 1 << 30):
            out, indices = io.BytesIO(), io.StringIO()
            counts = anonymise_file(io.BytesIO(data), out, policy, DEVICE, dialect, chunk_bytes=chunk_bytes,
                                    indices_out=indices)
            assert out.getvalue() == want.data
            assert [int(line) for line in indices.getvalue().split()] == want.indices
            assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                              "in_bytes": len(data), "events": want.events, "undecoded": want.frames - want.events,
                              "host_frames": ga.anonymise(data, policy, DEVICE, dialect)[1]}
            assert counts["host_frames"] > 0


def test_anonymise_is_deterministic():
    data = _corpus("fold_corpus")
    first = anonymise_gpu(data, POLICIES[1], DEVICE)
    assert first == anonymise_gpu(data, POLICIES[1], DEVICE) == _want(data, POLICIES[1], "protobufjs")


def test_the_size_check_raises_before_any_upload(monkeypatch):
    def no_upload(*a, **kw):
        raise AssertionError("the size check comes first")
    data = frames([(PROGRESS_ID, _event())] * 4)
    monkeypatch.setattr(gpu_fold, "upload", no_upload)
    monkeypatch.setattr(hip_lib, "lib", no_upload)
    monkeypatch.setattr(gpu_fold, "index", lambda d: (2 ** 25, None))  # 72 bytes more per frame pass 2^31
    with pytest.raises(ValueError, match="2\\^31") as e:
        ga.anonymise(data, POLICIES[0], DEVICE)
    assert isinstance(e.value, ga.TooLarge)
    with pytest.raises(ValueError, match="--chunk-bytes"):
        anonymise_file(io.BytesIO(data), io.BytesIO(), POLICIES[0], DEVICE)
    ga.check_size(2 ** 31 - 1 - ga.AN_GROWTH_MAX, 1)
    for size, n, extra in ((2 ** 31 - ga.AN_GROWTH_MAX, 1, 0), (2 ** 31 - 1 - ga.AN_GROWTH_MAX, 1, 1), (5, 2 ** 25, 0)):
        with pytest.raises(ga.TooLarge):
            ga.check_size(size, n, extra)


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch

    from beholder_amd import normalise
    data = frames([(PROGRESS_ID, _event())] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    tables = ga.allocate(buf, offs_dev, n)
    policy = POLICIES[0]

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        ga.allocate(buf, offs_dev.to(torch.int64), n)  # wrong dtype
    with pytest.raises(ValueError):
        ga.allocate(buf.cpu(), offs_dev.cpu(), n)  # host tensors
    with pytest.raises(ValueError):
        ga.allocate(buf, offs_dev, n + 1)  # offs is not n + 1
    with pytest.raises(ValueError):
        ga.allocate(buf[:0], offs_dev[:1], 0)  # n >= 1
    with pytest.raises(ValueError):
        ga.classify(tables, policy, dialect="proto2")
    for no_policy in ("keep", normalise.Policy()):
        with pytest.raises(TypeError):
            ga.classify(tables, no_policy)
        with pytest.raises(TypeError):
            ga.anonymise(data, no_policy, DEVICE)
    for name, value in (("undecoded", "first"), ("fields", frozenset()), ("fields", frozenset({"status"})),
                        ("key", KEY[:15]), ("key", KEY + b"!"), ("key", KEY.hex())):
        bad = Policy(KEY)
        object.__setattr__(bad, name, value)  # a policy that got past its own check
        for call in (lambda: ga.classify(tables, bad), lambda: ga.anonymise(data, bad, DEVICE)):
            with pytest.raises(ValueError):
                call()
    for kept, kept_bytes in ((-1, 5), (n + 1, 50), (1, 0), (0, 5), (1, 2 ** 31)):
        with pytest.raises(ValueError):
            ga.emit(tables, kept, kept_bytes)
    with pytest.raises(ValueError):
        anonymise_gpu(data, policy, DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        anonymise_gpu(data, policy, "cpu")
    with pytest.raises(ValueError):
        anonymise_gpu(data[:-1], policy, DEVICE)  # broken framing never reaches the device
    with pytest.raises(ValueError):
        anonymise_file(io.BytesIO(data), io.BytesIO(), policy, DEVICE, dialect="proto2")
