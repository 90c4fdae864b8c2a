"""``extract`` on the GPU (ops/hip/telemetry_select.hip, ops/gpu_extract.py) against its definition,
``extract.extract_cpu``: every comparison is full ``Extract`` equality (the output bytes, the kept
indices and the frame count), exact. Both gather shapes are held to it."""
from __future__ import annotations

import functools
import random

import pytest

from beholder_amd import ops
from beholder_amd.bench.generator import Workload
from beholder_amd.extract import Extract, Selector, extract_cpu, extract_gpu
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

np = pytest.importorskip("numpy")
from beholder_amd.ops import gpu_extract as gx, gpu_fold, hip_lib  # noqa: E402
from extract_cases import FFFD, KINDS, collision_pairs  # noqa: E402
from telemetry_corpus import body as _body, fold_corpus as _corpus, varint as _varint  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
SHAPES = sorted(gx.GATHER_SHAPES)


def _both_shapes(data: bytes, selector: Selector, want: Extract, dialect: str = "protobufjs", **kw) -> int:
    """Asserts both gather shapes against ``want``; returns the host-frame count."""
    assert extract_gpu(data, selector, DEVICE, dialect, **kw) == want  # the public call, the default shape
    counts = set()
    for shape in SHAPES:
        got, host_frames = gx.extract(data, selector, DEVICE, dialect, shape=shape, **kw)
        assert got.frames == want.frames and got.indices == want.indices, shape
        assert got.data == want.data, shape
        counts.add(host_frames)
    assert len(counts) == 1
    return counts.pop()


@functools.lru_cache(maxsize=None)
def _corpus_cpu(kind: str, dialect: str) -> Extract:
    return extract_cpu(_corpus(), KINDS[kind], dialect)


def test_empty_stream_launches_nothing(monkeypatch):
    def no_library():
        raise AssertionError("an empty stream must not reach the library")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    for selector in (Selector(), Selector(media={"m"}, invert=True)):
        assert extract_gpu(b"", selector, DEVICE) == Extract() == extract_cpu(b"", selector)


@pytest.mark.parametrize("topic", [STATUS_ID, PROGRESS_ID, 9])
def test_single_frame_kept_and_dropped(topic):
    for body in (_body(b"m-1", 3), b"", b"\x2e"):
        data = frames([(topic, body)])
        for selector in (Selector(), Selector(invert=True), Selector(topics={topic}), Selector(media={"m-1"}),
                         Selector(outcomes={"error"})):
            want = extract_cpu(data, selector)
            assert want.frames == 1 and want.data in (data, b"")
            _both_shapes(data, selector, want)


def _keep_pattern(name: str, n: int) -> list:
    rng = random.Random(7)
    return {"all": [True] * n, "none": [False] * n, "first": [i == 0 for i in range(n)],
            "last": [i == n - 1 for i in range(n)], "every-other": [i % 2 == 0 for i in range(n)],
            "random-half": [rng.random() < 0.5 for _ in range(n)]}[name]


@pytest.mark.parametrize("pattern", ["all", "none", "first", "last", "every-other", "random-half"])
def test_one_block_and_one_lane(pattern):
    """257 frames: block 0 is full and block 1 holds a single frame. Kept frames are topic 9."""
    pattern_bits = _keep_pattern(pattern, 257)
    data = frames([(9 if keep else PROGRESS_ID, _body(b"m-%d" % i, i % 7)) for i, keep in enumerate(pattern_bits)])
    want = extract_cpu(data, Selector(topics={9}))
    assert want.indices == [i for i, keep in enumerate(pattern_bits) if keep]
    _both_shapes(data, Selector(topics={9}), want)


GATHER_LENGTHS = [0, 1, 2, 3, 4, 11, 59, 60, 63, 64, 65, 127, 128, 129, 255, 256, 257, 5000]


def _edge_events(rng: random.Random) -> list:
    """Progress frames whose body lengths run through GATHER_LENGTHS, eight of each, shuffled: a body
    is one ``host`` field (tag, length, that many bytes) sized to the length asked for."""
    events = []
    for length in GATHER_LENGTHS * 8:
        if length < 2:
            body = b"\x10"[:length]
        else:
            fill = length - 2 if length - 2 < 128 else length - 3  # the length varint takes 1 or 2 bytes
            body = b"\x22" + _varint(fill) + b"h" * fill
        assert len(body) == length, (length, len(body))
        events.append((PROGRESS_ID, body))
    rng.shuffle(events)
    return events


@pytest.mark.parametrize("ends_kept", [False, True])
def test_gather_edges(ends_kept):
    """Body lengths through every size around the 16-byte word and the 64-lane stride, shuffled, every
    other frame kept: source and destination offsets take every alignment mod 16. With ``ends_kept``
    the first and the last frame of the buffer are kept: a read past ``buf`` or a write past the
    output would be theirs."""
    events = _edge_events(random.Random(6 + ends_kept))  # seeds under which the assertion on alignments holds
    n = len(events)
    kept = [i % 2 == (0 if ends_kept else 1) for i in range(n)]
    if ends_kept:
        kept[n - 1] = True
    else:
        kept[0] = kept[n - 1] = False
    data = frames([(9 if keep else topic, body) for keep, (topic, body) in zip(kept, events)])
    offs = gpu_fold.index(data)[1]
    want = extract_cpu(data, Selector(topics={9}))
    assert want.indices == [i for i, keep in enumerate(kept) if keep]
    src = {int(offs[i]) % 16 for i in want.indices}
    out_offs = np.concatenate(([0], np.cumsum([int(offs[i + 1] - offs[i]) for i in want.indices])))
    assert src == set(range(16)) and {int(o) % 16 for o in out_offs[:-1]} == set(range(16))
    _both_shapes(data, Selector(topics={9}), want)


@pytest.mark.parametrize("select", ["alternate", "last"])
def test_the_totals_scan_takes_a_second_tile(select):
    """256 * 256 + 1 empty-body frames: 257 block totals, one more than the totals scan covers in one
    step (gpu_extract.SCAN_BLOCK = 256), so its carry crosses a tile."""
    assert gx.SCAN_BLOCK == 256
    n = 256 * 256 + 1
    data = bytearray(frames([(9 if i % 2 == 0 else STATUS_ID, b"") for i in range(n)]))
    assert len(data) == 5 * n
    if select == "last":
        data[4:5 * (n - 1):10] = bytes([STATUS_ID]) * len(data[4:5 * (n - 1):10])  # only frame n - 1 keeps topic 9
    data = bytes(data)
    want = extract_cpu(data, Selector(topics={9}))
    assert want.indices == (list(range(0, n, 2)) if select == "alternate" else [n - 1])
    _both_shapes(data, Selector(topics={9}), want)


@pytest.mark.parametrize("dialect", ops.DIALECTS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fold_corpus(kind, dialect):
    want = _corpus_cpu(kind, dialect)
    assert want.frames > 5000 and want.indices
    host_frames = _both_shapes(_corpus(), KINDS[kind], want, dialect)
    assert 0 < host_frames <= 0.05 * want.frames


def test_the_extract_is_deterministic():
    first = extract_gpu(_corpus(), KINDS["media"], DEVICE)
    assert first == extract_gpu(_corpus(), KINDS["media"], DEVICE) == _corpus_cpu("media", "protobufjs")


@pytest.mark.parametrize("hash_mask", [0x3, 0])
def test_forced_collisions_stay_exact(hash_mask):
    """Only the -x id of each of 60 pairs is queried; hash_mask 0x3 homes them in four slots (0: in
    one), and a -y id differs from its -x in the last byte only: no -y frame is kept."""
    pairs = collision_pairs()
    rng = random.Random(1)
    events = [(topic, _body(mid, rng.randrange(6))) for pair in pairs for mid in pair
              for topic in (STATUS_ID, PROGRESS_ID)]
    rng.shuffle(events)
    data = frames(events)
    selector = Selector(media={x.decode() for x, _ in pairs})
    want = extract_cpu(data, selector)
    assert len(want.indices) == 120 and want.frames == 240 and b"-y" not in want.data
    assert _both_shapes(data, selector, want, hash_mask=hash_mask) == 0


@pytest.mark.parametrize("dialect", ops.DIALECTS)
def test_non_ascii_ids_take_the_host_path(dialect):
    rng = random.Random(4)
    plain = [b"ascii-%d" % k for k in range(20)]
    other = ["é".encode(), "メディア".encode(), b"\xff", b"\xfe", b"ok\x80", b"\xc3", b"caf\xc3\xa9", b"\xf0\x9f\x8e\xac"]
    events, host = [], 0
    for _ in range(600):
        mid = rng.choice(other) if rng.random() < 0.3 else rng.choice(plain)
        host += mid in other
        events.append((rng.choice((STATUS_ID, PROGRESS_ID)), _body(mid, rng.randrange(7))))
    data = frames(events)
    assert 100 < host < 300
    kept = {}
    for query in ({FFFD}, {"é"}, {"ascii-3"}, {FFFD, "é", "ascii-3"}):
        selector = Selector(media=query)
        want = extract_cpu(data, selector, dialect)
        assert _both_shapes(data, selector, want, dialect) == host
        kept[frozenset(query)] = len(want.indices)
    assert kept[frozenset({"ascii-3"})] > 0 and kept[frozenset({"é"})] > 0
    assert (kept[frozenset({FFFD})] > 20) == (dialect == "protobufjs")  # upb rejects invalid UTF-8


def test_larger_batch():
    w = Workload(n_media=256, seed=9)
    data = w.framed(200_000)
    selector = Selector(media={w.media[17].id})
    want = extract_cpu(data, selector)
    assert want.frames == 200_000 and 400 < len(want.indices) < 1600
    assert extract_gpu(data, selector, DEVICE) == want


def test_argument_checks_come_before_any_launch(monkeypatch):
    import torch
    data = frames([(STATUS_ID, _body(b"m", 1))] * 2)
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, DEVICE)
    table, blob = gx.build_media_table([b"m"])
    tables = gx.allocate(buf, offs_dev, n, table, blob)
    params = gx.select_params(Selector(media={"m"}), len(table))

    def no_library():
        raise AssertionError("argument checks come first")
    monkeypatch.setattr(hip_lib, "lib", no_library)
    with pytest.raises(ValueError):
        gx.allocate(buf, offs_dev.to(torch.int64), n, table, blob)  # wrong dtype
    with pytest.raises(ValueError):
        gx.allocate(buf.to(torch.int8), offs_dev, n, table, blob)
    with pytest.raises(ValueError):
        gx.allocate(buf.cpu(), offs_dev.cpu(), n, table, blob)  # host tensors
    with pytest.raises(ValueError):
        gx.allocate(buf, offs_dev, n + 1, table, blob)  # offs is not n + 1
    with pytest.raises(ValueError):
        gx.allocate(buf, offs_dev, n, table[:1], blob)  # not a power of two of entries
    with pytest.raises(ValueError):
        gx.mark(tables, params, dialect="proto2")
    with pytest.raises(ValueError):
        gx.mark(tables, gx.select_params(Selector(), 8))  # params of another table
    with pytest.raises(ValueError):
        gx.gather(tables, 1, 0)  # totals that cannot be
    with pytest.raises(ValueError):
        gx.gather(tables, 3, 40)
    with pytest.raises(ValueError):
        gx.gather(tables, 1, 20, shape="spiral")
    with pytest.raises(ValueError):
        gx.select_params(Selector(), 2, hash_mask=1 << 64)
    with pytest.raises(ValueError):
        extract_gpu(data, Selector(), DEVICE, dialect="proto2")
    with pytest.raises(ValueError):
        extract_gpu(data, Selector(statuses={64}), DEVICE)
    with pytest.raises(ValueError):
        extract_gpu(data, Selector(), "cpu")
    with pytest.raises(ValueError):
        extract_gpu(data[:-1], Selector(), DEVICE)  # broken framing never reaches the device
