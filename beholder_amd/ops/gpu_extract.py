"""Cut a framed telemetry stream down to selected frames on the GPU
(``ops/hip/telemetry_select.hip``): the device path of ``python -m beholder_amd extract --device gpu``
(:mod:`beholder_amd.extract` defines the result).

The stages, which ``scripts/gpu_extract_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the host, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`mark` — one lane per frame evaluates the selector and writes the frame's kept length.
   The selector travels as :class:`SelectParams` plus a media table (:func:`build_media_table`).
   Frames the device does not decide (the fold's rule: ids with a byte >= 0x80; in the upb dialect
   also non-ASCII hosts and groups) come back as a list; :func:`decide_on_host` asks
   ``extract.predicate`` about them and scatters their lengths in before the scan. Only the list's
   length is read back here, and the scatter is skipped when it is 0.
3. :func:`scan` — the exclusive prefix sum over (kept, kept length) in three launches; :func:`totals`
   reads back the one word that sizes the output.
4. :func:`gather` — copies the kept bytes into a buffer of exactly ``kept_bytes``.
5. :func:`collect` — the output bytes and the kept indices come back.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`extract`.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, NamedTuple, Optional, Tuple

import numpy as np

from . import gpu_fold, hip_lib
from .gpu_fold import ALL_ONES

SCAN_BLOCK = 256  # BLOCK of telemetry_select.hip: frames per block, and totals per step of the totals scan
# flags and outcome bits of telemetry_select.hpp
F_MEDIA, F_STATUS, F_UNKNOWN, F_INVERT = 1, 2, 4, 8
OUTCOME_BITS = {"decoded": 1, "error": 2, "other": 4}
GATHER_SHAPES = {"search": 0, "walk": 1}
DEFAULT_GATHER = "walk"  # the faster one wherever the gather is more than a launch: docs/DESIGN.md "The extract"

ENTRY = np.dtype([("hash", "<u8"), ("off", "<i4"), ("len", "<i4")])  # MediaEntry of telemetry_select.hpp


class SelectParams(ctypes.Structure):
    """SelectParams of telemetry_select.hpp, field for field."""
    _fields_ = [("topics", ctypes.c_uint64 * 4), ("status_mask", ctypes.c_uint64), ("known_mask", ctypes.c_uint64),
                ("hash_mask", ctypes.c_uint64), ("outcomes", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("slot_mask", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


assert ctypes.sizeof(SelectParams) == 72


def ascii_ids(media: Optional[Iterable[str]]) -> List[bytes]:
    """The query ids the device can hold, as bytes, in a fixed order. The others live only on the
    host: a frame that could match one has an id byte >= 0x80 and is left to the host anyway."""
    return sorted(m.encode("ascii") for m in media or () if m.isascii())


def hash64_many(ids: List[bytes]) -> np.ndarray:
    """``gpu_fold.hash64`` of every id, one numpy step per byte position."""
    n = len(ids)
    lens = np.fromiter((len(b) for b in ids), dtype=np.int64, count=n)
    starts = np.concatenate(([0], np.cumsum(lens)[:-1])) if n else lens
    blob = np.frombuffer(b"".join(ids), dtype=np.uint8).astype(np.uint64)
    h = np.full(n, 0xcbf29ce484222325, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(int(lens.max()) if n else 0):
            live = np.nonzero(lens > k)[0]
            h[live] = (h[live] ^ blob[starts[live] + k]) * np.uint64(0x100000001b3)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h


def table_slots(n_ids: int) -> int:
    """Entries of the media table for ``n_ids`` ids: the power of two that is at least twice as many."""
    return max(2, 1 << (2 * n_ids - 1).bit_length()) if n_ids else 2


def build_media_table(ids: List[bytes], hash_mask: int = ALL_ONES) -> Tuple[np.ndarray, np.ndarray]:
    """``(table, blob)`` for distinct ASCII ``ids``: open addressing with linear probing from
    ``hash & hash_mask & (slots - 1)``, an empty entry has ``len`` -1; ``blob`` holds the id bytes
    (one spare byte, so it is never empty)."""
    slots = table_slots(len(ids))
    table = np.zeros(slots, dtype=ENTRY)
    table["len"] = -1
    hashes = hash64_many(ids)
    off = 0
    lens = table["len"]
    for mid, h in zip(ids, hashes.tolist()):
        slot = h & hash_mask & (slots - 1)
        while lens[slot] >= 0:
            slot = (slot + 1) & (slots - 1)
        table[slot] = (h, off, len(mid))
        off += len(mid)
    return table, np.frombuffer(b"".join(ids) + b"\0", dtype=np.uint8)


def select_params(selector, slots: int, hash_mask: int = ALL_ONES) -> SelectParams:
    """``selector`` flattened for the kernel. Checks what the kernel cannot: the 64-bit masks."""
    from .. import replay
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    if slots < 2 or slots & (slots - 1):
        raise ValueError("the media table's size is a power of two")
    p = SelectParams()
    for t in (range(256) if selector.topics is None else selector.topics):
        p.topics[t >> 6] |= 1 << (t & 63)
    p.outcomes = 7 if selector.outcomes is None else sum(OUTCOME_BITS[o] for o in selector.outcomes)
    for s in selector.statuses or ():
        if not 0 <= s <= 63:
            raise ValueError(f"status {s!r} is outside 0-63")
        p.status_mask |= 1 << s
    p.known_mask = gpu_fold.known_mask(replay.status_names())
    p.hash_mask = hash_mask
    p.flags = ((F_MEDIA if selector.media is not None else 0) | (F_STATUS if selector.asks_status else 0)
               | (F_UNKNOWN if selector.unknown_status else 0) | (F_INVERT if selector.invert else 0))
    p.slot_mask = slots - 1
    return p


class ScanTables(NamedTuple):
    """The device tensors that :func:`scan`, :func:`totals`, :func:`gather` and :func:`collect` read,
    over any ``keep_len``: the other commands' way to the extract's prefix sum and copy. Their fields
    are :class:`Tables`'s, so the four functions take either. A caller that fills ``pos``, ``out_offs``
    and ``indices`` itself and only gathers (the shard) may leave ``totals`` and ``base`` ``None``."""
    n: int
    buf: object
    offs: object
    keep_len: object  # n int32: the frame's length where it is kept, else 0
    totals: object    # blocks int64, scratch of the scan
    base: object      # blocks + 1 int64; the last is kept << 32 | kept_bytes
    pos: object       # n int64: output index << 32 | output byte offset
    out_offs: object  # n + 1 int32
    indices: object   # n int32


def scan_tables(keep_len, count: int, buf, offs) -> ScanTables:
    """Scratch and outputs of a scan over the ``count`` words of ``keep_len``, next to it."""
    import torch
    dev = keep_len.device
    blocks = (count + SCAN_BLOCK - 1) // SCAN_BLOCK

    def empty(size, dtype):
        return torch.empty(size, dtype=dtype, device=dev)
    return ScanTables(count, buf, offs, keep_len, empty(blocks, torch.int64), empty(blocks + 1, torch.int64),
                      empty(count, torch.int64), empty(count + 1, torch.int32), empty(count, torch.int32))


class Tables(NamedTuple):
    """The device tensors of one extract."""
    n: int
    buf: object
    offs: object
    table: object     # (slots, 2) int64: the media table's 16-byte entries
    blob: object      # uint8: the table's id bytes
    keep_len: object  # n int32: the frame's length where it is kept, else 0
    cursor: object    # 1 int32: the length of overflow
    overflow: object  # n int32
    totals: object    # blocks int64, scratch of the scan
    base: object      # blocks + 1 int64; the last is kept << 32 | kept_bytes
    pos: object       # n int64: output index << 32 | output byte offset
    out_offs: object  # n + 1 int32
    indices: object   # n int32


def allocate(buf_dev, offs_dev, n: int, table: np.ndarray, blob: np.ndarray) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, the media table uploaded. Checks the arguments
    on the host."""
    import torch
    hip_lib.check_stream(buf_dev, offs_dev, n, "the extract")
    if table.dtype != ENTRY or blob.dtype != np.uint8 or len(table) < 2 or len(table) & (len(table) - 1):
        raise ValueError("the media table is build_media_table's")
    dev = buf_dev.device
    keep_len = torch.empty(n, dtype=torch.int32, device=dev)
    s = scan_tables(keep_len, n, buf_dev, offs_dev)
    return Tables(n, buf_dev, offs_dev,
                  torch.from_numpy(table.view(np.int64).reshape(-1, 2).copy()).to(dev),
                  torch.from_numpy(blob.copy()).to(dev),
                  keep_len, torch.zeros(1, dtype=torch.int32, device=dev),
                  torch.empty(n, dtype=torch.int32, device=dev), s.totals, s.base, s.pos, s.out_offs, s.indices)


def mark(t: Tables, params: SelectParams, dialect: str = "protobufjs") -> None:
    """The mark launch over ``t`` on the current torch stream. ``t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``t.cursor`` must be zero."""
    dialect_id = hip_lib.check_dialect(dialect)
    if params.slot_mask + 1 != t.table.shape[0]:
        raise ValueError("params were made for another table")
    hip_lib.call("bh_select_mark", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id,
                 ctypes.addressof(params), t.table.data_ptr(), t.blob.data_ptr(), t.keep_len.data_ptr(),
                 t.cursor.data_ptr(), t.overflow.data_ptr())


def decide_on_host(t: Tables, data, offs: np.ndarray, selector, dialect: str = "protobufjs") -> int:
    """Reads the overflow list's length; where it is not 0, decides those frames with
    ``extract.predicate`` and writes their kept lengths into ``t.keep_len``. Returns the length."""
    import torch

    from .. import extract
    count = int(t.cursor.item())
    if count == 0:
        return 0
    frames, events = hip_lib.overflow_frames(t.overflow, count, data, offs)
    keep = extract.predicate(selector, dialect)
    lengths = np.zeros(count, dtype=np.int32)
    for k, (i, topic, body) in enumerate(events):
        if keep(topic, body):
            lengths[k] = int(offs[i + 1]) - int(offs[i])
    dev = t.buf.device
    t.keep_len[torch.from_numpy(frames.astype(np.int64)).to(dev)] = torch.from_numpy(lengths).to(dev)
    return count


def scan(t) -> None:
    """The three scan launches over ``t.keep_len`` on the current torch stream. ``t`` is a
    :class:`Tables` or a :class:`ScanTables`, here and in the functions below."""
    hip_lib.call("bh_select_scan", t.keep_len, t.keep_len.data_ptr(), t.n, t.totals.data_ptr(), t.base.data_ptr(),
                 t.pos.data_ptr(), t.out_offs.data_ptr(), t.indices.data_ptr())


def totals(t) -> Tuple[int, int]:
    """``(kept, kept_bytes)`` after :func:`scan`: the one word the host reads to size the output."""
    word = int(t.base[-1].item())
    return word >> 32, word & 0xFFFFFFFF


def gather(t, kept: int, kept_bytes: int, shape: str = DEFAULT_GATHER):
    """The kept bytes in a new device buffer of exactly ``kept_bytes``. ``kept`` and ``kept_bytes``
    must be :func:`totals`'s: the kernels trust them."""
    import torch
    if shape not in GATHER_SHAPES:
        raise ValueError(f"unknown gather shape {shape!r} ({'|'.join(GATHER_SHAPES)})")
    if not (0 <= kept <= t.n and 0 <= kept_bytes <= t.buf.numel() and (kept == 0) == (kept_bytes == 0)):
        raise ValueError("kept and kept_bytes are the scan's totals")
    out = torch.empty(kept_bytes, dtype=torch.uint8, device=t.buf.device)
    if kept == 0:
        return out
    hip_lib.call("bh_select_gather", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, t.keep_len.data_ptr(),
                 t.pos.data_ptr(), t.out_offs.data_ptr(), t.indices.data_ptr(), kept, kept_bytes, out.data_ptr(),
                 GATHER_SHAPES[shape])
    return out


def collect(t, out, kept: int) -> Tuple[bytes, List[int]]:
    """The output stream and the kept frames' input indices, on the host."""
    return out.cpu().numpy().tobytes(), t.indices[:kept].cpu().numpy().tolist()


def extract(data, selector, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None,
            shape: str = DEFAULT_GATHER):
    """``(Extract, frames decided on the host)`` of a framed stream through the device."""
    from .. import extract as definition
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "extract")
    if shape not in GATHER_SHAPES:
        raise ValueError(f"unknown gather shape {shape!r} ({'|'.join(GATHER_SHAPES)})")
    ids = ascii_ids(selector.media)
    params = select_params(selector, table_slots(len(ids)), hash_mask)
    n, offs = gpu_fold.index(data)
    if n == 0:
        return definition.Extract(), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    table, blob = build_media_table(ids, params.hash_mask)
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    t = allocate(buf, offs_dev, n, table, blob)
    mark(t, params, dialect)
    host_frames = decide_on_host(t, data, offs, selector, dialect)
    scan(t)
    kept, kept_bytes = totals(t)
    out = gather(t, kept, kept_bytes, shape)
    out_bytes, indices = collect(t, out, kept)
    return definition.Extract(out_bytes, indices, n), host_frames
