"""Drop the byte-identical repeat frames of a framed telemetry stream on the GPU
(``ops/hip/telemetry_dedupe.hip``): the device path of ``python -m beholder_amd dedupe --device gpu``
(:mod:`beholder_amd.dedupe` defines the result).

The stages, which ``scripts/gpu_dedupe_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the host, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`launch` — hash (one lane per frame: kept as it is because its topic is not selected, left
   to the host because its content is longer than ``DEDUPE_DEVICE_MAX``, or hashed), claim (equal
   contents meet in an open-addressing table whose key compare walks the whole content, and each
   content's last or first frame wins an atomic max) and mark (the kept length of every frame). The
   policy travels as :class:`DedupeParams`. ``method`` picks the form of the hash loop and the
   compare loop: ``wide`` reads 8 bytes at a time, ``bytes`` one.
3. :func:`decide_on_host` — the frames above the cap come back as a list and are decided by content
   in a plain dict. Only the list's length is read back when it is empty. A host frame is longer
   than the cap and a device frame is not, so the two never share a content.
4. ``gpu_extract.scan``, ``totals`` and ``gather`` — the extract's prefix sum and copy, as they are,
   over this module's ``keep_len``.
5. :func:`collect` — the output bytes, the kept indices and the kept frames' 64-bit hashes come
   back, so that ``dedupe.dedupe_file`` need not hash in Python when it joins chunks.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`dedupe`.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import gpu_extract, gpu_fold, hip_lib
from .gpu_fold import ALL_ONES

DEDUPE_DEVICE_MAX = 4096  # telemetry_dedupe.hpp: a longer content is decided on the host
DF_FIRST, DF_WIDE = 1, 2  # DF_* of telemetry_dedupe.hpp
STAGE_HASH, STAGE_CLAIM, STAGE_MARK, ALL_STAGES = 1, 2, 4, 7
METHODS = ("wide", "bytes")
DEFAULT_METHOD = "wide"  # docs/DESIGN.md "The dedupe"


class DedupeParams(ctypes.Structure):
    """DedupeParams of telemetry_dedupe.hpp, field for field."""
    _fields_ = [("topics", ctypes.c_uint64 * 4), ("hash_mask", ctypes.c_uint64), ("slot_mask", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


assert ctypes.sizeof(DedupeParams) == 48


def frame_hash(content: bytes) -> int:
    """The kernel's hash of a frame's content (its topic byte and body): the fold's hash, FNV-1a and
    then murmur3's 64-bit finaliser. It only orders the probe and pre-filters; no result depends on it."""
    return gpu_fold.hash64(content)


def _check_policy(policy) -> None:
    from .. import dedupe
    if not isinstance(policy, dedupe.Policy):
        raise TypeError(f"policy is a dedupe.Policy, not {type(policy).__name__}")


def _check_method(method) -> None:
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r} ({'|'.join(METHODS)})")


def dedupe_params(policy, slots: int, hash_mask: int = ALL_ONES, method: str = DEFAULT_METHOD) -> DedupeParams:
    """``policy`` flattened for the kernels. Checks what they cannot: the 64-bit mask."""
    _check_policy(policy)
    _check_method(method)
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    if slots < 2 or slots & (slots - 1) or slots > 1 << 32:
        raise ValueError("the table's size is a power of two")
    p = DedupeParams()
    for t in (range(256) if policy.topics is None else policy.topics):
        p.topics[t >> 6] |= 1 << (t & 63)
    p.hash_mask = hash_mask
    p.slot_mask = slots - 1
    p.flags = (DF_FIRST if policy.keep == "first" else 0) | (DF_WIDE if method == "wide" else 0)
    return p


class Tables(NamedTuple):
    """The device tensors of one dedupe. ``select`` holds the extract's tensors over the same
    ``keep_len``, for ``gpu_extract.scan``, ``totals`` and ``gather``."""
    n: int
    slots: int
    buf: object
    offs: object
    rows: object      # (n, 2) int64: the content hash; the content's offset | its length << 32 (0: kept, -1: host)
    claim: object     # slots int64: 0 or 1 + the frame that claimed the slot
    winner: object    # slots int32: 0, or 1 + the content's last frame, or n - its first frame
    slot_of: object   # n int32: a participating device frame's slot
    keep_len: object  # n int32: the frame's length where it is kept, else 0
    cursor: object    # 1 int32: the length of overflow
    overflow: object  # n int32
    select: gpu_extract.ScanTables


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, the table zeroed. Checks the arguments on the host."""
    import torch
    hip_lib.check_stream(buf_dev, offs_dev, n, "the dedupe")
    dev = buf_dev.device
    slots = gpu_fold.table_slots(n)

    def empty(count, dtype):
        return torch.empty(count, dtype=dtype, device=dev)
    keep_len = empty(n, torch.int32)
    return Tables(n, slots, buf_dev, offs_dev, empty((n, 2), torch.int64),
                  torch.zeros(slots, dtype=torch.int64, device=dev), torch.zeros(slots, dtype=torch.int32, device=dev),
                  empty(n, torch.int32), keep_len, torch.zeros(1, dtype=torch.int32, device=dev), empty(n, torch.int32),
                  gpu_extract.scan_tables(keep_len, n, buf_dev, offs_dev))


def launch(t: Tables, params: DedupeParams, stages: int = ALL_STAGES) -> None:
    """Hash, claim and/or mark (``stages``, a sum of ``STAGE_*``) over ``t`` on the current torch
    stream. ``t.offs`` must come from ``gpu_fold.index``: the kernels trust it. ``t.cursor``,
    ``t.claim`` and ``t.winner`` must be zero before hash and claim."""
    if not isinstance(stages, int) or not 1 <= stages <= ALL_STAGES:
        raise ValueError("stages is a sum of STAGE_HASH, STAGE_CLAIM and STAGE_MARK")
    if params.slot_mask + 1 != t.slots:
        raise ValueError("params were made for another table")
    hip_lib.call("bh_dedupe_mark", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, ctypes.addressof(params),
                 t.rows.data_ptr(), t.cursor.data_ptr(), t.overflow.data_ptr(), t.claim.data_ptr(),
                 t.winner.data_ptr(), t.slot_of.data_ptr(), t.keep_len.data_ptr(), stages)


def decide_on_host(t: Tables, data, offs: np.ndarray, policy) -> int:
    """Reads the overflow list's length; where it is not 0, decides those frames by content in a
    plain dict, the last or the first of each content, and writes the kept ones' lengths into
    ``t.keep_len``. Returns the list's length."""
    import torch
    count = int(t.cursor.item())
    if count == 0:
        return 0
    frames, events = hip_lib.overflow_frames(t.overflow, count, data, offs)
    winner = {}  # content -> position in frames of the one that is kept
    for k, (_, topic, body) in enumerate(events):
        content = (topic, body)  # the topic byte and the body are the content
        if policy.keep == "last":
            winner[content] = k  # frames ascend, so the last write is the last frame
        else:
            winner.setdefault(content, k)
    lengths = np.zeros(count, dtype=np.int32)
    for k in winner.values():
        i = int(frames[k])
        lengths[k] = int(offs[i + 1]) - int(offs[i])
    dev = t.buf.device
    t.keep_len[torch.from_numpy(frames.astype(np.int64)).to(dev)] = torch.from_numpy(lengths).to(dev)
    return count


def collect(t: Tables, out, kept: int, data=None,
            offs: Optional[np.ndarray] = None) -> Tuple[bytes, List[int], np.ndarray]:
    """The output stream, the kept frames' input indices and their hashes (a uint64 array, left as
    it arrives: only a many-chunk run reads it), on the host. A kept frame that does not take part
    has the hash 0, which nothing reads. A kept host frame has no device hash: with ``data`` and
    ``offs`` it gets Python's own hash of its bytes instead, which serves the same end because a
    host frame's content is never a device frame's."""
    indices = t.select.indices[:kept]
    rows = t.rows[indices.long()].cpu().numpy()
    indices = indices.cpu().numpy().tolist()
    hashes = rows[:, 0].view(np.uint64).copy()
    if data is not None:
        view = memoryview(data)
        for k in np.flatnonzero((rows[:, 1] >> 32) < 0).tolist():  # len -1: decided on the host
            i = indices[k]
            hashes[k] = hash(bytes(view[int(offs[i]):int(offs[i + 1])])) & ALL_ONES
    return out.cpu().numpy().tobytes(), indices, hashes


def dedupe(data, policy, device="cuda", hash_mask: Optional[int] = None, method: str = DEFAULT_METHOD):
    """``(Deduped, frames decided on the host)`` of a framed stream through the device."""
    from .. import dedupe as definition
    _check_policy(policy)
    _check_method(method)
    hip_lib.require_gpu(device, "dedupe")
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    n, offs = gpu_fold.index(data)
    if n == 0:
        return definition.Deduped(keep=policy.keep, topics=policy.topics, hashes=np.zeros(0, dtype=np.uint64)), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    params = dedupe_params(policy, gpu_fold.table_slots(n), hash_mask, method)
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    t = allocate(buf, offs_dev, n)
    launch(t, params)
    host_frames = decide_on_host(t, data, offs, policy)
    gpu_extract.scan(t.select)
    kept, kept_bytes = gpu_extract.totals(t.select)
    out = gpu_extract.gather(t.select, kept, kept_bytes)
    out_bytes, indices, hashes = collect(t, out, kept, data if host_frames else None, offs)
    return definition.Deduped(out_bytes, indices, n, policy.keep, policy.topics, hashes), host_frames
