"""Cut a framed telemetry stream down to the frames that set its end state on the GPU
(``ops/hip/telemetry_coalesce.hip``): the device path of ``python -m beholder_amd coalesce --device gpu``
(:mod:`beholder_amd.coalesce` defines the result).

The stages, which ``scripts/gpu_coalesce_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the host, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`launch` — classify (one lane per frame decides it: drop, keep, keyed, or left to the
   host), claim (the keyed frames group by key in an open-addressing table and each group's last
   frame wins an atomic max) and mark (the kept length of every frame, and which frames are keyed).
   The policy travels as :class:`CoalesceParams`.
3. :func:`decide_on_host` — frames the device does not decide (the fold's rule: ids with a byte
   >= 0x80; in the upb dialect also non-ASCII hosts and groups) come back as a list, and
   ``coalesce.key_of`` decides them. Only the list's length is read back when it is empty. A host
   frame's key can equal a device frame's only where its id is ASCII (upb: a valid non-ASCII host);
   then, and only then, the device's groups are read back and the loser's kept length is cleared.
4. ``gpu_extract.scan``, ``totals`` and ``gather`` — the extract's prefix sum and copy, as they are,
   over this module's ``keep_len``.
5. :func:`collect` — the output bytes, the kept indices and their keyed flags come back.
6. :func:`finish` — the host calls ``key_of`` on the kept keyed frames only, one decode per distinct
   key, to fill ``Coalesced.keys``.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`coalesce`.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from . import gpu_extract, gpu_fold, hip_lib
from .gpu_fold import ALL_ONES

# CF_* of telemetry_coalesce.hpp
CF_STATUS_ALL, CF_PROGRESS_KEYED, CF_PER_STATUS, CF_PROGRESS_ALL, CF_UNDECODED_KEEP = 1, 2, 4, 8, 16
# CL_* of telemetry_coalesce.hpp, the low two bits of a row's flags; R_STATUS marks a keyed status row
CL_DROP, CL_KEEP, CL_KEYED, CL_HOST = 0, 1, 2, 3
R_KIND, R_STATUS = 3, 4
STAGE_CLASSIFY, STAGE_CLAIM, STAGE_MARK, ALL_STAGES = 1, 2, 4, 7


class CoalesceParams(ctypes.Structure):
    """CoalesceParams of telemetry_coalesce.hpp, field for field."""
    _fields_ = [("hash_mask", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("slot_mask", ctypes.c_uint32)]


assert ctypes.sizeof(CoalesceParams) == 16


def key_hash(mid: bytes, topic: int, status: int = 0) -> int:
    """The kernel's hash of a key: the fold's hash of the id bytes, then the topic and the status
    (0 unless the policy is ``per-status`` and the topic is progress) mixed in."""
    h = gpu_fold.hash64(mid)
    h ^= (topic << 32) | (status & 0xFFFFFFFF)
    h = (h * 0xff51afd7ed558ccd) & ALL_ONES
    return h ^ (h >> 33)


def policy_flags(policy) -> int:
    from .. import coalesce
    if not isinstance(policy, coalesce.Policy):
        raise TypeError(f"policy is a coalesce.Policy, not {type(policy).__name__}")
    return ((CF_STATUS_ALL if policy.status == "all" else 0)
            | (CF_PROGRESS_KEYED if policy.progress in ("last", "per-status") else 0)
            | (CF_PER_STATUS if policy.progress == "per-status" else 0)
            | (CF_PROGRESS_ALL if policy.progress == "all" else 0)
            | (CF_UNDECODED_KEEP if policy.undecoded == "keep" else 0))


def coalesce_params(policy, slots: int, hash_mask: int = ALL_ONES) -> CoalesceParams:
    """``policy`` flattened for the kernels. Checks what they cannot: the 64-bit mask."""
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    if slots < 2 or slots & (slots - 1) or slots > 1 << 32:
        raise ValueError("the group table's size is a power of two")
    return CoalesceParams(hash_mask, policy_flags(policy), slots - 1)


class Tables(NamedTuple):
    """The device tensors of one coalesce. ``select`` holds the extract's tensors over the same
    ``keep_len``, for ``gpu_extract.scan``, ``totals`` and ``gather``."""
    n: int
    slots: int
    buf: object
    offs: object
    rows: object      # (n, 6) int32: hash lo, hash hi, id_off, id_len, status, flags
    claim: object     # slots int64: 0 or 1 + the frame that claimed the slot
    winner: object    # slots int32: 0 or 1 + the last frame of the slot's key
    slot_of: object   # n int32: a keyed frame's slot
    keep_len: object  # n int32: the frame's length where it is kept, else 0
    keyed: object     # n uint8: 1 for a keyed frame
    cursor: object    # 1 int32: the length of overflow
    overflow: object  # n int32
    select: gpu_extract.ScanTables


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Tables for ``n`` frames next to ``buf_dev``, the group table zeroed. Checks the arguments on
    the host."""
    import torch
    hip_lib.check_stream(buf_dev, offs_dev, n, "the coalesce")
    dev = buf_dev.device
    slots = gpu_fold.table_slots(n)

    def empty(count, dtype):
        return torch.empty(count, dtype=dtype, device=dev)
    keep_len = empty(n, torch.int32)
    return Tables(n, slots, buf_dev, offs_dev, empty((n, 6), torch.int32),
                  torch.zeros(slots, dtype=torch.int64, device=dev), torch.zeros(slots, dtype=torch.int32, device=dev),
                  empty(n, torch.int32), keep_len, empty(n, torch.uint8), torch.zeros(1, dtype=torch.int32, device=dev),
                  empty(n, torch.int32), gpu_extract.scan_tables(keep_len, n, buf_dev, offs_dev))


def launch(t: Tables, params: CoalesceParams, dialect: str = "protobufjs", stages: int = ALL_STAGES) -> None:
    """Classify, claim and/or mark (``stages``, a sum of ``STAGE_*``) over ``t`` on the current torch
    stream. ``t.offs`` must come from ``gpu_fold.index``: the kernels trust it. ``t.cursor``,
    ``t.claim`` and ``t.winner`` must be zero before classify and claim."""
    dialect_id = hip_lib.check_dialect(dialect)
    if not isinstance(stages, int) or not 1 <= stages <= ALL_STAGES:
        raise ValueError("stages is a sum of STAGE_CLASSIFY, STAGE_CLAIM and STAGE_MARK")
    if params.slot_mask + 1 != t.slots:
        raise ValueError("params were made for another table")
    hip_lib.call("bh_coalesce_mark", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id,
                 ctypes.addressof(params), t.rows.data_ptr(), t.cursor.data_ptr(), t.overflow.data_ptr(),
                 t.claim.data_ptr(), t.winner.data_ptr(), t.slot_of.data_ptr(), t.keep_len.data_ptr(),
                 t.keyed.data_ptr(), stages)


def device_groups(t: Tables, data, per_status: bool) -> dict:
    """key -> the winner's frame index for every group of the device's table, with keys as
    ``coalesce.key_of`` writes them. The device keeps ASCII ids only."""
    from ..topics import PROGRESS_ID, STATUS_ID
    used = t.claim.nonzero().squeeze(1)
    rows = t.rows[t.claim[used] - 1].cpu().numpy()
    winners = t.winner[used].cpu().numpy()
    view = memoryview(data)
    groups = {}
    for (_, _, off, length, status, flags), winner in zip(rows.tolist(), winners.tolist()):
        mid = str(view[off:off + length], "ascii")
        if flags & R_STATUS:
            key = (STATUS_ID, mid)
        else:
            key = (PROGRESS_ID, mid, status) if per_status else (PROGRESS_ID, mid)
        groups[key] = winner - 1
    return groups


def decide_on_host(t: Tables, data, offs: np.ndarray, policy, dialect: str = "protobufjs") -> int:
    """Reads the overflow list's length; where it is not 0, decides those frames with
    ``coalesce.key_of``: a kept one gets its length in ``t.keep_len``, a keyed one its flag in
    ``t.keyed``. Among host frames of one key the last is kept. Where a host frame's key has an ASCII
    id the device may hold the same key: its groups are read back, and the earlier of the two
    winners loses its kept length. Returns the list's length."""
    import torch

    from .. import coalesce
    count = int(t.cursor.item())
    if count == 0:
        return 0
    frames, events = hip_lib.overflow_frames(t.overflow, count, data, offs)
    key = coalesce.key_of(policy, dialect)
    lengths = np.zeros(count, dtype=np.int32)
    keyed = np.zeros(count, dtype=np.uint8)
    last = {}  # key -> position in frames of its last host frame
    for k, (i, topic, body) in enumerate(events):
        answer = key(topic, body)
        if answer is coalesce.KEEP:
            lengths[k] = int(offs[i + 1]) - int(offs[i])
        elif answer is not coalesce.DROP:
            keyed[k] = 1
            last[answer] = k  # frames ascend, so the last write is the last frame
    clear = []
    if any(answer[1].isascii() for answer in last):
        groups = device_groups(t, data, policy.progress == "per-status")
        for answer, k in list(last.items()):
            theirs = groups.get(answer)
            if theirs is None:
                continue
            if theirs > int(frames[k]):
                del last[answer]
            else:
                clear.append(theirs)
    for k in last.values():
        i = int(frames[k])
        lengths[k] = int(offs[i + 1]) - int(offs[i])
    dev = t.buf.device
    where = torch.from_numpy(frames.astype(np.int64)).to(dev)
    t.keep_len[where] = torch.from_numpy(lengths).to(dev)
    t.keyed[where] = torch.from_numpy(keyed).to(dev)
    if clear:
        t.keep_len[torch.tensor(clear, dtype=torch.int64, device=dev)] = 0
    return count


def collect(t: Tables, out, kept: int) -> Tuple[bytes, List[int], np.ndarray]:
    """The output stream, the kept frames' input indices and their keyed flags, on the host."""
    indices = t.select.indices[:kept]
    flags = t.keyed[indices.long()].cpu().numpy()
    return out.cpu().numpy().tobytes(), indices.cpu().numpy().tolist(), flags


def finish(data, offs: np.ndarray, indices: List[int], flags: np.ndarray, policy, dialect: str = "protobufjs") -> list:
    """``Coalesced.keys``: ``key_of`` over the kept keyed frames, ``None`` for the others."""
    from .. import coalesce
    key = coalesce.key_of(policy, dialect)
    view = memoryview(data)
    keys: list = [None] * len(indices)
    for k in np.flatnonzero(flags).tolist():  # the keyed ones only: most kept frames of a damaged capture have no key
        i = indices[k]
        a, b = int(offs[i]), int(offs[i + 1])
        keys[k] = key(view[a + 4], bytes(view[a + 5:b]))
    return keys


def coalesce(data, policy, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None):
    """``(Coalesced, frames decided on the host)`` of a framed stream through the device."""
    from .. import coalesce as definition
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "coalesce")
    policy_flags(policy)
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    n, offs = gpu_fold.index(data)
    if n == 0:
        return definition.Coalesced(), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    params = coalesce_params(policy, gpu_fold.table_slots(n), hash_mask)
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    t = allocate(buf, offs_dev, n)
    launch(t, params, dialect)
    host_frames = decide_on_host(t, data, offs, policy, dialect)
    gpu_extract.scan(t.select)
    kept, kept_bytes = gpu_extract.totals(t.select)
    out = gpu_extract.gather(t.select, kept, kept_bytes)
    out_bytes, indices, flags = collect(t, out, kept)
    keys = finish(data, offs, indices, flags, policy, dialect)
    return definition.Coalesced(out_bytes, indices, keys, n), host_frames
