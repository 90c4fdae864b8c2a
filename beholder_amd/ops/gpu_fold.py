"""Fold a framed telemetry stream on the GPU (``ops/hip/telemetry_fold.hip``): the device path of
``python -m beholder_amd summarise --device gpu`` (:mod:`beholder_amd.replay` defines the fold).

The stages, which ``scripts/gpu_fold_probe.py`` times one by one:

1. :func:`index` — the only per-event host work: one pass over the length headers in C
   (``frame_index``, ops/csrc/py_codec.cpp) gives the ``n + 1`` int32 frame starts. It validates the
   framing, so the kernels can trust the offsets.
2. :func:`upload` — the stream goes to the device as it lies in the file, with the offsets.
3. :func:`launch` — pass A (decode, hash, count) and pass B (group by ``mediaId``), two launches on
   the current torch stream.
4. :func:`collect` — compaction with torch on the device (``claim.nonzero()`` and gathers); only the
   counters, the histogram, one row per distinct media and the overflow indices come back.
5. :func:`finish` — the host turns ``(id_off, id_len)`` into id strings from its own copy of the
   stream, and folds the frames the device left to it (ids with a byte >= 0x80, whose identity is
   the *decoded* string; in the upb dialect also non-ASCII hosts and groups) with the service's
   codec.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`fold`.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

from . import hip_lib

ALL_ONES = hip_lib.ALL_ONES
# counters[] of telemetry_fold.hip
C_STATUS_ERR, C_PROGRESS_ERR, C_UNKNOWN_STATUS, C_OTHER_TOPIC, C_OVERFLOW, C_HIST, N_COUNTERS = 0, 1, 2, 3, 4, 8, 72


def hash64(b: bytes) -> int:
    """The kernel's hash of an id: FNV-1a, then murmur3's 64-bit finaliser."""
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & ALL_ONES
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & ALL_ONES
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & ALL_ONES
    return h ^ (h >> 33)


def table_slots(n: int) -> int:
    """Slots of the group table for ``n`` frames: the power of two that is at least ``2n``."""
    return max(2, 1 << (2 * n - 1).bit_length())


def known_mask(names: Dict[int, str]) -> int:
    """Bit ``s`` set for every enum number ``s``; the kernel knows numbers 0-63."""
    mask = 0
    for number in names:
        if not 0 <= number < 64:
            raise ValueError(f"enum number {number} is outside the kernel's 0-63")
        mask |= 1 << number
    return mask


def index(data) -> Tuple[int, np.ndarray]:
    """``(n, offs)``: the frame count and the ``n + 1`` int32 frame starts of a framed stream.
    Raises ``ValueError`` for broken framing or a stream of 2^31 bytes or more."""
    from . import native
    n, raw = native.frame_index(data)
    return n, np.frombuffer(raw, dtype=np.int32)


class Tables(NamedTuple):
    """The device tensors of one fold."""
    n: int
    slots: int
    buf: object
    offs: object
    rows: object      # (n, 6) int32: hash lo, hash hi, id_off, id_len, status, flags
    counters: object  # N_COUNTERS int32
    overflow: object  # n int32
    claim: object     # slots int64: 0 or 1 + the frame that claimed the slot
    last: object      # slots int64: (1 + frame) << 32 | status of the last status frame
    counts: object    # (slots, 3) int32: status_events, progress_events, progress_counted


def upload(data, offs: np.ndarray, device="cuda") -> Tuple[object, object]:
    """The stream and its offsets on ``device``; the host side is viewed in place, not copied."""
    import warnings

    import torch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # a read-only view is all the copy needs
        buf = torch.frombuffer(data, dtype=torch.uint8).to(device)
        return buf, torch.from_numpy(offs).to(device)


def allocate(buf_dev, offs_dev, n: int) -> Tables:
    """Zeroed tables for ``n`` frames next to ``buf_dev``. Checks the arguments on the host."""
    import torch
    hip_lib.check_stream(buf_dev, offs_dev, n, "the fold")
    dev = buf_dev.device
    slots = table_slots(n)
    return Tables(n, slots, buf_dev, offs_dev,
                  torch.empty((n, 6), dtype=torch.int32, device=dev),
                  torch.zeros(N_COUNTERS, dtype=torch.int32, device=dev),
                  torch.empty(n, dtype=torch.int32, device=dev),
                  torch.zeros(slots, dtype=torch.int64, device=dev),
                  torch.zeros(slots, dtype=torch.int64, device=dev),
                  torch.zeros((slots, 3), dtype=torch.int32, device=dev))


def launch(t: Tables, dialect: str = "protobufjs", mask: int = 0, hash_mask: int = ALL_ONES, passes: int = 3) -> None:
    """Pass A and/or pass B (``passes`` 1, 2 or 3) over ``t`` on the current torch stream. ``t.offs``
    must come from :func:`index`: the kernels trust it."""
    dialect_id = hip_lib.check_dialect(dialect)
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    if not 0 <= mask <= ALL_ONES or passes not in (1, 2, 3):
        raise ValueError("the status mask is 64-bit, passes is 1, 2 or 3")
    hip_lib.call("bh_fold_telemetry", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id, mask, hash_mask,
                 t.rows.data_ptr(), t.counters.data_ptr(), t.overflow.data_ptr(), t.claim.data_ptr(),
                 t.last.data_ptr(), t.counts.data_ptr(), t.slots, passes)


class Collected(NamedTuple):
    """What crosses back to the host: O(statuses + distinct media + overflow)."""
    counters: np.ndarray  # N_COUNTERS
    id_off: np.ndarray
    id_len: np.ndarray
    counts: np.ndarray    # (groups, 3)
    last: np.ndarray      # groups, int64
    overflow: object      # the frame indices left to the host, as the device listed them


def collect(t: Tables) -> Collected:
    counters = t.counters.cpu().numpy()
    used = t.claim.nonzero().squeeze(1)
    owner = t.claim[used] - 1
    ids = t.rows[owner, 2:4].cpu().numpy()
    return Collected(counters, ids[:, 0], ids[:, 1], t.counts[used].cpu().numpy(), t.last[used].cpu().numpy(),
                     t.overflow[:int(counters[C_OVERFLOW])].cpu())


def finish(data, offs: np.ndarray, n: int, c: Collected, dialect: str = "protobufjs"):
    """The :class:`~beholder_amd.replay.Summary` from the device's columns and the host's own copy
    of the stream; frames in ``c.overflow`` are folded here with the service's codec."""
    from .. import replay
    names = replay.status_names()
    counters = c.counters
    s = replay.Summary(frames=n, status_decode_errors=int(counters[C_STATUS_ERR]),
                       progress_decode_errors=int(counters[C_PROGRESS_ERR]),
                       progress_unknown_status=int(counters[C_UNKNOWN_STATUS]),
                       other_topic=int(counters[C_OTHER_TOPIC]))
    for number, count in enumerate(counters[C_HIST:C_HIST + 64].tolist()):
        if count:
            s.progress_updates[names[number].lower()] = count
    view = memoryview(data)
    media = s.media
    for off, length, (st, pr, counted), last in zip(c.id_off.tolist(), c.id_len.tolist(), c.counts.tolist(),
                                                    c.last.tolist()):
        fold = replay.MediaFold(st, pr, counted)
        if last:
            status = last & 0xFFFFFFFF
            fold.last_status = status - (1 << 32) if status >= 1 << 31 else status
            fold.last_status_index = ((last >> 32) & 0xFFFFFFFF) - 1
        media[str(view[off:off + length], "ascii")] = fold  # the device keeps ASCII ids only
    if len(c.overflow):
        # the host's frames may share media with the device's (upb), so they fold into the same summary
        replay.fold_events(hip_lib.overflow_frames(c.overflow, len(c.overflow), data, offs)[1], dialect, into=s)
    return s


def fold(data, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None):
    """``(Summary, frames folded on the host)`` of a framed stream through the device."""
    from .. import replay
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "fold")
    hash_mask = hip_lib.check_hash_mask(hash_mask)
    n, offs = index(data)
    if n == 0:
        return replay.Summary(), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf, offs_dev = upload(data, offs, device)
    t = allocate(buf, offs_dev, n)
    launch(t, dialect, known_mask(replay.status_names()), hash_mask)
    c = collect(t)
    return finish(data, offs, n, c, dialect), len(c.overflow)
