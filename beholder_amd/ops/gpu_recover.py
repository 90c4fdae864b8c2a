"""Salvage the frames of a damaged capture on the GPU (``ops/hip/telemetry_recover.hip``): the device
path of ``python -m beholder_amd recover --device gpu`` (:mod:`beholder_amd.recover` defines the
result).

There is no frame index to start from, the framing is what is broken: every table is per byte
offset. The stages, which ``scripts/gpu_recover_probe.py`` times one by one:

1. :func:`upload` — the bytes go to the device as they lie in the file, padded to the candidates
   kernel's 16-byte loads.
2. :func:`candidates` — one lane per offset: a flag byte (``WF``, ``ANCHOR``, ``ASK_HOST``) and
   ``end[p]``. Under upb an offset whose decode rests on a string with a byte >= 0x80 or on a
   start-group goes to the overflow list.
3. :func:`decide_on_host` — reads the list's length; where it is not 0 the host asks
   ``recover.rules_of`` about those offsets and writes their flags back.
4. :func:`next_anchor` — a reverse inclusive min-scan of ``anchor(q) ? q : n`` in three launches, the
   successor of every offset fused into the last.
5. :func:`reach` — pointer doubling from the start, ``(n // 5 + 1).bit_length()`` rounds, no
   readback between them.
6. :func:`collect` — the reached, decided offsets are marked, compacted by the extract's scan
   (``gpu_extract.scan``) and resolved to where their frames start. The host reads the nodes back
   and :func:`assemble` cuts the gaps out of its own copy of the bytes: no gather is needed.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`recover`.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import gpu_extract, hip_lib

RC_WF, RC_ANCHOR, RC_ASK_HOST = 1, 2, 4  # the flag byte of telemetry_recover.hpp
BLOCK = 256  # offsets per block of every kernel of telemetry_recover.hip
# The most bytes one call takes (RC_LIMIT of telemetry_recover.hpp). The tables take 43 bytes per offset
# next to the byte itself: flags 1, end 4, next 4, the two jump buffers 8 (the first doubles as the
# scan's keep_len), reach 1, the overflow list 4, and the scan's pos 8, out_offs 4 and indices 4, plus
# 5 per node of the walk; 11 GiB and a half at the limit.
LIMIT = 2 ** 28


class TooLarge(ValueError):
    """More than :data:`LIMIT` bytes in one call."""


class Tables(NamedTuple):
    """The device tensors of one recover over ``n`` bytes, of which the offsets below ``decided``
    are decided."""
    n: int
    decided: int
    max_frame: int
    buf: object       # uint8, padded: ceil(n / 256) * 256 + 16 bytes, zero behind n
    flags: object     # n + 1 uint8
    end: object       # n int32
    cursor: object    # 1 int32: the length of overflow
    overflow: object  # n int32
    mins: object      # blocks int32, scratch of the min-scan (blocks over n + 1 offsets)
    sfx: object       # blocks + 1 int32, scratch
    next: object      # n + 1 int32: the first anchor at or behind p, or n
    jump: object      # n + 1 int32: succ, then scratch of the doubling, then the scan's keep_len
    spare: object     # n + 1 int32: the doubling's other buffer
    reach: object     # n + 1 uint8


class Nodes(NamedTuple):
    """What :func:`collect` reads back: the walk's decided nodes, ascending, where each one's frame
    starts (``n`` for none), and whether the node is well framed."""
    at: np.ndarray
    frame_at: np.ndarray
    framed: np.ndarray


def _check_policy(policy) -> None:
    from .. import recover
    if not isinstance(policy, recover.Policy):
        raise TypeError(f"policy is a recover.Policy, not {type(policy).__name__}")
    if isinstance(policy.max_frame, bool) or not isinstance(policy.max_frame, int) or \
            not 1 <= policy.max_frame <= recover.MAX_FRAME_LIMIT:
        raise ValueError(f"max_frame must be in 1..{recover.MAX_FRAME_LIMIT}")


def check_size(size: int) -> None:
    """:class:`TooLarge` for more bytes than one call takes."""
    if size > LIMIT:
        raise TooLarge(f"{size} bytes are more than the {LIMIT} that one recover call on the device takes")


def padded_size(n: int) -> int:
    """The bytes of the device buffer for ``n`` bytes: whole blocks and the last block's halo."""
    return (n + BLOCK - 1) // BLOCK * BLOCK + 16


def upload(data, device):
    """``data`` in a zeroed device buffer of :func:`padded_size`."""
    import torch
    n = len(data)
    check_size(n)
    buf = torch.zeros(padded_size(n), dtype=torch.uint8, device=device)
    buf[:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8) if n else buf[:0]
    return buf


def allocate(buf_dev, n: int, policy, final: bool = True) -> Tables:
    """Tables for the ``n`` bytes at the head of ``buf_dev``, zeroed where the kernels need it. Checks
    the arguments on the host."""
    import torch

    from .. import recover
    _check_policy(policy)
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("the recover needs n >= 1")
    check_size(n)
    if buf_dev.dtype != torch.uint8 or not buf_dev.is_cuda or not buf_dev.is_contiguous() or buf_dev.dim() != 1:
        raise ValueError("the kernels need a contiguous uint8 buf on a GPU")
    if buf_dev.numel() < padded_size(n) or buf_dev.data_ptr() % 16:
        raise ValueError("buf is upload()'s: padded to whole blocks and 16 bytes, 16-byte aligned")
    if not isinstance(final, bool):
        raise TypeError("final is a bool")
    dev = buf_dev.device
    blocks = (n + 1 + BLOCK - 1) // BLOCK

    def empty(size, dtype=torch.int32):
        return torch.empty(size, dtype=dtype, device=dev)
    return Tables(n, recover.decided_end(n, policy, final), policy.max_frame, buf_dev,
                  torch.zeros(n + 1, dtype=torch.uint8, device=dev), empty(n),
                  torch.zeros(1, dtype=torch.int32, device=dev), empty(n), empty(blocks), empty(blocks + 1),
                  empty(n + 1), empty(n + 1), empty(n + 1), torch.zeros(n + 1, dtype=torch.uint8, device=dev))


def candidates(t: Tables, dialect: str = "protobufjs") -> None:
    """The candidates launch over ``t`` on the current torch stream. ``t.cursor`` must be zero."""
    dialect_id = hip_lib.check_dialect(dialect)
    hip_lib.call("bh_recover_candidates", t.buf, t.buf.data_ptr(), t.buf.numel(), t.n, t.decided, t.max_frame,
                 dialect_id, t.flags.data_ptr(), t.end.data_ptr(), t.cursor.data_ptr(), t.overflow.data_ptr())


def decide_on_host(t: Tables, data, policy, dialect: str = "protobufjs") -> int:
    """Reads the overflow list's length; where it is not 0, asks ``recover.rules_of`` about those
    offsets and writes ``WF | ANCHOR`` or ``WF`` back into ``t.flags``. Returns the length."""
    import torch

    from .. import recover
    count = int(t.cursor.item())
    if count == 0:
        return 0
    asked = np.sort(t.overflow[:count].cpu().numpy()).astype(np.int64)
    anchor = recover.rules_of(data, policy, dialect)[1]
    flags = np.fromiter((RC_WF | RC_ANCHOR if anchor(q) else RC_WF for q in asked.tolist()), dtype=np.uint8, count=count)
    dev = t.buf.device
    t.flags[torch.from_numpy(asked).to(dev)] = torch.from_numpy(flags).to(dev)
    return count


def next_anchor(t: Tables) -> None:
    """The three launches of the reverse min-scan, with the successor: fills ``t.next`` and ``t.jump``."""
    hip_lib.call("bh_recover_next", t.buf, t.flags.data_ptr(), t.end.data_ptr(), t.n, t.decided, t.mins.data_ptr(),
                 t.sfx.data_ptr(), t.next.data_ptr(), t.jump.data_ptr())


def reach(t: Tables, resync: bool = False) -> None:
    """The doubling rounds from the start: 0, or ``next[0]`` when entered with a gap open.
    ``t.reach`` must be zero and ``t.jump`` :func:`next_anchor`'s."""
    if not isinstance(resync, bool):
        raise TypeError("resync is a bool")
    hip_lib.call("bh_recover_reach", t.buf, t.next.data_ptr(), t.jump.data_ptr(), t.spare.data_ptr(),
                 t.reach.data_ptr(), t.n, int(resync))


def collect(t: Tables) -> Nodes:
    """Marks the reached, decided offsets, compacts them with the extract's scan and resolves each
    to its frame; the three lists come back to the host."""
    import torch
    keep_len = t.jump[:t.n]  # the doubling is done with it
    hip_lib.call("bh_recover_mark", t.buf, t.reach.data_ptr(), t.n, t.decided, keep_len.data_ptr())
    s = gpu_extract.scan_tables(keep_len, t.n, t.buf, None)
    gpu_extract.scan(s)
    count = gpu_extract.totals(s)[0]
    frame_at = torch.empty(count, dtype=torch.int32, device=t.buf.device)
    framed = torch.empty(count, dtype=torch.uint8, device=t.buf.device)
    if count:
        hip_lib.call("bh_recover_resolve", t.buf, s.indices.data_ptr(), count, t.flags.data_ptr(), t.next.data_ptr(),
                     frame_at.data_ptr(), framed.data_ptr())
    return Nodes(s.indices[:count].cpu().numpy().astype(np.int64), frame_at.cpu().numpy().astype(np.int64),
                 framed.cpu().numpy().astype(bool))


def assemble(nodes: Nodes, data, policy, dialect: str, final: bool, resync: bool, base: int = 0):
    """The :class:`recover.Recovered` of the walk's nodes over the host's copy of the bytes."""
    from .. import recover
    n = len(data)
    decided = recover.decided_end(n, policy, final)
    found = nodes.frame_at < n  # every node but, at most, the last: a gap with no anchor behind it
    offsets = nodes.frame_at[found]
    opened = ~nodes.framed
    gap_at = nodes.at[opened]
    gap_end = np.where(found[opened], nodes.frame_at[opened], decided)
    anchors = int((opened & found).sum())
    if resync:  # the walk began at next[0]: a gap from 0 up to it, and its frame is an anchor's
        first = int(nodes.at[0]) if len(nodes.at) else decided
        gap_at, gap_end = np.concatenate(([0], gap_at)), np.concatenate(([first], gap_end))
        anchors += bool(len(nodes.at))
    still_open = not bool(found[-1]) if len(found) else resync
    if still_open:
        consumed = decided
    elif len(offsets):
        last = int(offsets[-1])
        consumed = last + 4 + int.from_bytes(bytes(memoryview(data)[last:last + 4]), "little")
    else:
        consumed = 0
    gaps = [(a, b - a) for a, b in zip(gap_at.tolist(), gap_end.tolist()) if b > a]
    return recover.assemble(data, offsets.tolist(), gaps, anchors, consumed, still_open, policy, dialect, base)


def recover(data, policy, device="cuda", dialect: str = "protobufjs", final: bool = True, resync: bool = False,
            base: int = 0):
    """``(Recovered, offsets decided on the host)`` of a buffer through the device."""
    from .. import recover as definition
    _check_policy(policy)
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "recover")
    definition._check_entry(final, resync, base)
    n = len(data)
    check_size(n)
    if n == 0:
        return definition.assemble(data, [], [], 0, 0, resync, policy, dialect, base), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    t = allocate(upload(data, device), n, policy, final)
    candidates(t, dialect)
    host_offsets = decide_on_host(t, data, policy, dialect)
    next_anchor(t)
    reach(t, resync)
    return assemble(collect(t), data, policy, dialect, final, resync, base), host_offsets
