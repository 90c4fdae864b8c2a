"""Split a framed telemetry stream by media into N framed streams on the GPU
(``ops/hip/telemetry_shard.hip``): the device path of ``python -m beholder_amd shard --device gpu``
(:mod:`beholder_amd.shard` defines the result).

The stages, which ``scripts/gpu_shard_probe.py`` times one by one:

1. ``gpu_fold.index`` and ``gpu_fold.upload`` — as for the fold: one pass over the length headers
   on the host, then the stream goes to the device as it lies in the file, with its offsets.
2. :func:`route` — one lane per frame decides its shard, or -1 for a dropped frame. The policy
   travels as :class:`ShardParams`.
3. :func:`decide_on_host` — frames the device does not decide (the fold's rule: ids with a byte
   >= 0x80; in the upb dialect also non-ASCII hosts and groups) come back as a list, and
   ``shard.route_of`` decides them; their shard numbers are scattered in before the partition. Only
   the list's length is read back when it is empty.
4. :func:`partition` — a stable counting sort of the frames by shard in three launches: per-block
   per-shard totals, one scan over all of them, and every frame's place among the frames of its
   shard. :func:`boundaries` reads back the ``shards + 1`` words that say where each shard starts;
   the last one sizes the output.
5. ``gpu_extract.gather`` — the extract's copy, as it is, over this module's arrays: one buffer with
   the shards back to back.
6. :func:`collect` — the output bytes and the indices come back and are split at the boundaries.

The extension is loaded by ``ops/hip_lib.py``. A missing library raises; there is no CPU fallback
behind :func:`shard`.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Tuple

import numpy as np

from . import gpu_extract, gpu_fold, hip_lib

BLOCK_FRAMES = 1024  # BLOCK * TILES of telemetry_shard.hip: frames per block of the partition
MAX_SHARDS = 256
SF_UNDECODED_FIRST = 1  # SF_* of telemetry_shard.hpp
METHODS = {"walk": 0, "ballot": 1}
DEFAULT_METHOD = "walk"  # the one whose cost does not depend on the data: docs/DESIGN.md "The shard"
STAGE_COUNT, STAGE_TOTALS, STAGE_APPLY, ALL_STAGES = 1, 2, 4, 7


class ShardParams(ctypes.Structure):
    """ShardParams of telemetry_shard.hpp, field for field."""
    _fields_ = [("shards", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


assert ctypes.sizeof(ShardParams) == 8


def shard_params(policy) -> ShardParams:
    """``policy`` flattened for the kernels."""
    from .. import shard
    if not isinstance(policy, shard.Policy):
        raise TypeError(f"policy is a shard.Policy, not {type(policy).__name__}")
    return ShardParams(policy.shards, SF_UNDECODED_FIRST if policy.undecoded == "first" else 0)


class Tables(NamedTuple):
    """The device tensors of one shard. ``select`` holds the extract's tensors over the same
    ``keep_len``, ``pos``, ``out_offs`` and ``indices``, for ``gpu_extract.gather``."""
    n: int
    shards: int
    blocks: int
    buf: object
    offs: object
    shard_of: object  # n int32: the frame's shard, -1 for a dropped frame
    cursor: object    # 1 int32: the length of overflow
    overflow: object  # n int32
    totals: object    # shards * blocks int64, shard-major: scratch of the partition
    base: object      # shards * blocks + 1 int64; [s * blocks] is frames << 32 | bytes before shard s
    select: gpu_extract.ScanTables


def allocate(buf_dev, offs_dev, n: int, shards: int) -> Tables:
    """Tables for ``n`` frames and ``shards`` shards next to ``buf_dev``. Checks the arguments on
    the host."""
    import torch
    hip_lib.check_stream(buf_dev, offs_dev, n, "the shard")
    if not isinstance(shards, int) or not 1 <= shards <= MAX_SHARDS:
        raise ValueError(f"shards must be in 1..{MAX_SHARDS}")
    blocks = (n + BLOCK_FRAMES - 1) // BLOCK_FRAMES
    if shards * blocks + 1 >= 2 ** 31:
        raise ValueError("the totals table is too large for int32 indexing: cut the stream into chunks")
    dev = buf_dev.device

    def empty(count, dtype):
        return torch.empty(count, dtype=dtype, device=dev)
    # the partition fills pos, out_offs and indices itself: no scan, so none of its scratch
    select = gpu_extract.ScanTables(n, buf_dev, offs_dev, empty(n, torch.int32), None, None, empty(n, torch.int64),
                                    empty(n + 1, torch.int32), empty(n, torch.int32))
    return Tables(n, shards, blocks, buf_dev, offs_dev, empty(n, torch.int32),
                  torch.zeros(1, dtype=torch.int32, device=dev), empty(n, torch.int32),
                  empty(shards * blocks, torch.int64), empty(shards * blocks + 1, torch.int64), select)


def route(t: Tables, params: ShardParams, dialect: str = "protobufjs") -> None:
    """The route launch over ``t`` on the current torch stream. ``t.offs`` must come from
    ``gpu_fold.index``: the kernel trusts it. ``t.cursor`` must be zero."""
    dialect_id = hip_lib.check_dialect(dialect)
    if params.shards != t.shards:
        raise ValueError("params were made for another shard count")
    hip_lib.call("bh_shard_route", t.buf, t.buf.data_ptr(), t.offs.data_ptr(), t.n, dialect_id,
                 ctypes.addressof(params), t.shard_of.data_ptr(), t.cursor.data_ptr(), t.overflow.data_ptr())


def decide_on_host(t: Tables, data, offs: np.ndarray, policy, dialect: str = "protobufjs") -> int:
    """Reads the overflow list's length; where it is not 0, decides those frames with
    ``shard.route_of`` and writes their shards into ``t.shard_of``. Returns the length."""
    import torch

    from .. import shard
    count = int(t.cursor.item())
    if count == 0:
        return 0
    frames, events = hip_lib.overflow_frames(t.overflow, count, data, offs)
    where = shard.route_of(policy, dialect)
    shards = np.full(count, -1, dtype=np.int32)
    for k, (_, topic, body) in enumerate(events):
        s = where(topic, body)
        if s is not shard.DROP:
            shards[k] = s
    dev = t.buf.device
    t.shard_of[torch.from_numpy(frames.astype(np.int64)).to(dev)] = torch.from_numpy(shards).to(dev)
    return count


def partition(t: Tables, method: str = DEFAULT_METHOD, stages: int = ALL_STAGES) -> None:
    """Count, totals and/or apply (``stages``, a sum of ``STAGE_*``) over ``t.shard_of`` on the
    current torch stream."""
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r} ({'|'.join(METHODS)})")
    if not isinstance(stages, int) or not 1 <= stages <= ALL_STAGES:
        raise ValueError("stages is a sum of STAGE_COUNT, STAGE_TOTALS and STAGE_APPLY")
    s = t.select
    hip_lib.call("bh_shard_partition", t.buf, t.shard_of.data_ptr(), t.offs.data_ptr(), t.n, t.shards,
                 t.totals.data_ptr(), t.base.data_ptr(), s.pos.data_ptr(), s.keep_len.data_ptr(),
                 s.out_offs.data_ptr(), s.indices.data_ptr(), METHODS[method], stages)


def boundaries(t: Tables) -> Tuple[np.ndarray, np.ndarray]:
    """``(frames, bytes)`` before each shard after :func:`partition`, ``shards + 1`` of each: the last
    pair is the grand total that sizes the output. One copy to the host."""
    words = t.base[::t.blocks].cpu().numpy()
    return words >> 32, words & 0xFFFFFFFF


def collect(t: Tables, out, first: np.ndarray, starts: np.ndarray) -> Tuple[List[bytes], List[List[int]]]:
    """The shards' bytes and input indices on the host, split at :func:`boundaries`."""
    data = out.cpu().numpy().tobytes()
    indices = t.select.indices[:int(first[-1])].cpu().numpy()
    return ([data[int(starts[s]):int(starts[s + 1])] for s in range(t.shards)],
            [indices[int(first[s]):int(first[s + 1])].tolist() for s in range(t.shards)])


def shard(data, policy, device="cuda", dialect: str = "protobufjs", shape: str = gpu_extract.DEFAULT_GATHER,
          method: str = DEFAULT_METHOD):
    """``(Sharded, frames decided on the host)`` of a framed stream through the device."""
    from .. import shard as definition
    hip_lib.check_dialect(dialect)
    hip_lib.require_gpu(device, "shard")
    params = shard_params(policy)
    if shape not in gpu_extract.GATHER_SHAPES:
        raise ValueError(f"unknown gather shape {shape!r} ({'|'.join(gpu_extract.GATHER_SHAPES)})")
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r} ({'|'.join(METHODS)})")
    n, offs = gpu_fold.index(data)
    if n == 0:
        return definition.Sharded(policy.shards), 0
    hip_lib.lib()  # a missing library raises before anything is uploaded
    buf, offs_dev = gpu_fold.upload(data, offs, device)
    t = allocate(buf, offs_dev, n, policy.shards)
    route(t, params, dialect)
    host_frames = decide_on_host(t, data, offs, policy, dialect)
    partition(t, method)
    first, starts = boundaries(t)
    out = gpu_extract.gather(t.select, int(first[-1]), int(starts[-1]), shape)
    out_data, indices = collect(t, out, first, starts)
    return definition.Sharded(policy.shards, out_data, indices, n), host_frames
