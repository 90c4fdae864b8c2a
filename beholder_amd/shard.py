"""Split a framed stream by media into N framed streams, for parallel replay that keeps its order.

``service.ordering: per_media`` serialises handlers per decoded ``mediaId`` (quirk Q9), but only
inside one process: ``run --workers N`` and extra replicas are competing consumers, and two events
of one media can reach Trello and the store out of order. A dead-letter file replayed through N
consumers therefore had to give up either order or parallelism. :func:`shard_cpu` partitions a
capture **by media**: every media's events stay in one stream, in their original order, so each
stream can go to a consumer of its own (``run --source stdin``, or one ``publish`` per queue).
:func:`shard_cpu` is the definition; :func:`shard_gpu` computes the same :class:`Sharded` on the
device (``ops/hip/telemetry_shard.hip``, ``ops/gpu_shard.py``).

Frame ``i`` of the stream is read the way the fold, the extract and the coalesce read it (topic 1
as ``api.TelemetryStatus``, topic 2 as ``api.TelemetryProgress``, in the service's dialect), which
gives it an outcome of ``decoded``, ``error`` or ``other``. A ``mediaId`` is the decoded string,
exactly as ``coalesce.key_of`` and ``Service._media_key`` see it: U+FFFD for invalid UTF-8 under
protobufjs, and an absent field is ``""``. Both topics of one media go to the same shard.

:func:`shard_of` is a function of the decoded string and the shard count alone, so shard files made
from different captures, chunks or machines agree. A frame that is no decoded event has no media
and no ordering constraint: under ``undecoded=first`` it goes to shard 0, so the shards are a
partition of the input; under ``drop`` it goes nowhere.

Results merge by concatenation: ``shard(a + b) == shard(a).merge(shard(b))`` for a cut at any frame
boundary, which is how :func:`shard_file` handles a file of any size in chunks.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, List, Optional

from . import capture_io, ops, replay
from .capture_io import frame_spans
from .models import proto
from .topics import PROGRESS_ID, STATUS_ID

DROP = "drop"  # route_of's answer that is no shard number
MAX_SHARDS = 256
UNDECODED_MODES = ("first", "drop")
_ALL_ONES = 0xFFFFFFFFFFFFFFFF


def hash64(b: bytes) -> int:
    """The fold's hash of an id (FNV-1a, then murmur3's 64-bit finaliser), restated from
    ``ops/gpu_fold.hash64`` so that the CPU path needs neither numpy nor torch."""
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & _ALL_ONES
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & _ALL_ONES
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & _ALL_ONES
    return h ^ (h >> 33)


def _check_shards(shards) -> None:
    if not isinstance(shards, int) or isinstance(shards, bool):
        raise TypeError(f"shards is an int, not {type(shards).__name__}")
    if not 1 <= shards <= MAX_SHARDS:
        raise ValueError(f"shards must be in 1..{MAX_SHARDS}, not {shards}")


def shard_of(media_id: str, shards: int) -> int:
    """The shard of ``media_id`` among ``shards``: the high half of its hash, scaled to
    ``[0, shards)`` by a multiply and a shift. Depends on nothing else."""
    _check_shards(shards)
    return ((hash64(media_id.encode("utf-8")) >> 32) * shards) >> 32


@dataclasses.dataclass(frozen=True)
class Policy:
    """How many shards, and what happens to frames that are no decoded event (``error``,
    ``other``): ``first`` sends them to shard 0, ``drop`` nowhere."""
    shards: int
    undecoded: str = "first"

    def __post_init__(self):
        _check_shards(self.shards)
        if not isinstance(self.undecoded, str):
            raise TypeError(f"undecoded is a string, not {type(self.undecoded).__name__}")
        if self.undecoded not in UNDECODED_MODES:
            raise ValueError(f"unknown undecoded policy {self.undecoded!r} ({'|'.join(UNDECODED_MODES)})")


@dataclasses.dataclass
class Sharded:
    shards: int
    data: List[bytes] = None        # per shard, its frames byte for byte, in stream order
    indices: List[List[int]] = None  # per shard, their indices in the input, ascending
    frames: int = 0                  # the input's frame count

    def __post_init__(self):
        if self.data is None:
            self.data = [b""] * self.shards
        if self.indices is None:
            self.indices = [[] for _ in range(self.shards)]

    def merge(self, later: "Sharded") -> "Sharded":
        """The result for this one's input followed by ``later``'s. Neither operand changes."""
        if later.shards != self.shards:
            raise ValueError(f"cannot merge {self.shards} shards with {later.shards}")
        return Sharded(self.shards, [a + b for a, b in zip(self.data, later.data)],
                       [a + [i + self.frames for i in b] for a, b in zip(self.indices, later.indices)],
                       self.frames + later.frames)


def route_of(policy: Policy, dialect: str = "protobufjs") -> Callable[[int, bytes], object]:
    """``route(topic, body)`` for ``policy``: the frame's shard number, or ``DROP``. The definition of
    where :func:`shard_cpu` puts a frame, and what the device path asks about the frames it leaves
    to the host."""
    if not isinstance(policy, Policy):
        raise TypeError(f"policy is a shard.Policy, not {type(policy).__name__}")
    replay._check_dialect(dialect)
    status_type, progress_type = replay._types()
    decoders = {STATUS_ID: ops.codec_for(status_type, dialect).decode,
                PROGRESS_ID: ops.codec_for(progress_type, dialect).decode}
    shards = policy.shards
    undecoded = 0 if policy.undecoded == "first" else DROP
    cache = {}  # mediaId -> shard: a capture holds many frames per media

    def route(topic: int, body: bytes):
        decode = decoders.get(topic)
        if decode is None:
            return undecoded
        try:
            mid = decode(body).mediaId
        except proto.DecodeError:
            return undecoded
        s = cache.get(mid)
        if s is None:
            s = cache[mid] = ((hash64(mid.encode("utf-8")) >> 32) * shards) >> 32
        return s
    return route


def shard_cpu(data, policy: Policy, dialect: str = "protobufjs") -> Sharded:
    """The shards of a framed stream, written plainly: the oracle and the ``--device cpu`` path.
    Raises ``ValueError`` for broken framing, as ``extract_cpu`` does."""
    route = route_of(policy, dialect)
    view = memoryview(data)
    parts = [[] for _ in range(policy.shards)]
    indices = [[] for _ in range(policy.shards)]
    frame = 0
    for frame, (a, b) in enumerate(frame_spans(view), 1):
        s = route(view[a + 4], bytes(view[a + 5:b]))
        if s is DROP:
            continue
        parts[s].append(view[a:b])
        indices[s].append(frame - 1)
    return Sharded(policy.shards, [b"".join(p) for p in parts], indices, frame)


def shard_gpu(data, policy: Policy, device="cuda", dialect: str = "protobufjs") -> Sharded:
    """The same :class:`Sharded` as :func:`shard_cpu`, computed on ``device``: the host indexes the
    frame headers, the device routes every frame, partitions them by shard with a stable counting
    sort and gathers the bytes (``ops/gpu_shard.py``). ``data`` must be below 2^31 bytes
    (:func:`shard_file` cuts chunks). Raises if the HIP library or the device is missing."""
    from .ops import gpu_shard
    replay._check_dialect(dialect)
    return gpu_shard.shard(data, policy, device=device, dialect=dialect)[0]


def shard_file(path, outs, policy: Policy, device: str = "cpu", dialect: str = "protobufjs",
               chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES, indices_outs: Optional[list] = None) -> dict:
    """Shard the file at ``path`` (or an open binary file) chunk by chunk into the binary files
    ``outs``, one per shard: each chunk is cut at a frame boundary (``replay.iter_chunks``) and its
    shards are written before the next is read, so memory stays at the chunk size and a stream that
    ends inside a frame leaves whole frames only, and then raises. ``device`` is ``cpu`` or a torch
    device string (``gpu`` means ``cuda``). ``indices_outs``, text files, one per shard, get the
    input indices of that shard's frames, one per line.
    Returns ``{frames, kept, kept_bytes, host_frames, per_shard: [{frames, bytes}, ...]}``;
    ``host_frames`` counts the frames a device run left to the host."""
    if not isinstance(policy, Policy):
        raise TypeError(f"policy is a shard.Policy, not {type(policy).__name__}")
    replay._check_dialect(dialect)
    if len(outs) != policy.shards or (indices_outs is not None and len(indices_outs) != policy.shards):
        raise ValueError(f"{policy.shards} shards need {policy.shards} output files")

    def on_device(device):
        from .ops import gpu_shard
        return lambda chunk: gpu_shard.shard(chunk, policy, device=device, dialect=dialect)
    cut = capture_io.per_chunk(device, lambda chunk: shard_cpu(chunk, policy, dialect), on_device)
    counts = {"frames": 0, "kept": 0, "kept_bytes": 0, "host_frames": 0,
              "per_shard": [{"frames": 0, "bytes": 0} for _ in range(policy.shards)]}
    with capture_io.open_source(path) as f:
        for _, part, host_frames in capture_io.chunk_parts(f, chunk_bytes, replay.iter_chunks, cut):
            for s, (data, indices) in enumerate(zip(part.data, part.indices)):
                if not indices:
                    continue
                outs[s].write(data)
                if indices_outs is not None:
                    capture_io.write_indices(indices_outs[s], indices, counts["frames"])
                counts["per_shard"][s]["frames"] += len(indices)
                counts["per_shard"][s]["bytes"] += len(data)
                counts["kept"] += len(indices)
                counts["kept_bytes"] += len(data)
            counts["frames"] += part.frames
            counts["host_frames"] += host_frames
    return counts
