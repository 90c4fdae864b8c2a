"""Cut a framed stream down to the frames that set its end state; the result is a framed stream again.

A dead-letter file or a queue dump from an hour of downtime holds hundreds of superseded events per
media. Replayed as it is, every card moves through every stale list and every stale progress comment
is posted. What decides the end state is, per media, the last status event and the last progress
event. ``extract`` (:mod:`beholder_amd.extract`) cannot say that, because whether a frame is kept
depends on the frames after it: this is a group-by followed by a compaction. :func:`coalesce_cpu`
does it and is the definition; :func:`coalesce_gpu` computes the same :class:`Coalesced` on the
device (``ops/hip/telemetry_coalesce.hip``, ``ops/gpu_coalesce.py``).

Frame ``i`` of the stream is read the way the fold and the extract read it (topic 1 as
``api.TelemetryStatus``, topic 2 as ``api.TelemetryProgress``, in the service's dialect), which
gives it an outcome of ``decoded``, ``error`` or ``other``. A ``mediaId`` is the decoded string:
U+FFFD for invalid UTF-8 under protobufjs, and an absent field is ``""``.

:func:`key_of` turns a :class:`Policy` into the per-frame decision: ``KEEP``, ``DROP`` or a key
tuple. **A keyed frame is kept iff no later frame of the stream has the same key.** Kept frames stay
in stream order, byte for byte.

Results merge: ``coalesce(a + b) == coalesce(a).merge(coalesce(b))`` for a cut at any frame
boundary, which is how :func:`coalesce_file` handles a file of any size in chunks. And coalescing
is idempotent: the coalesced stream coalesces to itself.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Iterator, List, Optional, Tuple

from . import capture_io, ops, replay
from .capture_io import frame_spans as _spans  # the name it had here: test_thin and test_normalise import it
from .models import proto
from .topics import PROGRESS_ID, STATUS_ID

KEEP = "keep"  # key_of's answers that are no key: the frame is kept, or dropped, whatever follows it
DROP = "drop"

STATUS_MODES = ("last", "all")
PROGRESS_MODES = ("last", "per-status", "all", "none")
UNDECODED_MODES = ("keep", "drop")


@dataclasses.dataclass(frozen=True)
class Policy:
    """What of each kind of frame survives. ``status``: the last status event per media, or all of
    them. ``progress``: the last progress event per media, the last per media and status number, all
    or none. ``undecoded``: what happens to frames that are no decoded event (``error``, ``other``)."""
    status: str = "last"
    progress: str = "last"
    undecoded: str = "keep"

    def __post_init__(self):
        for name, allowed in (("status", STATUS_MODES), ("progress", PROGRESS_MODES), ("undecoded", UNDECODED_MODES)):
            value = getattr(self, name)
            if not isinstance(value, str):
                raise TypeError(f"{name} is a string, not {type(value).__name__}")
            if value not in allowed:
                raise ValueError(f"unknown {name} policy {value!r} ({'|'.join(allowed)})")


@dataclasses.dataclass
class Coalesced:
    data: bytes = b""            # the kept frames, headers included, in stream order
    indices: List[int] = dataclasses.field(default_factory=list)  # their indices in the input, ascending
    keys: List[Optional[tuple]] = dataclasses.field(default_factory=list)  # parallel; None: kept without a key
    frames: int = 0              # the input's frame count

    def merge(self, later: "Coalesced") -> "Coalesced":
        """The result for this one's input followed by ``later``'s, from the two results alone: a
        keyed frame of this one goes where ``later`` holds its key. Neither operand changes."""
        superseded = {k for k in later.keys if k is not None}
        view = memoryview(self.data)
        parts, indices, keys = [], [], []
        for (a, b), i, k in zip(_spans(view), self.indices, self.keys):
            if k is None or k not in superseded:
                parts.append(view[a:b])
                indices.append(i)
                keys.append(k)
        parts.append(later.data)
        return Coalesced(b"".join(parts), indices + [i + self.frames for i in later.indices],
                         keys + list(later.keys), self.frames + later.frames)


def key_of(policy: Policy = Policy(), dialect: str = "protobufjs") -> Callable[[int, bytes], object]:
    """``key(topic, body)`` for ``policy``: ``KEEP``, ``DROP`` or the frame's key tuple,
    ``(topic, mediaId)`` or under ``per-status`` ``(topic, mediaId, status)``. The definition of what
    :func:`coalesce_cpu` keeps, and what the device path asks about the frames it leaves to the host."""
    replay._check_dialect(dialect)
    status_type, progress_type = replay._types()
    decode_status = ops.codec_for(status_type, dialect).decode
    decode_progress = ops.codec_for(progress_type, dialect).decode
    undecoded = KEEP if policy.undecoded == "keep" else DROP
    status_mode, progress_mode = policy.status, policy.progress

    def key(topic: int, body: bytes):
        if topic == STATUS_ID:
            try:
                m = decode_status(body)
            except proto.DecodeError:
                return undecoded
            return KEEP if status_mode == "all" else (STATUS_ID, m.mediaId)
        if topic == PROGRESS_ID:
            try:
                m = decode_progress(body)
            except proto.DecodeError:
                return undecoded
            if progress_mode == "last":
                return PROGRESS_ID, m.mediaId
            if progress_mode == "per-status":
                return PROGRESS_ID, m.mediaId, m.status
            return KEEP if progress_mode == "all" else DROP
        return undecoded
    return key


def coalesce_cpu(data, policy: Policy = Policy(), dialect: str = "protobufjs") -> Coalesced:
    """The coalesced stream, written plainly: the oracle and the ``--device cpu`` path. Raises
    ``ValueError`` for broken framing, as ``extract_cpu`` does."""
    key = key_of(policy, dialect)
    view = memoryview(data)
    candidates, last = [], {}
    frame = 0
    for frame, (a, b) in enumerate(_spans(view), 1):
        k = key(view[a + 4], bytes(view[a + 5:b]))
        if k is DROP:
            continue
        if k is KEEP:
            k = None
        else:
            last[k] = frame - 1
        candidates.append((frame - 1, a, b, k))
    kept = [c for c in candidates if c[3] is None or last[c[3]] == c[0]]
    return Coalesced(b"".join(view[a:b] for _, a, b, _ in kept), [i for i, _, _, _ in kept],
                     [k for _, _, _, k in kept], frame)


def coalesce_gpu(data, policy: Policy = Policy(), device="cuda", dialect: str = "protobufjs",
                 hash_mask: Optional[int] = None) -> Coalesced:
    """The same :class:`Coalesced` as :func:`coalesce_cpu`, computed on ``device``: the host indexes
    the frame headers, the device classifies every frame, groups the keyed ones, marks each group's
    last frame, compacts and gathers the kept bytes (``ops/gpu_coalesce.py``). ``data`` must be below
    2^31 bytes (:func:`coalesce_file` cuts chunks). Raises if the HIP library or the device is
    missing."""
    from .ops import gpu_coalesce
    replay._check_dialect(dialect)
    return gpu_coalesce.coalesce(data, policy, device=device, dialect=dialect, hash_mask=hash_mask)[0]


class _Accumulator:
    """The result so far of :func:`coalesce_file`: the kept frames in stream order and a key ->
    position map. A superseded frame becomes a tombstone (its bytes are released at once); the lists
    are rebuilt when more than half of them is tombstones, so the work stays linear in the input."""

    def __init__(self):
        self.frames: List[Optional[bytes]] = []
        self.indices: List[int] = []
        self.keys: List[Optional[tuple]] = []
        self.where = {}
        self.dead = 0

    def add(self, part: Coalesced, base: int) -> None:
        view = memoryview(part.data)
        frames, indices, keys, where = self.frames, self.indices, self.keys, self.where
        for (a, b), i, k in zip(_spans(view), part.indices, part.keys):
            if k is not None:
                old = where.get(k)
                if old is not None:
                    frames[old] = None
                    self.dead += 1
                where[k] = len(frames)
            frames.append(bytes(view[a:b]))
            indices.append(base + i)
            keys.append(k)
        if self.dead > 1024 and 2 * self.dead > len(frames):
            self._compact()

    def _compact(self) -> None:
        live = [p for p, f in enumerate(self.frames) if f is not None]
        self.frames = [self.frames[p] for p in live]
        self.indices = [self.indices[p] for p in live]
        self.keys = [self.keys[p] for p in live]
        self.where = {k: p for p, k in enumerate(self.keys) if k is not None}
        self.dead = 0

    def live(self) -> Iterator[Tuple[bytes, int]]:
        return ((f, i) for f, i in zip(self.frames, self.indices) if f is not None)


def coalesce_file(path, out, policy: Policy = Policy(), device: str = "cpu", dialect: str = "protobufjs",
                  chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES, indices_out=None) -> dict:
    """Coalesce the file at ``path`` (or an open binary file) chunk by chunk into the binary file
    ``out``: each chunk is cut at a frame boundary (``replay.iter_chunks``) and the chunks' results
    are merged on the host. Nothing is written before the last chunk is in, because no frame's fate
    is known before then; a stream that ends inside a frame raises and writes nothing. Memory is the
    chunk plus the result so far (at most one frame per distinct key, plus the frames kept without a
    key), not the file. ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``).
    ``indices_out``, a text file, gets the kept input indices, one per line.
    Returns ``{frames, kept, kept_bytes, keys, host_frames}``: ``keys`` counts the distinct keys of
    the result, ``host_frames`` the frames a device run left to the host."""
    replay._check_dialect(dialect)

    def on_device(device):
        from .ops import gpu_coalesce
        return lambda chunk: gpu_coalesce.coalesce(chunk, policy, device=device, dialect=dialect)
    cut = capture_io.per_chunk(device, lambda chunk: coalesce_cpu(chunk, policy, dialect), on_device)
    acc = _Accumulator()
    frames = host = 0
    with capture_io.open_source(path) as f:
        for _, part, host_frames in capture_io.chunk_parts(f, chunk_bytes, replay.iter_chunks, cut):
            acc.add(part, frames)
            frames += part.frames
            host += host_frames
    kept = kept_bytes = 0
    for frame, i in acc.live():
        out.write(frame)
        if indices_out is not None:
            indices_out.write(f"{i}\n")
        kept += 1
        kept_bytes += len(frame)
    return {"frames": frames, "kept": kept, "kept_bytes": kept_bytes, "keys": len(acc.where), "host_frames": host}
