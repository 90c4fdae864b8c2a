"""Cut a framed stream down to selected frames; the result is a framed stream again.

``summarise`` (:mod:`beholder_amd.replay`) tells an operator what a capture, a ``--dead-letter`` file
or a queue dump will have done once it has gone through the service. The step after it, before
``publish`` replays the file, is a cut: only the frames that fail to decode, only what belongs to
these media, only the progress events whose status is no ``TelemetryStatusEntry`` number (quirk
Q6), or everything except those. :func:`extract_cpu` does that and is the definition;
:func:`extract_gpu` computes the same :class:`Extract` on the device
(``ops/hip/telemetry_select.hip``, ``ops/gpu_extract.py``).

A :class:`Selector` is a conjunction: every field that is given must hold for a frame to match,
and ``invert`` keeps exactly the frames the rest rejects. Frame ``i`` of the stream is read the way
the fold reads it (topic 1 as ``api.TelemetryStatus``, topic 2 as ``api.TelemetryProgress``, in the
service's dialect), which gives it one of three outcomes:

* ``other``: the topic byte is neither ``STATUS_ID`` nor ``PROGRESS_ID``;
* ``error``: the topic's codec raises ``proto.DecodeError``;
* ``decoded``: otherwise. Only a decoded frame has a ``mediaId`` and a ``status``, so ``media`` and
  ``statuses`` / ``unknown_status`` never match any other frame.

A ``mediaId`` is the decoded string, as in the fold: U+FFFD for invalid UTF-8 under protobufjs, and
an absent field is ``""``. ``unknown_status`` is the fold's ``progress_unknown_status`` test (the
status is no number of ``replay.status_names()``), applied to either topic.

Extracts concatenate: ``extract(a + b) == extract(a) + extract(b)`` for a cut at any frame
boundary, which is how :func:`extract_file` handles a file of any size in chunks. And the fold of
the extract for one media is that media's row of the whole fold, with ``indices`` mapping the
frame numbers back.
"""
from __future__ import annotations

import dataclasses
import struct
from typing import Callable, FrozenSet, List, Optional

from . import capture_io, ops, replay
from .models import proto
from .topics import PROGRESS_ID, STATUS_ID

OUTCOMES = ("decoded", "error", "other")


@dataclasses.dataclass(frozen=True)
class Selector:
    """Which frames to keep. A field left at ``None`` (``unknown_status`` at ``False``) asks nothing;
    a selector with nothing set keeps every frame. Sets may be given as any iterable."""
    topics: Optional[FrozenSet[int]] = None     # topic bytes, 0-255
    outcomes: Optional[FrozenSet[str]] = None   # a subset of OUTCOMES
    media: Optional[FrozenSet[str]] = None      # mediaId strings
    statuses: Optional[FrozenSet[int]] = None   # status numbers, 0-63
    unknown_status: bool = False                # ... or a status that is no TelemetryStatusEntry number
    invert: bool = False

    def __post_init__(self):
        for name in ("topics", "outcomes", "media", "statuses"):
            value = getattr(self, name)
            if value is not None:
                if isinstance(value, (str, bytes)):
                    raise TypeError(f"{name} is a set, not a single {type(value).__name__}")
                object.__setattr__(self, name, frozenset(value))
        for t in self.topics or ():
            if not isinstance(t, int) or not 0 <= t <= 255:
                raise ValueError(f"topic {t!r} is no byte (0-255)")
        for o in self.outcomes or ():
            if o not in OUTCOMES:
                raise ValueError(f"unknown outcome {o!r} ({'|'.join(OUTCOMES)})")
        for m in self.media or ():
            if not isinstance(m, str):
                raise TypeError(f"media ids are strings, not {type(m).__name__}")
        for s in self.statuses or ():
            if not isinstance(s, int) or not 0 <= s <= 63:
                raise ValueError(f"status {s!r} is outside 0-63")

    @property
    def asks_status(self) -> bool:
        return self.statuses is not None or self.unknown_status


@dataclasses.dataclass
class Extract:
    data: bytes = b""            # the kept frames, headers included, in stream order
    indices: List[int] = dataclasses.field(default_factory=list)  # their indices in the input, ascending
    frames: int = 0              # the input's frame count

    def __add__(self, later: "Extract") -> "Extract":
        """The extract of this one's input followed by ``later``'s. Neither operand changes."""
        return Extract(self.data + later.data, self.indices + [i + self.frames for i in later.indices],
                       self.frames + later.frames)


def predicate(selector: Selector, dialect: str = "protobufjs") -> Callable[[int, bytes], bool]:
    """``keep(topic, body)`` for ``selector``: the definition of what :func:`extract_cpu` keeps, and
    what the device path asks about the frames it leaves to the host."""
    replay._check_dialect(dialect)
    status_type, progress_type = replay._types()
    decoders = {STATUS_ID: ops.codec_for(status_type, dialect).decode,
                PROGRESS_ID: ops.codec_for(progress_type, dialect).decode}
    names = replay.status_names()
    topics, outcomes, media, statuses = selector.topics, selector.outcomes, selector.media, selector.statuses
    unknown, invert, asks_status = selector.unknown_status, selector.invert, selector.asks_status
    reads = outcomes is not None or media is not None or asks_status  # else the topic byte decides

    def keep(topic: int, body: bytes) -> bool:
        if topics is not None and topic not in topics:
            return invert
        if not reads:
            return not invert
        decode = decoders.get(topic)
        m = None
        if decode is None:
            outcome = "other"
        else:
            try:
                m = decode(body)
                outcome = "decoded"
            except proto.DecodeError:
                outcome = "error"
        match = outcomes is None or outcome in outcomes
        if match and media is not None:
            match = m is not None and m.mediaId in media
        if match and asks_status:
            match = m is not None and (statuses is not None and m.status in statuses
                                       or unknown and m.status not in names)
        return match != invert
    return keep


def extract_cpu(data, selector: Selector, dialect: str = "protobufjs") -> Extract:
    """The extract of a framed stream, written plainly: the oracle and the ``--device cpu`` path.
    Raises ``ValueError`` for broken framing, as ``iter_frames`` does."""
    keep = predicate(selector, dialect)
    view = memoryview(data)
    out, indices = [], []
    i, n, frame = 0, len(view), 0
    while i < n:
        if n - i < 4:
            raise ValueError("truncated frame header")
        (length,) = struct.unpack_from("<I", view, i)
        if length == 0 or n - i - 4 < length:
            raise ValueError("truncated or empty frame")
        end = i + 4 + length
        if keep(view[i + 4], bytes(view[i + 5:end])):
            out.append(view[i:end])
            indices.append(frame)
        i = end
        frame += 1
    return Extract(b"".join(out), indices, frame)


def extract_gpu(data, selector: Selector, device="cuda", dialect: str = "protobufjs",
                hash_mask: Optional[int] = None) -> Extract:
    """The same :class:`Extract` as :func:`extract_cpu`, computed on ``device``: the host indexes the
    frame headers, the device evaluates the selector per frame, compacts and gathers the kept bytes
    (``ops/gpu_extract.py``). ``data`` must be below 2^31 bytes (:func:`extract_file` cuts chunks).
    Raises if the HIP library or the device is missing."""
    from .ops import gpu_extract
    replay._check_dialect(dialect)
    return gpu_extract.extract(data, selector, device=device, dialect=dialect, hash_mask=hash_mask)[0]


def extract_file(path, out, selector: Selector, device: str = "cpu", dialect: str = "protobufjs",
                 chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES, indices_out=None) -> dict:
    """Extract the file at ``path`` (or an open binary file) chunk by chunk into the binary file
    ``out``: each chunk is cut at a frame boundary (``replay.iter_chunks``) and its kept bytes are
    written before the next is read, so memory stays at the chunk size and a stream that ends inside
    a frame leaves whole frames only. ``device`` is ``cpu`` or a torch device string (``gpu`` means
    ``cuda``). ``indices_out``, a text file, gets the kept input indices, one per line.
    Returns ``{frames, kept, kept_bytes, host_frames}``; ``host_frames`` counts the frames a device
    run left to the host."""
    replay._check_dialect(dialect)

    def on_device(device):
        from .ops import gpu_extract
        return lambda chunk: gpu_extract.extract(chunk, selector, device=device, dialect=dialect)
    cut = capture_io.per_chunk(device, lambda chunk: extract_cpu(chunk, selector, dialect), on_device)
    counts = {"frames": 0, "kept": 0, "kept_bytes": 0, "host_frames": 0}
    with capture_io.open_source(path) as f:
        for _, part, host_frames in capture_io.chunk_parts(f, chunk_bytes, replay.iter_chunks, cut):
            out.write(part.data)
            if indices_out is not None and part.indices:  # no write call for a part that keeps nothing
                capture_io.write_indices(indices_out, part.indices, counts["frames"])
            counts["frames"] += part.frames
            counts["kept"] += len(part.indices)
            counts["kept_bytes"] += len(part.data)
            counts["host_frames"] += host_frames
    return counts
