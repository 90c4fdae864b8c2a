"""Rewrite every decodable event of a framed stream as the service's own encoder would write it; the
result is a framed stream again.

Every other cut (``extract``, ``dedupe``, ``thin``, ``coalesce``, ``shard``) copies whole input frames
byte for byte. A capture that passed through two producers holds one event under several encodings
(an explicit ``status = 0``, another field order, an unknown field, an overlong varint), ``dedupe``
keeps every one of them, and the malformed-but-decodable bodies read differently in the two
dialects. ``normalise`` decodes each frame in the dialect it was captured under and encodes what it
decoded. :func:`normalise_cpu` is the definition; :func:`normalise_gpu` computes the same
:class:`Normalised` on the device (``ops/hip/telemetry_normalise.hip``, ``ops/gpu_normalise.py``).

Frames are read as the fold reads them: topic 1 decodes as ``api.TelemetryStatus`` and topic 2 as
``api.TelemetryProgress`` with ``ops.codec_for(type, dialect)``, and the new body is that codec's
``encode`` of what it decoded. A frame where the codec raises, or of another topic, is **undecoded**:
``Policy.undecoded`` keeps it as it is or drops it. Frames stay in stream order.

The canonical body, written out:

* fields are in ascending number, and each is omitted at its default;
* ``mediaId`` is ``0x0a``, varint(len), bytes;
* ``status`` is ``0x10``, then the varint of the int32 sign-extended to 64 bits, so a negative number
  takes 10 bytes;
* ``progress`` (progress messages only) is ``0x18``, written likewise;
* ``host`` (progress messages only) is ``0x22``, varint(len), bytes;
* fields 3 and 4 of a status message and every unknown field are gone;
* an all-default message is an empty body, so a frame of 5 bytes (``u32 1 | topic``).

A string is the decoded string: invalid UTF-8 under protobufjs comes back as U+FFFD (three bytes per
substitution), which is what every report calls that media anyway. So the output can be longer than
the input: a 5-byte varint of a negative int32 becomes 10 bytes, a substituted byte becomes three.

The laws (``tests/test_normalise.py``): normalising is idempotent; ``summarise``, ``transitions``,
``hosts`` and ``stages`` report the same for a stream and its normalised form in the same dialect;
the output reads the same in either dialect, and is a fixed point of the other dialect's normalise;
``dedupe`` after ``normalise`` keeps no more frames than ``dedupe`` alone. It never changes what the
service would do with a frame in that dialect.

Results merge by concatenation: every frame is decided on its own, which is how
:func:`normalise_file` handles a file of any size in chunks, each written before the next is read.
"""
from __future__ import annotations

import dataclasses
import struct
from typing import Callable, List

from . import capture_io, ops, replay
from .capture_io import frame_spans
from .coalesce import DROP, KEEP, UNDECODED_MODES
from .models import proto
from .topics import PROGRESS_ID, STATUS_ID


@dataclasses.dataclass(frozen=True)
class Policy:
    """What happens to the frames that are no decoded event (the codec raises, or another topic
    byte): ``keep`` leaves them as they are, ``drop`` removes them."""
    undecoded: str = "keep"

    def __post_init__(self):
        if not isinstance(self.undecoded, str):
            raise TypeError(f"undecoded is a string, not {type(self.undecoded).__name__}")
        if self.undecoded not in UNDECODED_MODES:
            raise ValueError(f"unknown undecoded policy {self.undecoded!r} ({'|'.join(UNDECODED_MODES)})")


def _check_policy(policy) -> None:
    if not isinstance(policy, Policy):
        raise TypeError(f"policy is a normalise.Policy, not {type(policy).__name__}")


def canon_of(policy: Policy = Policy(), dialect: str = "protobufjs") -> Callable[[int, bytes], object]:
    """``canon(topic, body)`` for ``policy``: ``KEEP`` (the frame stays as it is), ``DROP``, or the
    new body bytes of a decoded event. The definition of what :func:`normalise_cpu` writes, and what
    the device path asks about the frames it leaves to the host."""
    _check_policy(policy)
    replay._check_dialect(dialect)
    status_type, progress_type = replay._types()
    codecs = {STATUS_ID: ops.codec_for(status_type, dialect), PROGRESS_ID: ops.codec_for(progress_type, dialect)}
    undecoded = KEEP if policy.undecoded == "keep" else DROP

    def canon(topic: int, body: bytes):
        codec = codecs.get(topic)
        if codec is None:
            return undecoded
        try:
            m = codec.decode(body)
        except proto.DecodeError:
            return undecoded
        return bytes(codec.encode(m))
    return canon


def frame_of(topic: int, body: bytes) -> bytes:
    """``u32 L | u8 topic | body``, one frame of the stream."""
    return struct.pack("<IB", 1 + len(body), topic) + body


@dataclasses.dataclass
class Normalised:
    data: bytes = b""            # the output frames, headers included, in stream order
    indices: List[int] = dataclasses.field(default_factory=list)  # their indices in the input, ascending
    frames: int = 0              # the input's frame count
    events: int = 0              # the input's decoded events
    rewritten: int = 0           # the decoded events whose bytes changed
    dialect: str = "protobufjs"  # what the frames were read as
    undecoded: str = "keep"

    def merge(self, later: "Normalised") -> "Normalised":
        """The result for this one's input followed by ``later``'s: every frame is decided on its
        own, so this is concatenation with ``later``'s indices shifted. Neither operand changes."""
        if (later.dialect, later.undecoded) != (self.dialect, self.undecoded):
            raise ValueError(f"cannot merge dialect={self.dialect!r} undecoded={self.undecoded!r} with "
                             f"dialect={later.dialect!r} undecoded={later.undecoded!r}")
        return Normalised(self.data + later.data, self.indices + [i + self.frames for i in later.indices],
                          self.frames + later.frames, self.events + later.events, self.rewritten + later.rewritten,
                          self.dialect, self.undecoded)


def normalise_cpu(data, policy: Policy = Policy(), dialect: str = "protobufjs") -> Normalised:
    """The normalised stream, written plainly: the oracle and the ``--device cpu`` path. Raises
    ``ValueError`` for broken framing, as ``extract_cpu`` does."""
    canon = canon_of(policy, dialect)
    view = memoryview(data)
    spans = list(frame_spans(view))
    parts, indices = [], []
    events = rewritten = 0
    for i, (a, b) in enumerate(spans):
        topic = view[a + 4]
        body = bytes(view[a + 5:b])
        c = canon(topic, body)
        if c is DROP:
            continue
        if c is KEEP:
            parts.append(view[a:b])
        else:
            events += 1
            rewritten += c != body
            parts.append(frame_of(topic, c))
        indices.append(i)
    return Normalised(b"".join(parts), indices, len(spans), events, rewritten, dialect, policy.undecoded)


def normalise_gpu(data, policy: Policy = Policy(), device="cuda", dialect: str = "protobufjs") -> Normalised:
    """The same :class:`Normalised` as :func:`normalise_cpu`, computed on ``device``: the host indexes
    the frame headers; the device decodes every frame into a plan, sizes the canonical frames, scans
    the sizes and writes the output bytes (``ops/gpu_normalise.py``). ``data`` must leave room for its
    growth below 2^31 bytes (:func:`normalise_file` cuts chunks). Raises if the HIP library or the
    device is missing."""
    from .ops import gpu_normalise
    _check_policy(policy)
    replay._check_dialect(dialect)
    return gpu_normalise.normalise(data, policy, device=device, dialect=dialect)[0]


def normalise_file(path, out, policy: Policy = Policy(), device: str = "cpu", dialect: str = "protobufjs",
                   chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES, indices_out=None) -> dict:
    """Normalise the file at ``path`` (or an open binary file) chunk by chunk into the binary file
    ``out``: each chunk is cut at a frame boundary (``replay.iter_chunks``), normalised on its own and
    written before the next chunk is read, so memory stays at the chunk size. A stream that ends
    inside a frame leaves whole frames only, and then raises.

    ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``). ``indices_out``, a text
    file, gets the input indices of the output's frames, one per line.
    Returns ``{frames, kept, kept_bytes, in_bytes, events, rewritten, undecoded, host_frames}``:
    ``undecoded`` counts the input's frames that are no decoded event, ``host_frames`` the frames a
    device run left to the host."""
    _check_policy(policy)
    replay._check_dialect(dialect)

    def on_device(device):
        from .ops import gpu_normalise
        return capture_io.with_chunk_bytes_hint(gpu_normalise.TooLarge, lambda chunk: gpu_normalise.normalise(
            chunk, policy, device=device, dialect=dialect))
    cut = capture_io.per_chunk(device, lambda chunk: normalise_cpu(chunk, policy, dialect), on_device)
    counts = {"frames": 0, "kept": 0, "kept_bytes": 0, "in_bytes": 0, "events": 0, "rewritten": 0, "undecoded": 0,
              "host_frames": 0}
    with capture_io.open_source(path) as f:
        for chunk, part, host_frames in capture_io.chunk_parts(f, chunk_bytes, replay.iter_chunks, cut):
            out.write(part.data)
            if indices_out is not None:
                capture_io.write_indices(indices_out, part.indices, counts["frames"])
            counts["frames"] += part.frames
            counts["kept"] += len(part.indices)
            counts["kept_bytes"] += len(part.data)
            counts["in_bytes"] += len(chunk)
            counts["events"] += part.events
            counts["rewritten"] += part.rewritten
            counts["undecoded"] += part.frames - part.events
            counts["host_frames"] += host_frames
    return counts
