"""Fold a captured event stream into its end state, without running the service over it.

A capture, a ``--dead-letter`` file or a queue dump is a framed stream (``u32 L | u8 topic | body``,
:mod:`beholder_amd.transport.framing`). Before replaying one, an operator wants to know what the
service will have done once it has gone through: which ``beholder_progress_updates_total{status}``
counts result, how many Trello comments are posted, which status each media row ends on, and how
many events fail to decode. :func:`fold_cpu` answers that, and is the definition; :func:`fold_gpu`
computes the same :class:`Summary` on the device (``ops/hip/telemetry_fold.hip``).

The fold (frame ``i`` of the stream is event ``i``; the dialect is the service's, ``protobufjs`` by
default as ``handlers._dialect``):

* topic 1 decodes as ``api.TelemetryStatus``. Where the codec raises, ``status_decode_errors += 1``.
  Otherwise, for that ``mediaId``: ``status_events += 1``, ``last_status = status`` and
  ``last_status_index = i`` (the frame with the highest ``i`` wins, which is what ``updateStatus``
  leaves behind, index.js:68). An unknown enum number is written all the same.
* topic 2 decodes as ``api.TelemetryProgress``. Where the codec raises,
  ``progress_decode_errors += 1``. Otherwise ``progress_events += 1`` for that ``mediaId``; if
  ``status`` is a number of ``TelemetryStatusEntry``, ``progress_updates[name.lower()] += 1`` and
  ``progress_counted += 1`` for the media (the counter the handler bumps before ``getByID``,
  index.js:136); if not, ``progress_unknown_status += 1`` (quirk Q6).
* any other topic byte: ``other_topic += 1``.

A ``mediaId`` is the decoded string, not the bytes: protobufjs turns invalid UTF-8 into U+FFFD, so
``b"\\xff"`` and ``b"\\xfe"`` are one media; an absent field is ``""``.

Summaries merge: ``fold(a + b) == fold(a).merge(fold(b))`` for a cut at any frame boundary, which is
how :func:`fold_file` handles a file of any size in chunks.
"""
from __future__ import annotations

import bisect
import dataclasses
from typing import Dict, Iterable, Iterator, Optional, Tuple

from . import capture_io, ops
from .models import proto
from .topics import PROGRESS_ID, STATUS_ID
from .transport.framing import iter_frames

TRELLO_CREATOR = 1  # handlers.TRELLO_CREATOR (index.js:79)
DEFAULT_CHUNK_BYTES = 256 << 20
MAX_CHUNK_BYTES = 2 ** 31 - 1  # a chunk is indexed with int32 offsets


@dataclasses.dataclass
class MediaFold:
    """What the stream does to one ``mediaId``."""
    status_events: int = 0
    progress_events: int = 0
    progress_counted: int = 0
    last_status: Optional[int] = None
    last_status_index: Optional[int] = None

    def absorb(self, other: "MediaFold", offset: int) -> None:
        """Add ``other``, whose frame indices start at ``offset`` of this one's stream."""
        self.status_events += other.status_events
        self.progress_events += other.progress_events
        self.progress_counted += other.progress_counted
        if other.last_status_index is not None:
            index = other.last_status_index + offset
            if self.last_status_index is None or index > self.last_status_index:
                self.last_status, self.last_status_index = other.last_status, index


@dataclasses.dataclass
class Summary:
    frames: int = 0
    status_decode_errors: int = 0
    progress_decode_errors: int = 0
    progress_unknown_status: int = 0
    other_topic: int = 0
    progress_updates: Dict[str, int] = dataclasses.field(default_factory=dict)
    media: Dict[str, MediaFold] = dataclasses.field(default_factory=dict)

    def merge(self, later: "Summary") -> "Summary":
        """The summary of this stream followed by ``later``'s. Neither operand changes."""
        out = Summary(self.frames + later.frames,
                      self.status_decode_errors + later.status_decode_errors,
                      self.progress_decode_errors + later.progress_decode_errors,
                      self.progress_unknown_status + later.progress_unknown_status,
                      self.other_topic + later.other_topic,
                      dict(self.progress_updates),
                      {k: dataclasses.replace(v) for k, v in self.media.items()})
        for name, count in later.progress_updates.items():
            out.progress_updates[name] = out.progress_updates.get(name, 0) + count
        for mid, fold in later.media.items():
            out.media.setdefault(mid, MediaFold()).absorb(fold, self.frames)
        return out

    def apply(self, media_rows: Iterable) -> dict:
        """The prediction for a run over ``media_rows`` (rows with ``id``, ``creator``, ``status``)
        with working sinks and store and default switches: the ``progress_updates`` counter values,
        the number of Trello comments, and the status each row ends on."""
        comments = 0
        statuses = {}
        for row in media_rows:
            fold = self.media.get(row.id)
            if fold is not None and row.creator == TRELLO_CREATOR:
                comments += fold.progress_counted
            statuses[row.id] = row.status if fold is None or fold.last_status_index is None else fold.last_status
        return {"progress_updates": dict(self.progress_updates), "trello_comments": comments, "statuses": statuses}

    def to_json(self) -> dict:
        out = {f.name: getattr(self, f.name) for f in dataclasses.fields(self) if f.name not in ("progress_updates", "media")}
        out["progress_updates"] = {k: self.progress_updates[k] for k in sorted(self.progress_updates)}
        out["media"] = {k: dataclasses.asdict(self.media[k]) for k in sorted(self.media)}
        return out

    @classmethod
    def from_json(cls, obj: dict) -> "Summary":
        scalars = {f.name: int(obj[f.name]) for f in dataclasses.fields(cls) if f.name not in ("progress_updates", "media")}
        return cls(progress_updates={k: int(v) for k, v in obj["progress_updates"].items()},
                   media={k: MediaFold(**v) for k, v in obj["media"].items()}, **scalars)


def _types():
    return proto.load("api.TelemetryStatus"), proto.load("api.TelemetryProgress")


def status_names() -> Dict[int, str]:
    """number -> name of ``TelemetryStatusEntry`` as the progress handler looks it up (index.js:134)."""
    return _types()[1].enum("TelemetryStatusEntry")[0]


def _check_dialect(dialect: str) -> None:
    if dialect not in ops.DIALECTS:
        raise ValueError(f"unknown dialect {dialect!r} ({'|'.join(ops.DIALECTS)})")


def fold_events(events: Iterable[Tuple[int, int, bytes]], dialect: str = "protobufjs",
                into: Optional[Summary] = None) -> Summary:
    """The definition, over ``(index, topic, body)`` triples. ``frames`` is left to the caller."""
    _check_dialect(dialect)
    status_type, progress_type = _types()
    decode_status = ops.codec_for(status_type, dialect).decode
    decode_progress = ops.codec_for(progress_type, dialect).decode
    names = status_names()
    s = Summary() if into is None else into
    media = s.media
    for i, topic, body in events:
        if topic == STATUS_ID:
            try:
                m = decode_status(body)
            except proto.DecodeError:
                s.status_decode_errors += 1
                continue
            fold = media.get(m.mediaId)
            if fold is None:
                fold = media[m.mediaId] = MediaFold()
            fold.status_events += 1
            if fold.last_status_index is None or i > fold.last_status_index:
                fold.last_status, fold.last_status_index = m.status, i
        elif topic == PROGRESS_ID:
            try:
                m = decode_progress(body)
            except proto.DecodeError:
                s.progress_decode_errors += 1
                continue
            fold = media.get(m.mediaId)
            if fold is None:
                fold = media[m.mediaId] = MediaFold()
            fold.progress_events += 1
            name = names.get(m.status)
            if name is None:
                s.progress_unknown_status += 1
            else:
                name = name.lower()
                s.progress_updates[name] = s.progress_updates.get(name, 0) + 1
                fold.progress_counted += 1
        else:
            s.other_topic += 1
    return s


def fold_cpu(data, dialect: str = "protobufjs") -> Summary:
    """The fold of a framed stream, written plainly: the oracle and the ``--device cpu`` path."""
    s = Summary()

    def events() -> Iterator[Tuple[int, int, bytes]]:
        for i, (topic, body) in enumerate(iter_frames(data)):
            s.frames = i + 1
            yield i, topic, body
    return fold_events(events(), dialect, into=s)


def fold_gpu(data, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None) -> Summary:
    """The same :class:`Summary` as :func:`fold_cpu`, computed on ``device``: the host indexes the
    frame headers, the device decodes, counts and groups (``ops/gpu_fold.py``), and only the
    counters and one row per distinct media come back. ``data`` must be below 2^31 bytes
    (:func:`fold_file` cuts chunks). Raises if the HIP library or the device is missing."""
    from .ops import gpu_fold
    _check_dialect(dialect)
    return gpu_fold.fold(data, device=device, dialect=dialect, hash_mask=hash_mask)[0]


def iter_chunks(f, chunk_bytes: int) -> Iterator[bytes]:
    """Cut the framed stream read from ``f`` at frame boundaries into pieces of at most
    ``chunk_bytes`` (a frame longer than that is a piece of its own). Raises ``ValueError`` for a
    stream that ends inside a frame, as ``iter_frames`` does."""
    if not 0 < chunk_bytes <= MAX_CHUNK_BYTES:
        raise ValueError(f"chunk_bytes must be in 1..{MAX_CHUNK_BYTES}")
    pending = bytearray()
    eof = False
    while True:
        cut = _cut(pending, chunk_bytes, eof)
        if cut:
            with memoryview(pending) as whole, whole[:cut] as head:
                chunk = bytes(head)
            del pending[:cut]
            yield chunk
            continue
        if eof:
            break
        block = f.read(chunk_bytes)
        eof = not block
        pending += block
    if pending:
        raise ValueError("truncated frame header" if len(pending) < 4 else "truncated or empty frame")


def _cut(pending: bytearray, limit: int, final: bool) -> int:
    """Where to cut ``pending``: the last frame boundary at or below ``limit``, or the end of the
    first frame where that one alone is longer; 0 to ask for more input first."""
    if not pending:
        return 0
    with memoryview(pending) as whole, whole[:MAX_CHUNK_BYTES] as view:
        n, offs = ops.native.frame_index(view, True)
    if n == 0:
        return 0
    with memoryview(offs) as raw, raw.cast("i") as starts:
        k = bisect.bisect_right(starts, limit) - 1  # starts[0] == 0, so k >= 0
        if k == 0:
            k = 1
        if k == n and starts[n] < limit and not final:
            return 0  # more frames may still fit
        return starts[k]


def fold_file(path, device: str = "cpu", dialect: str = "protobufjs",
              chunk_bytes: int = DEFAULT_CHUNK_BYTES) -> Summary:
    """Fold the file at ``path`` (or an open binary file) chunk by chunk, each chunk cut at a frame
    boundary and below 2^31 bytes, and merge the chunks' summaries on the host. ``device`` is
    ``cpu`` or a torch device string (``gpu`` means ``cuda``)."""
    _check_dialect(dialect)

    def on_device(device):
        return lambda chunk: (fold_gpu(chunk, device, dialect), 0)
    cut = capture_io.per_chunk(device, lambda chunk: fold_cpu(chunk, dialect), on_device)
    return merge_chunks(path, chunk_bytes, Summary(), cut)[0]


def merge_chunks(path, chunk_bytes: int, empty, cut) -> Tuple[object, int]:
    """What the report commands share: ``(empty merged with every chunk's part in turn, the host
    frames' sum)`` over the file at ``path`` (or an open binary file), cut by :func:`iter_chunks`;
    ``cut(chunk)`` gives ``(part, host_frames)``."""
    total, host_frames = empty, 0
    with capture_io.open_source(path) as f:
        for _, part, on_host in capture_io.chunk_parts(f, chunk_bytes, iter_chunks, cut):
            total = total.merge(part)
            host_frames += on_host
    return total, host_frames
