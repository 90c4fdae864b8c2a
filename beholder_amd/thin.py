"""Drop the progress events that repeat their media's step; the result is a framed stream again.

Progress events are the bulk of any real capture, and on replay each one for a Trello-created media
is one Trello comment (``handlers.py`` ``on_progress``) against a budget of 100 requests per 10 s.
``coalesce --progress all`` keeps every one of them, ``--progress per-status`` keeps one per stage
and loses the whole course. ``thin`` sits in between: a media's progress history stays, but only
where it moves by a step the operator chooses (10 % by default). Whether a frame is kept depends on
its media's neighbouring progress event in stream order, so this is the order machinery of
``transitions`` with the output of ``coalesce`` and ``dedupe``. :func:`thin_cpu` is the definition;
:func:`thin_gpu` computes the same :class:`Thinned` on the device (``ops/hip/telemetry_thin.hip``,
``ops/gpu_thin.py``).

Frames are read as the fold and ``coalesce`` read them: frame ``i`` is event ``i``, the dialect is
the service's (``protobufjs`` by default), and a ``mediaId`` is the decoded string (U+FFFD for
invalid UTF-8 under protobufjs, ``""`` for an absent field). A topic-2 frame that decodes as
``api.TelemetryProgress`` is a **progress event** with a ``status`` (the raw int32) and a
``progress`` (int32). Every other frame takes no part and is kept as it is: status frames, other
topics, and progress frames where the codec raises.

An event's **mark** is ``(status, progress // step)``, with Python's floor division (``-1 // 10 ==
-1``). The host, the field-4 string that the comment text also carries, is no part of the mark: a
change of host alone does not keep a frame.

For one media, let ``e_1 ... e_k`` be its progress events in stream order. Under ``keep="last"``
**``e_j`` is dropped iff ``j < k`` and ``mark(e_j) == mark(e_j+1)``**; under ``keep="first"`` iff
``j > 1`` and ``mark(e_j) == mark(e_j-1)``. Kept frames stay in stream order, byte for byte.

``last`` is the default for the reason it is ``dedupe``'s: it keeps every media's last progress
event, and the last event of every stage (``DOWNLOADING 100`` survives before ``CONVERTING 0``), so
coalescing the thinned stream gives what coalescing the input gives, and the fold's statuses stay.

Results merge: ``thin(a + b) == thin(a).merge(thin(b))`` for a cut at any frame boundary, which is
how :func:`thin_file` handles a file of any size in chunks. And thinning is idempotent.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Iterator, List, Optional, Tuple

from . import capture_io, ops, replay
from .capture_io import frame_spans
from .models import proto
from .topics import PROGRESS_ID

KEEP_MODES = ("last", "first")
STEP_MAX = 2 ** 31 - 1


@dataclasses.dataclass(frozen=True)
class Policy:
    """The width of a step in percentage points (``1 .. 2**31 - 1``), and which event of a stretch
    of equal marks survives (``last`` or ``first``)."""
    step: int = 10
    keep: str = "last"

    def __post_init__(self):
        if isinstance(self.step, bool) or not isinstance(self.step, int):
            raise TypeError(f"step is an int, not {type(self.step).__name__}")
        if not 1 <= self.step <= STEP_MAX:
            raise ValueError(f"step {self.step!r} is outside 1..{STEP_MAX}")
        if not isinstance(self.keep, str):
            raise TypeError(f"keep is a string, not {type(self.keep).__name__}")
        if self.keep not in KEEP_MODES:
            raise ValueError(f"unknown keep policy {self.keep!r} ({'|'.join(KEEP_MODES)})")


def _check_policy(policy) -> None:
    if not isinstance(policy, Policy):
        raise TypeError(f"policy is a thin.Policy, not {type(policy).__name__}")


def mark_of(policy: Policy = Policy(), dialect: str = "protobufjs") -> Callable[[int, bytes], Optional[tuple]]:
    """``mark(topic, body)`` for ``policy``: ``(mediaId, status, progress // step)`` for a progress
    event, ``None`` for every other frame. The host string is no part of it. The definition of what
    :func:`thin_cpu` compares, and what the device path asks about the frames it leaves to the host."""
    _check_policy(policy)
    replay._check_dialect(dialect)
    decode = ops.codec_for(replay._types()[1], dialect).decode
    step = policy.step

    def mark(topic: int, body: bytes):
        if topic != PROGRESS_ID:
            return None
        try:
            m = decode(body)
        except proto.DecodeError:
            return None
        return m.mediaId, m.status, m.progress // step
    return mark


def drops(events: List[tuple], keep: str) -> List[bool]:
    """The rule on one media's marks in stream order: per event, whether it is dropped."""
    k = len(events)
    if keep == "last":
        return [j + 1 < k and events[j] == events[j + 1] for j in range(k)]
    return [j > 0 and events[j] == events[j - 1] for j in range(k)]


@dataclasses.dataclass
class Thinned:
    data: bytes = b""            # the kept frames, headers included, in stream order
    indices: List[int] = dataclasses.field(default_factory=list)  # their indices in the input, ascending
    frames: int = 0              # the input's frame count
    step: int = 10
    keep: str = "last"
    dialect: str = "protobufjs"  # what the frames were read as: merge reads the kept ones again
    progress_events: int = 0     # the input's progress events, the dropped ones included

    def merge(self, later: "Thinned") -> "Thinned":
        """The result for this one's input followed by ``later``'s, from the two results alone.
        Under ``last`` only this one's last kept progress event per media can change its fate: it
        goes iff its mark is the mark of that media's first kept progress event in ``later``
        (dropped events share their successor's mark, so the first kept one carries the first
        one's). ``first`` is the mirror image. Neither operand changes."""
        if (later.step, later.keep, later.dialect) != (self.step, self.keep, self.dialect):
            raise ValueError(f"cannot merge step={self.step} keep={self.keep!r} dialect={self.dialect!r} with "
                             f"step={later.step} keep={later.keep!r} dialect={later.dialect!r}")
        mine, theirs = list(_marks(self, self.dialect)), list(_marks(later, self.dialect))
        edge_mine: Dict[str, Tuple[int, tuple]] = {}    # media -> (position, mark) of its last kept event here
        for p, (_, _, m) in enumerate(mine):
            if m is not None:
                edge_mine[m[0]] = (p, m)
        edge_theirs: Dict[str, Tuple[int, tuple]] = {}  # media -> the same of its first kept event in later
        for p, (_, _, m) in enumerate(theirs):
            if m is not None:
                edge_theirs.setdefault(m[0], (p, m))
        gone_mine, gone_theirs = set(), set()
        for mid, (p, m) in edge_mine.items():
            other = edge_theirs.get(mid)
            if other is not None and other[1] == m:
                (gone_mine if self.keep == "last" else gone_theirs).add(p if self.keep == "last" else other[0])
        kept = [(f, i) for p, (f, i, _) in enumerate(mine) if p not in gone_mine]
        kept += [(f, i + self.frames) for p, (f, i, _) in enumerate(theirs) if p not in gone_theirs]
        return Thinned(b"".join(f for f, _ in kept), [i for _, i in kept], self.frames + later.frames, self.step,
                       self.keep, self.dialect, self.progress_events + later.progress_events)


def _marks(part: Thinned, dialect: str) -> Iterator[Tuple[bytes, int, Optional[tuple]]]:
    """``(frame, index, mark)`` of every kept frame of ``part``; ``mark`` is None where the frame is
    no progress event."""
    mark = mark_of(Policy(part.step, part.keep), dialect)
    view = memoryview(part.data)
    for (a, b), i in zip(frame_spans(view), part.indices):
        frame = bytes(view[a:b])
        yield frame, i, mark(frame[4], frame[5:])


def thin_cpu(data, policy: Policy = Policy(), dialect: str = "protobufjs") -> Thinned:
    """The thinned stream, written plainly: the oracle and the ``--device cpu`` path. Raises
    ``ValueError`` for broken framing, as ``extract_cpu`` does."""
    mark = mark_of(policy, dialect)
    view = memoryview(data)
    spans = list(frame_spans(view))
    per_media: Dict[str, list] = {}  # media -> its (frame, mark) pairs in stream order
    events = 0
    for i, (a, b) in enumerate(spans):
        m = mark(view[a + 4], bytes(view[a + 5:b]))
        if m is not None:
            per_media.setdefault(m[0], []).append((i, m))
            events += 1
    dropped = set()
    for run in per_media.values():
        dropped.update(i for (i, _), gone in zip(run, drops([m for _, m in run], policy.keep)) if gone)
    kept = [i for i in range(len(spans)) if i not in dropped]
    return Thinned(b"".join(view[spans[i][0]:spans[i][1]] for i in kept), kept, len(spans), policy.step, policy.keep,
                   dialect, events)


def thin_gpu(data, policy: Policy = Policy(), device="cuda", dialect: str = "protobufjs",
             hash_mask: Optional[int] = None) -> Thinned:
    """The same :class:`Thinned` as :func:`thin_cpu`, computed on ``device``: the host indexes the
    frame headers; the device decodes the progress frames, groups them by ``mediaId``, sorts them
    stably by media, compares every event's mark with its neighbour's, compacts and gathers the kept
    bytes (``ops/gpu_thin.py``). ``data`` must be below 2^31 bytes (:func:`thin_file` cuts chunks).
    Raises if the HIP library or the device is missing."""
    from .ops import gpu_thin
    _check_policy(policy)
    replay._check_dialect(dialect)
    return gpu_thin.thin(data, policy, device=device, dialect=dialect, hash_mask=hash_mask)[0]


class _KeepLast:
    """The result so far of :func:`thin_file` under ``last``: the kept frames in stream order, a
    dropped one replaced by a tombstone, and per media the position and mark of its last kept
    progress event, the only one whose fate a later chunk can change."""

    def __init__(self):
        self.frames: List[Optional[bytes]] = []
        self.indices: List[int] = []
        self.edge: Dict[str, Tuple[int, tuple]] = {}

    def add(self, part: Thinned, base: int, dialect: str) -> None:
        frames, edge = self.frames, self.edge
        seen = set()  # the media that had an event in this part already
        for frame, i, m in _marks(part, dialect):
            if m is not None:
                old = edge.get(m[0])
                if old is not None and m[0] not in seen and old[1] == m:
                    frames[old[0]] = None
                seen.add(m[0])
                edge[m[0]] = (len(frames), m)
            frames.append(frame)
            self.indices.append(base + i)

    def live(self) -> Iterator[Tuple[bytes, int]]:
        return ((f, i) for f, i in zip(self.frames, self.indices) if f is not None)


def thin_file(path, out, policy: Policy = Policy(), device: str = "cpu", dialect: str = "protobufjs",
              chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES, indices_out=None) -> dict:
    """Thin the file at ``path`` (or an open binary file) chunk by chunk into the binary file
    ``out``: each chunk is cut at a frame boundary (``replay.iter_chunks``) and thinned on its own,
    and the chunks' results are joined on the host as :meth:`Thinned.merge` joins them.

    Under ``first`` each chunk's survivors are written before the next chunk is read, and the
    cross-chunk state is one mark per media; a stream that ends inside a frame leaves whole frames
    only, and then raises. Under ``last`` a media's last kept event may still go when the next
    chunk arrives, so the chunks are merged on the host and written once at the end, as
    ``coalesce_file`` does; a stream that ends inside a frame raises and writes nothing.

    A stream that fits in one chunk (the usual case at 256 MiB) has that chunk's result written as
    it is, and no per-frame host state is built: the kept frames are decoded again only when a
    second chunk arrives.

    ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``). ``indices_out``, a text
    file, gets the kept input indices, one per line.
    Returns ``{frames, kept, kept_bytes, progress_events, dropped, host_frames}``: ``progress_events``
    counts the input's, ``dropped`` is ``frames - kept``, ``host_frames`` counts the frames a device
    run left to the host."""
    _check_policy(policy)
    replay._check_dialect(dialect)

    def on_device(device):
        from .ops import gpu_thin
        return lambda chunk: gpu_thin.thin(chunk, policy, device=device, dialect=dialect)
    cut = capture_io.per_chunk(device, lambda chunk: thin_cpu(chunk, policy, dialect), on_device)
    counts = {"frames": 0, "kept": 0, "kept_bytes": 0, "progress_events": 0, "dropped": 0, "host_frames": 0}

    def write(data: bytes, indices) -> None:
        out.write(data)
        if indices_out is not None:
            capture_io.write_indices(indices_out, indices)
        counts["kept"] += len(indices)
        counts["kept_bytes"] += len(data)

    first = policy.keep == "first"
    held = None   # the first chunk's result, until a second chunk arrives or the stream ends
    state = None  # media -> mark under first, _KeepLast under last: built when a second chunk arrives
    with capture_io.open_source(path) as f:
        for _, part, host_frames in capture_io.chunk_parts(f, chunk_bytes, replay.iter_chunks, cut):
            base = counts["frames"]
            counts["frames"] += part.frames
            counts["progress_events"] += part.progress_events
            counts["host_frames"] += host_frames
            if base == 0:
                held = part
                if first:
                    write(part.data, part.indices)
                continue
            if first:
                if state is None:
                    state = {m[0]: m for _, _, m in _marks(held, dialect) if m is not None}
                    held = None
                parts, indices, seen = [], [], set()
                for frame, i, m in _marks(part, dialect):
                    if m is not None:
                        repeat = m[0] not in seen and state.get(m[0]) == m
                        seen.add(m[0])
                        state[m[0]] = m
                        if repeat:
                            continue
                    parts.append(frame)
                    indices.append(base + i)
                write(b"".join(parts), indices)
            else:
                if state is None:
                    state = _KeepLast()
                    state.add(held, 0, dialect)
                    held = None
                state.add(part, base, dialect)
    if not first:
        if state is not None:
            for frame, i in state.live():
                write(frame, (i,))
        elif held is not None:
            write(held.data, held.indices)
    counts["dropped"] = counts["frames"] - counts["kept"]
    return counts
