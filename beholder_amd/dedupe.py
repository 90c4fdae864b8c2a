"""Drop the byte-identical repeat frames of a framed stream; the result is a framed stream again.

Delivery is at least once, so a dead-letter file or a queue dump holds frames that are byte for byte
the same: a delivery that was never acked is dead-lettered twice, the files of ``--workers N`` get
concatenated, a dump is published twice. Replayed as they are, every repeat moves the card again and
posts the same comment again. ``coalesce`` would remove them, but only by cutting the whole history
down to one event per media and topic; ``extract`` cannot say it, because whether a frame is kept
depends on the other frames. :func:`dedupe_cpu` keeps every distinct event and drops only the exact
repeats, and is the definition; :func:`dedupe_gpu` computes the same :class:`Deduped` on the device
(``ops/hip/telemetry_dedupe.hip``, ``ops/gpu_dedupe.py``).

A frame's **content** is its topic byte and body: the bytes after the length header. Two frames are
equal iff their contents are equal bytes. Nothing is decoded, so there is no dialect, and two
encodings of one event are two contents (:mod:`beholder_amd.normalise`, run first, gives every event
one encoding). Under ``keep="last"`` **a frame is kept iff no later frame
has its content**; under ``keep="first"`` iff no earlier one has. With ``topics`` only frames of
those topic bytes take part; every other frame is kept as it is and equals nothing.

``last`` is the default because it is the one that is safe to replay. A media that goes ``QUEUED,
ERRORED, QUEUED`` has two equal status frames: ``first`` turns that into ``QUEUED, ERRORED`` and a
replay ends on the wrong status, ``last`` gives ``ERRORED, QUEUED``. The last frame of every
coalesce key is the last occurrence of its own content, so it survives ``last``: coalescing the
deduped stream gives what coalescing the input gives, and the fold ends on the same statuses.

Content cannot tell "the same event again" from "the same state reached again": two reports of one
progress percentage are equal frames and collapse too. That is why one capture is never subtracted
from another as a *set*: one such frame in B would erase both of A's. What is offered is the multiset
comparison of :mod:`beholder_amd.compare`, which pairs the k-th occurrence of a content in A with
the k-th in B, so two in A and one in B leave one "only in A", and which claims nothing about why.

Results merge: ``dedupe(a + b) == dedupe(a).merge(dedupe(b))`` for a cut at any frame boundary,
which is how :func:`dedupe_file` handles a file of any size in chunks. And deduping is idempotent.
"""
from __future__ import annotations

import dataclasses
from typing import FrozenSet, Iterator, List, Optional, Tuple

from . import capture_io, replay
from .capture_io import frame_spans

KEEP_MODES = ("last", "first")


@dataclasses.dataclass(frozen=True)
class Policy:
    """Which occurrence of a content survives (``last`` or ``first``), and the topic bytes whose
    frames take part (``None``: all of them)."""
    keep: str = "last"
    topics: Optional[FrozenSet[int]] = None

    def __post_init__(self):
        if not isinstance(self.keep, str):
            raise TypeError(f"keep is a string, not {type(self.keep).__name__}")
        if self.keep not in KEEP_MODES:
            raise ValueError(f"unknown keep policy {self.keep!r} ({'|'.join(KEEP_MODES)})")
        if self.topics is None:
            return
        if isinstance(self.topics, (str, bytes)) or not hasattr(self.topics, "__iter__"):
            raise TypeError(f"topics is a set of topic bytes, not {type(self.topics).__name__}")
        topics = frozenset(self.topics)
        for t in topics:
            if not isinstance(t, int) or isinstance(t, bool):
                raise TypeError(f"a topic is an int, not {type(t).__name__}")
            if not 0 <= t <= 255:
                raise ValueError(f"topic {t!r} is no byte (0-255)")
        object.__setattr__(self, "topics", topics)

    def takes_part(self, topic: int) -> bool:
        return self.topics is None or topic in self.topics


def _check_policy(policy) -> None:
    if not isinstance(policy, Policy):
        raise TypeError(f"policy is a dedupe.Policy, not {type(policy).__name__}")


@dataclasses.dataclass
class Deduped:
    data: bytes = b""            # the kept frames, headers included, in stream order
    indices: List[int] = dataclasses.field(default_factory=list)  # their indices in the input, ascending
    frames: int = 0              # the input's frame count
    keep: str = "last"
    topics: Optional[FrozenSet[int]] = None  # the policy's: a kept frame takes part iff its topic byte is among them
    # per kept frame a 64-bit number that equal contents share (the device's hash, as the uint64 array it
    # came back in; see dedupe_file), or None. It only pre-filters and is no part of the result.
    hashes: Optional[object] = dataclasses.field(default=None, compare=False, repr=False)

    def merge(self, later: "Deduped") -> "Deduped":
        """The result for this one's input followed by ``later``'s, from the two results alone. Under
        ``last`` a frame of this one goes where its content is among ``later``'s kept frames that
        take part; under ``first`` a frame of ``later`` goes where its content is among this one's.
        Neither operand changes."""
        if later.keep != self.keep or later.topics != self.topics:
            raise ValueError(f"cannot merge keep={self.keep!r} topics={_names(self.topics)} with "
                             f"keep={later.keep!r} topics={_names(later.topics)}")
        policy = Policy(self.keep, self.topics)
        loser, other = (self, later) if self.keep == "last" else (later, self)
        view = memoryview(other.data)
        taken = {bytes(view[a:b]) for a, b in frame_spans(view) if policy.takes_part(view[a + 4])}
        view = memoryview(loser.data)
        parts, indices = [], []
        for (a, b), i in zip(frame_spans(view), loser.indices):
            if not policy.takes_part(view[a + 4]) or bytes(view[a:b]) not in taken:
                parts.append(view[a:b])
                indices.append(i)
        cut = b"".join(parts)
        frames = self.frames + later.frames
        if loser is self:
            return Deduped(cut + later.data, indices + [i + self.frames for i in later.indices], frames,
                           self.keep, self.topics)
        return Deduped(self.data + cut, self.indices + [i + self.frames for i in indices], frames,
                       self.keep, self.topics)


def _names(topics) -> str:
    return "all" if topics is None else "{" + ",".join(map(str, sorted(topics))) + "}"


def dedupe_cpu(data, policy: Policy = Policy()) -> Deduped:
    """The deduped stream, written plainly: the oracle and the ``--device cpu`` path. Raises
    ``ValueError`` for broken framing, as ``extract_cpu`` does."""
    _check_policy(policy)
    view = memoryview(data)
    spans = list(frame_spans(view))
    winner = {}  # content -> the frame that is kept for it
    for i, (a, b) in enumerate(spans):
        if policy.takes_part(view[a + 4]):
            content = bytes(view[a + 4:b])
            if policy.keep == "last":
                winner[content] = i
            else:
                winner.setdefault(content, i)
    kept = [i for i, (a, b) in enumerate(spans)
            if not policy.takes_part(view[a + 4]) or winner[bytes(view[a + 4:b])] == i]
    return Deduped(b"".join(view[spans[i][0]:spans[i][1]] for i in kept), kept, len(spans), policy.keep, policy.topics)


def dedupe_gpu(data, policy: Policy = Policy(), device="cuda", hash_mask: Optional[int] = None) -> Deduped:
    """The same :class:`Deduped` as :func:`dedupe_cpu`, computed on ``device``: the host indexes the
    frame headers, the device hashes every frame's content, groups equal contents in a table whose
    key compare walks the bytes, marks each group's first or last frame, compacts and gathers the
    kept bytes (``ops/gpu_dedupe.py``). ``data`` must be below 2^31 bytes (:func:`dedupe_file` cuts
    chunks). Raises if the HIP library or the device is missing."""
    from .ops import gpu_dedupe
    return gpu_dedupe.dedupe(data, policy, device=device, hash_mask=hash_mask)[0]


def _kept(part: Deduped, policy: Policy) -> Iterator[Tuple[bytes, int, Optional[int]]]:
    """``(frame, index, number)`` of every kept frame of ``part``: ``number`` is None where the
    frame does not take part, else a number that equal contents share, the device's hash where
    ``part`` brought it and Python's own hash of the bytes where it did not."""
    view = memoryview(part.data)
    hashes = None if part.hashes is None else part.hashes.tolist()
    for k, ((a, b), i) in enumerate(zip(frame_spans(view), part.indices)):
        frame = bytes(view[a:b])
        if not policy.takes_part(frame[4]):
            yield frame, i, None
        else:
            yield frame, i, (hash(frame) if hashes is None else hashes[k])


class _Seen:
    """The cross-chunk state of :func:`dedupe_file`: every distinct content that takes part, once,
    under a 64-bit number. The number only pre-filters: frames are equal iff their bytes are (the
    header is the content's length, so whole frames are compared). ``find`` gives what ``add``
    stored with the frame."""

    def __init__(self):
        self.by_number = {}  # number -> (frame, value), or a list of them where numbers collide

    def find(self, number: int, frame: bytes):
        entry = self.by_number.get(number)
        if entry is None:
            return None
        for f, value in (entry if isinstance(entry, list) else (entry,)):
            if f == frame:
                return value
        return None

    def add(self, number: int, frame: bytes, value) -> None:
        """Stores or replaces ``frame``'s value."""
        entry = self.by_number.get(number)
        if entry is None:
            self.by_number[number] = (frame, value)
            return
        entries = entry if isinstance(entry, list) else [entry]
        for k, (f, _) in enumerate(entries):
            if f == frame:
                entries[k] = (f, value)
                break
        else:
            entries.append((frame, value))
        self.by_number[number] = entries if len(entries) > 1 else entries[0]


class _KeepLast:
    """The result so far under ``last``: the kept frames in stream order, a superseded one replaced
    by a tombstone, and the position of every content in :class:`_Seen`. The lists are rebuilt when
    more than half of them is tombstones, as the coalesce's accumulator does."""

    def __init__(self, policy: Policy):
        self.policy = policy
        self.frames: List[Optional[bytes]] = []
        self.indices: List[int] = []
        self.numbers: List[Optional[int]] = []
        self.seen = _Seen()
        self.dead = 0

    def add(self, part: Deduped, base: int) -> None:
        frames, seen = self.frames, self.seen
        for frame, i, number in _kept(part, self.policy):
            if number is not None:
                old = seen.find(number, frame)
                if old is not None:
                    frame = frames[old]  # the one copy of this content
                    frames[old] = None
                    self.dead += 1
                seen.add(number, frame, len(frames))
            frames.append(frame)
            self.indices.append(base + i)
            self.numbers.append(number)
        if self.dead > 1024 and 2 * self.dead > len(frames):
            live = [p for p, f in enumerate(frames) if f is not None]
            self.frames = [frames[p] for p in live]
            self.indices = [self.indices[p] for p in live]
            self.numbers = [self.numbers[p] for p in live]
            self.seen = _Seen()
            for p, (f, number) in enumerate(zip(self.frames, self.numbers)):
                if number is not None:
                    self.seen.add(number, f, p)
            self.dead = 0

    def live(self) -> Iterator[Tuple[bytes, int]]:
        return ((f, i) for f, i in zip(self.frames, self.indices) if f is not None)


def dedupe_file(path, out, policy: Policy = Policy(), device: str = "cpu",
                chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES, indices_out=None) -> dict:
    """Dedupe the file at ``path`` (or an open binary file) chunk by chunk into the binary file
    ``out``: each chunk is cut at a frame boundary (``replay.iter_chunks``) and deduped on its own,
    and the chunks' results are joined on the host.

    Under ``last`` no frame's fate is known before the last chunk is in, so the output is written
    once at the end; a stream that ends inside a frame raises and writes nothing. Under ``first``
    each chunk's survivors are written before the next chunk is read, so a stream that ends inside
    a frame leaves whole frames only, and then raises.

    A stream that fits in one chunk (the usual case at 256 MiB) has that chunk's result written as
    it is, and no per-frame host state is built. When a second chunk arrives the cross-chunk state
    is built: **one copy of every distinct content that takes part**, for the whole run, under a
    64-bit number (the device's content hash, which comes back with each chunk's result, or
    Python's own hash of the bytes on the CPU path). The number only pre-filters; the bytes decide,
    so the result is exact. Under ``last`` the frames that do not take part are held until the end
    as well. So memory is the chunk plus the distinct contents, not the file; a capture of mostly
    distinct frames needs about its own size.

    ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``). ``indices_out``, a text
    file, gets the kept input indices, one per line.
    Returns ``{frames, kept, kept_bytes, duplicates, host_frames}``: ``duplicates`` is ``frames -
    kept``, ``host_frames`` counts the frames a device run left to the host."""
    _check_policy(policy)

    def on_device(device):
        from .ops import gpu_dedupe
        return lambda chunk: gpu_dedupe.dedupe(chunk, policy, device=device)
    cut = capture_io.per_chunk(device, lambda chunk: dedupe_cpu(chunk, policy), on_device)
    counts = {"frames": 0, "kept": 0, "kept_bytes": 0, "duplicates": 0, "host_frames": 0}

    def write(data: bytes, indices) -> None:
        out.write(data)
        if indices_out is not None:
            capture_io.write_indices(indices_out, indices)
        counts["kept"] += len(indices)
        counts["kept_bytes"] += len(data)

    first = policy.keep == "first"
    held = None   # the first chunk's result, until a second chunk arrives or the stream ends
    state = None  # _Seen under first, _KeepLast under last: built when a second chunk arrives
    with capture_io.open_source(path) as f:
        for _, part, host_frames in capture_io.chunk_parts(f, chunk_bytes, replay.iter_chunks, cut):
            base = counts["frames"]
            counts["frames"] += part.frames
            counts["host_frames"] += host_frames
            if base == 0:
                held = part
                if first:
                    write(part.data, part.indices)
                continue
            if first:
                if state is None:
                    state = _Seen()
                    for frame, _, number in _kept(held, policy):
                        if number is not None:
                            state.add(number, frame, True)
                    held = None
                parts, indices = [], []
                for frame, i, number in _kept(part, policy):
                    if number is not None:
                        if state.find(number, frame):
                            continue
                        state.add(number, frame, True)
                    parts.append(frame)
                    indices.append(base + i)
                write(b"".join(parts), indices)
            else:
                if state is None:
                    state = _KeepLast(policy)
                    state.add(held, 0)
                    held = None
                state.add(part, base)
    if not first:
        if state is not None:
            for frame, i in state.live():
                write(frame, (i,))
        elif held is not None:
            write(held.data, held.indices)
    counts["duplicates"] = counts["frames"] - counts["kept"]
    return counts
