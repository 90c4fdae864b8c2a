"""How the media of a captured event stream *got* where they end: the status moves of every media.

``summarise`` says where a capture ends. Before a replay an operator also wants to know what the
replay will do on the way: the status handler moves a Trello card per status event, and on
``DEPLOYED`` posts to Telegram and refreshes Emby. How many card moves, between which lists? Are
there backwards moves (``DEPLOYED -> CONVERTING``, ``ERRORED -> QUEUED`` retries) or status events
after ``DEPLOYED``? Which media repeat one status over and over (a redelivery storm)? None of that
is in a :class:`~beholder_amd.replay.Summary`: it depends on the *order* of one media's status
events, and the fold keeps only the last of them. :func:`transitions_cpu` answers it, and is the
definition; :func:`transitions_gpu` computes the same :class:`Transitions` on the device
(``ops/hip/telemetry_transitions.hip``, ``ops/gpu_transitions.py``).

Frames are read as the fold reads them (:mod:`beholder_amd.replay`): frame ``i`` is event ``i``, the
dialect is the service's (``protobufjs`` by default), and a ``mediaId`` is the decoded string
(U+FFFD for invalid UTF-8 under protobufjs, ``""`` for an absent field). Only topic-1 frames
(``api.TelemetryStatus``) take part: where the codec raises, ``status_decode_errors += 1``; every
other one is a **status event**. Every other frame counts in ``frames`` only.

The **class** of a status number is the number itself where ``replay.status_names()`` names it, and
:data:`UNKNOWN` for every other int32: all unnamed numbers share that one class.

For one media, let ``s_1 ... s_k`` be the status numbers of its status events in stream order. The
**transition matrix** of the capture adds 1 to cell ``(class(s_j), class(s_j+1))`` for every
``j < k``. A transition whose two classes differ is a **change**, one on the diagonal a **repeat**.

Results merge: ``transitions(a + b) == transitions(a).merge(transitions(b))`` for a cut at any frame
boundary, which is how :func:`transitions_file` handles a file of any size in chunks.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Iterable, Iterator, Optional, Tuple

from . import capture_io, ops, replay
from .models import proto
from .topics import STATUS_ID
from .transport.framing import iter_frames

UNKNOWN = "unknown"  # the class of every status number that TelemetryStatusEntry does not name


def class_of(status: int, names: Optional[Dict[int, str]] = None):
    """``status`` itself where the enum names it, else :data:`UNKNOWN`."""
    return status if status in (replay.status_names() if names is None else names) else UNKNOWN


@dataclasses.dataclass
class MediaFlow:
    """The status events of one ``mediaId``: how many, how many of its transitions are changes, and
    its first and last one (the raw status number and the frame index)."""
    status_events: int = 0
    changes: int = 0
    first_status: Optional[int] = None
    first_index: Optional[int] = None
    last_status: Optional[int] = None
    last_index: Optional[int] = None


def flow_of(events: Iterable[Tuple[int, int]], names: Dict[int, str]) -> Tuple[MediaFlow, Dict[tuple, int]]:
    """The row and the matrix cells of one media from its ``(frame index, status)`` pairs in stream
    order (at least one)."""
    flow, cells = MediaFlow(), {}
    for i, status in events:
        if flow.status_events == 0:
            flow.first_status, flow.first_index = status, i
        else:
            cell = (class_of(flow.last_status, names), class_of(status, names))
            cells[cell] = cells.get(cell, 0) + 1
            flow.changes += cell[0] != cell[1]
        flow.status_events += 1
        flow.last_status, flow.last_index = status, i
    return flow, cells


def _class_name(cls, names: Dict[int, str]) -> str:
    return UNKNOWN if cls == UNKNOWN else names[cls]


@dataclasses.dataclass
class Transitions:
    frames: int = 0
    status_events: int = 0
    status_decode_errors: int = 0
    matrix: Dict[tuple, int] = dataclasses.field(default_factory=dict)    # (from class, to class) -> count, no zeros
    media: Dict[str, MediaFlow] = dataclasses.field(default_factory=dict)  # media with at least one status event

    @property
    def transitions(self) -> int:
        return sum(self.matrix.values())

    @property
    def changes(self) -> int:
        return sum(count for (a, b), count in self.matrix.items() if a != b)

    @property
    def repeats(self) -> int:
        return sum(count for (a, b), count in self.matrix.items() if a == b)

    def starts(self) -> Dict[object, int]:
        """Per class, the media whose first status event has it."""
        return self._ends("first_status")

    def ends(self) -> Dict[object, int]:
        """Per class, the media whose last status event has it."""
        return self._ends("last_status")

    def _ends(self, field: str) -> Dict[object, int]:
        names = replay.status_names()
        out: Dict[object, int] = {}
        for flow in self.media.values():
            cls = class_of(getattr(flow, field), names)
            out[cls] = out.get(cls, 0) + 1
        return out

    def add_cells(self, cells: Dict[tuple, int], sign: int = 1) -> None:
        """Add (or with ``sign`` -1 take out) ``cells``; a cell that reaches zero leaves the matrix."""
        matrix = self.matrix
        for cell, count in cells.items():
            value = matrix.get(cell, 0) + sign * count
            if value:
                matrix[cell] = value
            else:
                matrix.pop(cell, None)

    def merge(self, later: "Transitions") -> "Transitions":
        """The result of this stream followed by ``later``'s. Neither operand changes."""
        names = replay.status_names()
        out = Transitions(self.frames + later.frames, self.status_events + later.status_events,
                          self.status_decode_errors + later.status_decode_errors, dict(self.matrix),
                          {k: dataclasses.replace(v) for k, v in self.media.items()})
        out.add_cells(later.matrix)
        for mid, flow in later.media.items():
            flow = dataclasses.replace(flow, first_index=flow.first_index + self.frames,
                                       last_index=flow.last_index + self.frames)
            mine = out.media.get(mid)
            if mine is None:
                out.media[mid] = flow
                continue
            cell = (class_of(mine.last_status, names), class_of(flow.first_status, names))
            out.add_cells({cell: 1})
            mine.changes += flow.changes + (cell[0] != cell[1])
            mine.status_events += flow.status_events
            mine.last_status, mine.last_index = flow.last_status, flow.last_index
        return out

    def to_json(self, per_media: bool = False) -> dict:
        """Classes by their enum names (``unknown`` for the rest); ``transitions`` is from -> to ->
        count with sorted keys. The per-media rows, ``media``, only where ``per_media``."""
        names = replay.status_names()
        nested: Dict[str, Dict[str, int]] = {}
        for (a, b), count in self.matrix.items():
            nested.setdefault(_class_name(a, names), {})[_class_name(b, names)] = count

        def by_name(counts):
            named = {_class_name(c, names): v for c, v in counts.items()}
            return {k: named[k] for k in sorted(named)}
        out = {"frames": self.frames, "status_events": self.status_events,
               "status_decode_errors": self.status_decode_errors, "media_count": len(self.media),
               "changes": self.changes, "repeats": self.repeats,
               "transitions": {a: {b: nested[a][b] for b in sorted(nested[a])} for a in sorted(nested)},
               "starts": by_name(self.starts()), "ends": by_name(self.ends())}
        if per_media:
            out["media"] = {k: dataclasses.asdict(self.media[k]) for k in sorted(self.media)}
        return out

    @classmethod
    def from_json(cls, obj: dict) -> "Transitions":
        """The inverse of ``to_json(per_media=True)``; an object without the per-media rows does not
        hold a whole result and raises ``ValueError``."""
        if "media" not in obj:
            raise ValueError("the object has no per-media rows (to_json(per_media=True) writes them)")
        numbers = {name: number for number, name in replay.status_names().items()}

        def number(name: str):
            if name == UNKNOWN:
                return UNKNOWN
            if name not in numbers:
                raise ValueError(f"unknown status class {name!r}")
            return numbers[name]
        matrix = {(number(a), number(b)): int(count) for a, row in obj["transitions"].items() for b, count in row.items()}
        return cls(int(obj["frames"]), int(obj["status_events"]), int(obj["status_decode_errors"]), matrix,
                   {k: MediaFlow(**v) for k, v in obj["media"].items()})


def status_events_of(events: Iterable[Tuple[int, int, bytes]], dialect: str = "protobufjs"):
    """``(per media its (index, status) pairs in the order given, decode errors)`` of ``(index, topic,
    body)`` triples, decoded with the service's codec; frames of other topics are passed over."""
    replay._check_dialect(dialect)
    decode = ops.codec_for(proto.load("api.TelemetryStatus"), dialect).decode
    per_media: Dict[str, list] = {}
    errors = 0
    for i, topic, body in events:
        if topic != STATUS_ID:
            continue
        try:
            m = decode(body)
        except proto.DecodeError:
            errors += 1
            continue
        per_media.setdefault(m.mediaId, []).append((i, m.status))
    return per_media, errors


def transitions_events(events: Iterable[Tuple[int, int, bytes]], dialect: str = "protobufjs") -> Transitions:
    """The definition, over ``(index, topic, body)`` triples in stream order. ``frames`` is left to
    the caller."""
    per_media, errors = status_events_of(events, dialect)
    names = replay.status_names()
    t = Transitions(status_decode_errors=errors)
    for mid, pairs in per_media.items():
        flow, cells = flow_of(pairs, names)
        t.media[mid] = flow
        t.status_events += flow.status_events
        t.add_cells(cells)
    return t


def transitions_cpu(data, dialect: str = "protobufjs") -> Transitions:
    """The transitions of a framed stream, written plainly: the oracle and the ``--device cpu``
    path. Raises ``ValueError`` for broken framing, as ``extract_cpu`` does."""
    frames = 0

    def events() -> Iterator[Tuple[int, int, bytes]]:
        nonlocal frames
        for i, (topic, body) in enumerate(iter_frames(data)):
            frames = i + 1
            yield i, topic, body
    t = transitions_events(events(), dialect)
    t.frames = frames
    return t


def transitions_gpu(data, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None) -> Transitions:
    """The same :class:`Transitions` as :func:`transitions_cpu`, computed on ``device``: the host
    indexes the frame headers; the device decodes, groups the status events by ``mediaId``, sorts
    them stably by media and counts the moves between neighbours (``ops/gpu_transitions.py``). Only
    the matrix, the counters and one row per media come back. ``data`` must be below 2^31 bytes
    (:func:`transitions_file` cuts chunks). Raises if the HIP library or the device is missing."""
    from .ops import gpu_transitions
    replay._check_dialect(dialect)
    return gpu_transitions.transitions(data, device=device, dialect=dialect, hash_mask=hash_mask)[0]


def transitions_file(path, device: str = "cpu", dialect: str = "protobufjs",
                     chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES) -> Tuple[Transitions, int]:
    """The transitions of the file at ``path`` (or an open binary file) chunk by chunk, each chunk cut
    at a frame boundary (``replay.iter_chunks``), merged on the host as ``fold_file`` does. ``device``
    is ``cpu`` or a torch device string (``gpu`` means ``cuda``). Returns ``(Transitions,
    host_frames)``: the frames that a device run left to the host."""
    replay._check_dialect(dialect)

    def on_device(device):
        from .ops import gpu_transitions
        return lambda chunk: gpu_transitions.transitions(chunk, device=device, dialect=dialect)
    cut = capture_io.per_chunk(device, lambda chunk: transitions_cpu(chunk, dialect), on_device)
    return replay.merge_chunks(path, chunk_bytes, Transitions(), cut)
