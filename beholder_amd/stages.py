"""Both topics of a captured event stream joined per media: what stage every media is in and how far,
which progress events would land under another list, and which stages were cut short.

The offline tools split a capture by topic: ``transitions`` reads the status events, ``thin`` and
``hosts`` the progress events, ``summarise`` keeps the end state and drops the order. The service is
where the two queues meet: a status event moves the Trello card to a list, a progress event comments
``CONVERTING 40%`` under whatever list the card is in at that moment. When a capture comes back from
a dead-letter queue the operator asks about exactly that meeting: which media are stuck, in which
stage, at what percent; how many progress events a replay would post under a card that is in another
list, or whose list the capture never set; how many stages ended before they reached 100. The answer
for a progress event depends on the latest earlier status event of the same media.
:func:`stages_cpu` answers it, and is the definition; :func:`stages_gpu` computes the same
:class:`StageReport` on the device (``ops/hip/telemetry_stages.hip``, ``ops/gpu_stages.py``).

Frames are read as ``transitions`` reads topic 1 and as ``thin`` reads topic 2: frame ``i`` is event
``i``, the dialect is the service's (``protobufjs`` by default), a ``mediaId`` is the decoded string
(``""`` for an absent field, U+FFFD for invalid UTF-8 under protobufjs), and the worker string takes
no part. A topic-1 frame that decodes as ``api.TelemetryStatus`` is a **status event** ``(mediaId,
status)``; a topic-2 frame that decodes as ``api.TelemetryProgress`` is a **progress event**
``(mediaId, status, progress)``. Where the codec raises, ``status_decode_errors`` or
``progress_decode_errors`` goes up by one. Every other frame counts in ``frames`` only.

The **class** of a status number is the transitions' (:func:`beholder_amd.transitions.class_of`): the
number itself where the enum names it, :data:`UNKNOWN` for every other int32.

For one media, take its events of both topics in stream order.

* The **standing status** of a progress event is the status of the latest status event of its media
  before it in the stream. A progress event with none is a **lead** event.
* A **stage** is one status event and the progress events that follow it up to the media's next
  status event. Its class is the class of that status, its ``count`` the number of those progress
  events, its ``last`` the progress of the last of them.
* A stage is **closed** if a later status event of its media ends it, and **open** if it is the
  media's last: every media with at least one status event has exactly one open stage.
* The media's **lead** is its progress events before its first status event (it may be empty): per
  media ``{reported class: count}`` and the progress of the last of them.
* A stage's **bucket** (:func:`bucket_of`, one of the 14 :data:`BUCKETS`) is ``none`` where ``count ==
  0``, ``below`` where ``last < 0``, ``"0"`` to ``"9"`` for ``last // 10`` where ``0 <= last < 100``,
  ``full`` where ``last == 100`` and ``over`` where ``last > 100``.

``matrix[(standing class, reported class)]`` counts the progress events that have a standing status:
its diagonal is ``agree``, the rest ``disagree``, the comments a replay posts under a card that sits
in another list than the one the worker reported.

Results merge: ``stages(a + b) == stages(a).merge(stages(b))`` for a cut at any frame boundary, which
is how :func:`stages_file` handles a file of any size in chunks. For a media in both operands ``b``'s
lead joins ``a``'s open stage (its count and last are updated, and every lead event moves into
``matrix[class of a's standing][reported class]``), or ``a``'s lead where ``a`` has no open stage;
then, if ``b`` has a status event of that media, ``a``'s stage as just updated becomes a closed stage
and ``b``'s open stage is the media's.

The laws the tests hold it to: ``sum(entered) == status_events ==`` closed stages + open stages;
``sum(matrix) + lead_events == progress_events``; the counts of all stages plus the lead events equal
``progress_events`` (the closed stages' counts are not stored: the tests take them from
:func:`course_of`); and each media's events equal its lead, its stage counts and its status events.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Iterable, Iterator, List, Optional, Tuple

from . import capture_io, ops, replay
from .models import proto
from .topics import PROGRESS_ID, STATUS_ID
from .transitions import UNKNOWN, _class_name, class_of
from .transport.framing import iter_frames

STATUS, PROGRESS = 1, 2  # the kind of an event: its topic
Event = Tuple[int, int, int, int]  # (frame index, kind, status, progress); a status event's progress is 0
Open = Tuple[int, int, int, Optional[int]]  # (frame index of the status event, raw status, count, last)

BUCKETS = ("none", "below") + tuple(str(k) for k in range(10)) + ("full", "over")


def bucket_of(count: int, last: Optional[int]) -> str:
    """The bucket of a stage of ``count`` progress events whose last reported ``last``."""
    if count == 0:
        return "none"
    if last < 0:
        return "below"
    if last < 100:
        return str(last // 10)
    return "full" if last == 100 else "over"


def _bump(counts: dict, key, by: int = 1) -> None:
    value = counts.get(key, 0) + by
    if value:
        counts[key] = value
    else:
        counts.pop(key, None)


@dataclasses.dataclass
class MediaStand:
    """One ``mediaId``: its lead as ``{reported class: count}`` with the progress of its last lead
    event, the number of its events of both topics, and its open stage (``None`` where it has no
    status event)."""
    lead: Dict[object, int] = dataclasses.field(default_factory=dict)  # no zeros
    lead_last: Optional[int] = None
    events: int = 0
    open: Optional[Open] = None

    @property
    def lead_count(self) -> int:
        return sum(self.lead.values())

    def copy(self) -> "MediaStand":
        return dataclasses.replace(self, lead=dict(self.lead))


@dataclasses.dataclass
class Course:
    """What one media adds to a report: its row and its cells of the three tables. ``stages`` lists
    every stage in order as ``(class, count, last, closed)``."""
    stand: MediaStand
    entered: Dict[object, int]
    matrix: Dict[tuple, int]
    closed: Dict[tuple, int]
    stages: List[tuple]


def course_of(events: Iterable[Event], names: Optional[Dict[int, str]] = None) -> Course:
    """The rule on one media's ``(frame index, kind, status, progress)`` events in stream order (at
    least one)."""
    names = replay.status_names() if names is None else names
    stand, entered, matrix, closed, stages = MediaStand(), {}, {}, {}, []
    for index, kind, status, progress in events:
        cls = class_of(status, names)
        stand.events += 1
        if kind == STATUS:
            _bump(entered, cls)
            if stand.open is not None:
                _, before, count, last = stand.open
                _bump(closed, (class_of(before, names), bucket_of(count, last)))
                stages.append((class_of(before, names), count, last, True))
            stand.open = (index, status, 0, None)
        elif stand.open is None:
            _bump(stand.lead, cls)
            stand.lead_last = progress
        else:
            at, standing, count, _ = stand.open
            _bump(matrix, (class_of(standing, names), cls))
            stand.open = (at, standing, count + 1, progress)
    if stand.open is not None:
        stages.append((class_of(stand.open[1], names), stand.open[2], stand.open[3], False))
    return Course(stand, entered, matrix, closed, stages)


@dataclasses.dataclass
class StageReport:
    frames: int = 0
    status_events: int = 0
    progress_events: int = 0
    status_decode_errors: int = 0
    progress_decode_errors: int = 0
    entered: Dict[object, int] = dataclasses.field(default_factory=dict)  # class -> status events, no zeros
    matrix: Dict[tuple, int] = dataclasses.field(default_factory=dict)    # (standing class, reported class), no zeros
    closed: Dict[tuple, int] = dataclasses.field(default_factory=dict)    # (class, bucket) -> closed stages, no zeros
    media: Dict[str, MediaStand] = dataclasses.field(default_factory=dict)  # media with at least one event

    @property
    def open(self) -> Dict[tuple, int]:
        """``(class, bucket)`` -> the media whose open stage is there."""
        names = replay.status_names()
        out: Dict[tuple, int] = {}
        for stand in self.media.values():
            if stand.open is not None:
                _bump(out, (class_of(stand.open[1], names), bucket_of(stand.open[2], stand.open[3])))
        return out

    @property
    def lead_events(self) -> int:
        return sum(stand.lead_count for stand in self.media.values())

    @property
    def agree(self) -> int:
        return sum(count for (a, b), count in self.matrix.items() if a == b)

    @property
    def disagree(self) -> int:
        return sum(count for (a, b), count in self.matrix.items() if a != b)

    def stuck(self, cls, below: int = 100) -> List[str]:
        """The media whose open stage has class ``cls`` and no progress event, or a last progress
        under ``below``, in sorted order."""
        names = replay.status_names()
        return sorted(mid for mid, stand in self.media.items()
                      if stand.open is not None and class_of(stand.open[1], names) == cls
                      and (stand.open[2] == 0 or stand.open[3] < below))

    def add_course(self, mid: str, course: Course, sign: int = 1) -> None:
        """Add one media's :func:`course_of` (or with ``sign`` -1 take it out again: the media's row
        leaves). A cell that reaches zero leaves its table."""
        for table, cells in ((self.entered, course.entered), (self.matrix, course.matrix), (self.closed, course.closed)):
            for cell, count in cells.items():
                _bump(table, cell, sign * count)
        statuses = sum(course.entered.values())
        self.status_events += sign * statuses
        self.progress_events += sign * (course.stand.events - statuses)
        if sign > 0:
            self.media[mid] = course.stand
        else:
            self.media.pop(mid, None)

    def merge(self, later: "StageReport") -> "StageReport":
        """The result of this stream followed by ``later``'s, from the two results alone. Neither
        operand changes."""
        names = replay.status_names()
        out = StageReport(self.frames + later.frames, self.status_events + later.status_events,
                          self.progress_events + later.progress_events,
                          self.status_decode_errors + later.status_decode_errors,
                          self.progress_decode_errors + later.progress_decode_errors, dict(self.entered),
                          dict(self.matrix), dict(self.closed), {k: v.copy() for k, v in self.media.items()})
        for table, cells in ((out.entered, later.entered), (out.matrix, later.matrix), (out.closed, later.closed)):
            for cell, count in cells.items():
                _bump(table, cell, count)
        shift = self.frames
        for mid, theirs in later.media.items():
            theirs = theirs.copy()
            if theirs.open is not None:
                theirs.open = (theirs.open[0] + shift,) + tuple(theirs.open[1:])
            mine = out.media.get(mid)
            if mine is None:
                out.media[mid] = theirs
                continue
            mine.events += theirs.events
            if theirs.lead:
                if mine.open is None:  # a lead joins a lead
                    for cls, count in theirs.lead.items():
                        _bump(mine.lead, cls, count)
                    mine.lead_last = theirs.lead_last
                else:                  # a lead joins an open stage
                    at, standing, count, _ = mine.open
                    for cls, events in theirs.lead.items():
                        _bump(out.matrix, (class_of(standing, names), cls), events)
                    mine.open = (at, standing, count + theirs.lead_count, theirs.lead_last)
            if theirs.open is not None:
                if mine.open is not None:  # the later operand closes the stage
                    _bump(out.closed, (class_of(mine.open[1], names), bucket_of(mine.open[2], mine.open[3])))
                mine.open = theirs.open
        return out

    def to_json(self, per_media: bool = False) -> dict:
        """Classes by their enum names (``unknown`` for the rest) in sorted order, buckets in the
        order of :data:`BUCKETS`; ``matrix`` is standing -> reported -> count. The per-media rows,
        ``media``, only where ``per_media``."""
        names = replay.status_names()

        def by_name(counts):
            named = {_class_name(c, names): v for c, v in counts.items()}
            return {k: named[k] for k in sorted(named)}

        def nested(cells, inner_order=None):
            rows: Dict[str, Dict[str, int]] = {}
            for (a, b), count in cells.items():
                rows.setdefault(_class_name(a, names), {})[b if inner_order else _class_name(b, names)] = count
            return {a: {b: rows[a][b] for b in (inner_order or sorted(rows[a])) if b in rows[a]} for a in sorted(rows)}
        out = {"frames": self.frames, "status_events": self.status_events, "progress_events": self.progress_events,
               "status_decode_errors": self.status_decode_errors,
               "progress_decode_errors": self.progress_decode_errors, "media_count": len(self.media),
               "lead_events": self.lead_events, "agree": self.agree, "disagree": self.disagree,
               "entered": by_name(self.entered), "matrix": nested(self.matrix),
               "closed": nested(self.closed, BUCKETS), "open": nested(self.open, BUCKETS)}
        if per_media:
            out["media"] = {mid: {"events": s.events, "lead": by_name(s.lead), "lead_last": s.lead_last,
                                  "open": None if s.open is None else list(s.open)}
                            for mid, s in ((mid, self.media[mid]) for mid in sorted(self.media))}
        return out

    @classmethod
    def from_json(cls, obj: dict) -> "StageReport":
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

        def bucket(name: str) -> str:
            if name not in BUCKETS:
                raise ValueError(f"unknown bucket {name!r}")
            return name

        def stage(o) -> Optional[Open]:
            return None if o is None else (int(o[0]), int(o[1]), int(o[2]), None if o[3] is None else int(o[3]))
        media = {mid: MediaStand({number(k): int(v) for k, v in row["lead"].items()},
                                 None if row["lead_last"] is None else int(row["lead_last"]), int(row["events"]),
                                 stage(row["open"])) for mid, row in obj["media"].items()}
        return cls(int(obj["frames"]), int(obj["status_events"]), int(obj["progress_events"]),
                   int(obj["status_decode_errors"]), int(obj["progress_decode_errors"]),
                   {number(k): int(v) for k, v in obj["entered"].items()},
                   {(number(a), number(b)): int(v) for a, row in obj["matrix"].items() for b, v in row.items()},
                   {(number(a), bucket(b)): int(v) for a, row in obj["closed"].items() for b, v in row.items()}, media)


def events_of(events: Iterable[Tuple[int, int, bytes]], dialect: str = "protobufjs"):
    """``(per media its (index, kind, status, progress) events in the order given, status decode
    errors, progress decode errors)`` of ``(index, topic, body)`` triples, decoded with the service's
    codecs; frames of other topics are passed over."""
    replay._check_dialect(dialect)
    status_type, progress_type = replay._types()
    decode_status = ops.codec_for(status_type, dialect).decode
    decode_progress = ops.codec_for(progress_type, dialect).decode
    per_media: Dict[str, List[Event]] = {}
    status_errors = progress_errors = 0
    for i, topic, body in events:
        if topic == STATUS_ID:
            try:
                m = decode_status(body)
            except proto.DecodeError:
                status_errors += 1
                continue
            per_media.setdefault(m.mediaId, []).append((i, STATUS, m.status, 0))
        elif topic == PROGRESS_ID:
            try:
                m = decode_progress(body)
            except proto.DecodeError:
                progress_errors += 1
                continue
            per_media.setdefault(m.mediaId, []).append((i, PROGRESS, m.status, m.progress))
    return per_media, status_errors, progress_errors


def stages_events(events: Iterable[Tuple[int, int, bytes]], dialect: str = "protobufjs") -> StageReport:
    """The definition, over ``(index, topic, body)`` triples in stream order. ``frames`` is left to
    the caller."""
    per_media, status_errors, progress_errors = events_of(events, dialect)
    names = replay.status_names()
    report = StageReport(status_decode_errors=status_errors, progress_decode_errors=progress_errors)
    for mid, run in per_media.items():
        report.add_course(mid, course_of(run, names))
    return report


def stages_cpu(data, dialect: str = "protobufjs") -> StageReport:
    """The stages of a framed stream, written plainly: the oracle and the ``--device cpu`` path.
    Raises ``ValueError`` for broken framing, as ``extract_cpu`` does."""
    frames = 0

    def events() -> Iterator[Tuple[int, int, bytes]]:
        nonlocal frames
        for i, (topic, body) in enumerate(iter_frames(data)):
            frames = i + 1
            yield i, topic, body
    report = stages_events(events(), dialect)
    report.frames = frames
    return report


def stages_gpu(data, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None) -> StageReport:
    """The same :class:`StageReport` as :func:`stages_cpu`, computed on ``device``: the host indexes
    the frame headers; the device decodes the frames of both topics, numbers the media, sorts the
    events stably by media, carries every media's latest status event along its run with a max-scan
    and settles every event against it (``ops/gpu_stages.py``). Only the three tables, one row per
    media and the lead events come back. ``data`` must be below 2^31 bytes (:func:`stages_file` cuts
    chunks). Raises if the HIP library or the device is missing."""
    from .ops import gpu_stages
    replay._check_dialect(dialect)
    return gpu_stages.stages(data, device=device, dialect=dialect, hash_mask=hash_mask)[0]


def stages_file(path, device: str = "cpu", dialect: str = "protobufjs",
                chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES) -> Tuple[StageReport, int]:
    """The stages of the file at ``path`` (or an open binary file) chunk by chunk, each chunk cut at a
    frame boundary (``replay.iter_chunks``), merged on the CPU as ``hosts_file`` does. ``device`` is
    ``cpu`` or a torch device string (``gpu`` means ``cuda``). Returns ``(StageReport, host_frames)``:
    the frames that a device run left to the CPU."""
    replay._check_dialect(dialect)

    def on_device(device):
        from .ops import gpu_stages
        return lambda chunk: gpu_stages.stages(chunk, device=device, dialect=dialect)
    cut = capture_io.per_chunk(device, lambda chunk: stages_cpu(chunk, dialect), on_device)
    return replay.merge_chunks(path, chunk_bytes, StageReport(), cut)
