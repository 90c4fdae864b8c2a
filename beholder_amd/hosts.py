"""What every worker host did in a captured event stream: its events, its media, its stints, the
media it took over and lost, and what it held when the capture ended.

Every progress event carries the name of the worker that sent it (``api.TelemetryProgress.host``,
field 4), and the progress handler renders it into every Trello comment. When a capture comes back
from a dead-letter queue the operator asks which worker did what, which media changed hands (a
worker that loses many media and takes none is the one that died or was drained), and what each
worker was holding at the end, at which stage: the list to check before a replay re-posts
``CONVERTING 40% (worker-2)`` for jobs that worker-2 will never finish. :func:`hosts_cpu` answers it,
and is the definition; :func:`hosts_gpu` computes the same :class:`HostReport` on the device
(``ops/hip/telemetry_hosts.hip``, ``ops/gpu_hosts.py``).

Frames are read as ``thin`` reads them: frame ``i`` is event ``i``, the dialect is the service's
(``protobufjs`` by default). A topic-2 frame that decodes as ``api.TelemetryProgress`` is a
**progress event** ``(mediaId, host, status, progress)``; ``mediaId`` and ``host`` are the decoded
strings (``""`` for an absent field, U+FFFD for invalid UTF-8 under protobufjs, a decode error under
upb). Where the codec raises, ``progress_decode_errors += 1``. Every other frame counts in ``frames``
only.

For one media, let ``e_1 ... e_k`` be its progress events in stream order.

* A **stint** is a maximal run of neighbouring events with the same host.
* A **handover** is a neighbouring pair whose hosts differ: one ``lost`` for ``host(e_j)``, one
  ``taken`` for ``host(e_j+1)``.
* A **rewind** is a neighbouring pair with the same host and the same raw status where
  ``progress(e_j+1) < progress(e_j)``: a worker started a job over. It counts for that host.

The **class** of a status number is the transitions' (:func:`beholder_amd.transitions.class_of`): the
number itself where the enum names it, :data:`UNKNOWN` for every other int32.

Results merge: ``hosts(a + b) == hosts(a).merge(hosts(b))`` for a cut at any frame boundary, which is
how :func:`hosts_file` handles a file of any size in chunks. The laws the tests hold it to: the
events of the hosts, of the pairs and of the media each sum to ``progress_events``; ``taken`` and
``lost`` each sum to ``handovers``; the stints sum to ``media_count + handovers``; per host ``stints ==
starts + taken`` and ``media_of <= stints <= events``; the held media sum to ``media_count``.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Iterable, Iterator, List, Optional, Tuple

from . import capture_io, ops, replay
from .models import proto
from .topics import PROGRESS_ID
from .transitions import UNKNOWN, _class_name, class_of
from .transport.framing import iter_frames

Event = Tuple[int, str, int, int]  # (frame index, host, status, progress)


@dataclasses.dataclass
class HostRow:
    """One worker host: its progress events (in all and per status class), its stints, the handovers
    it took and lost, and its rewinds."""
    events: int = 0
    by_class: Dict[object, int] = dataclasses.field(default_factory=dict)  # no zeros
    stints: int = 0
    taken: int = 0
    lost: int = 0
    rewinds: int = 0

    def add(self, other: "HostRow", sign: int = 1) -> None:
        self.events += sign * other.events
        self.stints += sign * other.stints
        self.taken += sign * other.taken
        self.lost += sign * other.lost
        self.rewinds += sign * other.rewinds
        for cls, count in other.by_class.items():
            value = self.by_class.get(cls, 0) + sign * count
            if value:
                self.by_class[cls] = value
            else:
                self.by_class.pop(cls, None)

    def copy(self) -> "HostRow":
        return dataclasses.replace(self, by_class=dict(self.by_class))


@dataclasses.dataclass
class MediaEdge:
    """One ``mediaId``: how many progress events, and the first and the last of them as ``(frame
    index, host, status, progress)``."""
    events: int = 0
    first: Optional[Event] = None
    last: Optional[Event] = None


def course_of(events: Iterable[Event], names: Optional[Dict[int, str]] = None):
    """The rule on one media's ``(frame index, host, status, progress)`` events in stream order (at
    least one): ``(MediaEdge, {host: HostRow}, {host: events})``, what this media adds to the hosts
    and its pair counts."""
    names = replay.status_names() if names is None else names
    edge, rows, pairs = MediaEdge(), {}, {}
    for event in events:
        event = tuple(event)
        _, worker, status, progress = event
        row = rows.get(worker)
        if row is None:
            row = rows[worker] = HostRow()
        last = edge.last
        if last is None:
            edge.first = event
            row.stints += 1
        elif last[1] != worker:
            rows[last[1]].lost += 1
            row.taken += 1
            row.stints += 1
        elif last[2] == status and progress < last[3]:
            row.rewinds += 1
        cls = class_of(status, names)
        row.events += 1
        row.by_class[cls] = row.by_class.get(cls, 0) + 1
        pairs[worker] = pairs.get(worker, 0) + 1
        edge.events += 1
        edge.last = event
    return edge, rows, pairs


@dataclasses.dataclass
class HostReport:
    frames: int = 0
    progress_events: int = 0
    progress_decode_errors: int = 0
    hosts: Dict[str, HostRow] = dataclasses.field(default_factory=dict)         # hosts with at least one event
    pairs: Dict[Tuple[str, str], int] = dataclasses.field(default_factory=dict)  # (mediaId, host) -> events, no zeros
    media: Dict[str, MediaEdge] = dataclasses.field(default_factory=dict)       # media with at least one event

    @property
    def handovers(self) -> int:
        return sum(row.taken for row in self.hosts.values())

    @property
    def rewinds(self) -> int:
        return sum(row.rewinds for row in self.hosts.values())

    def media_of(self, host: str) -> int:
        """The media that ``host`` sent at least one event for: the pairs with that host."""
        return sum(1 for _, worker in self.pairs if worker == host)

    def holding(self) -> Dict[str, Dict[object, int]]:
        """Per host and status class, the media whose last event names the host."""
        names = replay.status_names()
        out: Dict[str, Dict[object, int]] = {}
        for edge in self.media.values():
            held = out.setdefault(edge.last[1], {})
            cls = class_of(edge.last[2], names)
            held[cls] = held.get(cls, 0) + 1
        return out

    def starts(self) -> Dict[str, int]:
        """Per host, the media whose first event names it."""
        out: Dict[str, int] = {}
        for edge in self.media.values():
            out[edge.first[1]] = out.get(edge.first[1], 0) + 1
        return out

    def add_course(self, mid: str, edge: Optional[MediaEdge], rows: Dict[str, HostRow], pairs: Dict[str, int],
                   sign: int = 1) -> None:
        """Add one media's :func:`course_of` (or with ``sign`` -1 take it out again; ``edge`` is then
        ignored and the media's row leaves). A host row or a pair that reaches zero leaves."""
        for worker, row in rows.items():
            mine = self.hosts.get(worker)
            if mine is None:
                mine = self.hosts[worker] = HostRow()
            mine.add(row, sign)
            if mine.events == 0:
                del self.hosts[worker]
        for worker, count in pairs.items():
            value = self.pairs.get((mid, worker), 0) + sign * count
            if value:
                self.pairs[(mid, worker)] = value
            else:
                self.pairs.pop((mid, worker), None)
            self.progress_events += sign * count
        if sign > 0:
            self.media[mid] = edge
        else:
            self.media.pop(mid, None)

    def merge(self, later: "HostReport") -> "HostReport":
        """The result of this stream followed by ``later``'s, from the two results alone. Neither
        operand changes."""
        out = HostReport(self.frames + later.frames, self.progress_events + later.progress_events,
                         self.progress_decode_errors + later.progress_decode_errors,
                         {k: v.copy() for k, v in self.hosts.items()}, dict(self.pairs),
                         {k: dataclasses.replace(v) for k, v in self.media.items()})
        for worker, row in later.hosts.items():
            out.hosts.setdefault(worker, HostRow()).add(row)
        for pair, count in later.pairs.items():
            out.pairs[pair] = out.pairs.get(pair, 0) + count
        shift = self.frames
        for mid, edge in later.media.items():
            first = (edge.first[0] + shift,) + tuple(edge.first[1:])
            last = (edge.last[0] + shift,) + tuple(edge.last[1:])
            mine = out.media.get(mid)
            if mine is None:
                out.media[mid] = MediaEdge(edge.events, first, last)
                continue
            before, worker = mine.last, first[1]
            if before[1] != worker:       # the boundary pair is a handover
                out.hosts[before[1]].lost += 1
                out.hosts[worker].taken += 1
            else:                          # the two stints are one
                out.hosts[worker].stints -= 1
                if before[2] == first[2] and first[3] < before[3]:
                    out.hosts[worker].rewinds += 1
            mine.events += edge.events
            mine.last = last
        return out

    def to_json(self, per_media: bool = False) -> dict:
        """Hosts with sorted names, classes by their enum names (``unknown`` for the rest). The
        per-media rows, ``media``, only where ``per_media``."""
        names = replay.status_names()

        def by_name(counts):
            named = {_class_name(c, names): v for c, v in counts.items()}
            return {k: named[k] for k in sorted(named)}
        holding = self.holding()
        media_of: Dict[str, int] = {}
        for _, worker in self.pairs:
            media_of[worker] = media_of.get(worker, 0) + 1
        hosts = {}
        for worker in sorted(self.hosts):
            row = self.hosts[worker]
            hosts[worker] = {"events": row.events, "media": media_of.get(worker, 0), "stints": row.stints,
                             "taken": row.taken, "lost": row.lost, "rewinds": row.rewinds,
                             "by_status": by_name(row.by_class), "holding": by_name(holding.get(worker, {}))}
        out = {"frames": self.frames, "progress_events": self.progress_events,
               "progress_decode_errors": self.progress_decode_errors, "host_count": len(self.hosts),
               "media_count": len(self.media), "handovers": self.handovers, "rewinds": self.rewinds, "hosts": hosts}
        if per_media:
            per: Dict[str, Dict[str, int]] = {}
            for (mid, worker), count in self.pairs.items():
                per.setdefault(mid, {})[worker] = count
            out["media"] = {mid: {"events": self.media[mid].events, "first": list(self.media[mid].first),
                                  "last": list(self.media[mid].last),
                                  "hosts": {w: per[mid][w] for w in sorted(per[mid])}} for mid in sorted(self.media)}
        return out

    @classmethod
    def from_json(cls, obj: dict) -> "HostReport":
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

        def event(e) -> Event:
            return int(e[0]), str(e[1]), int(e[2]), int(e[3])
        hosts = {w: HostRow(int(r["events"]), {number(k): int(v) for k, v in r["by_status"].items()}, int(r["stints"]),
                            int(r["taken"]), int(r["lost"]), int(r["rewinds"])) for w, r in obj["hosts"].items()}
        pairs = {(mid, w): int(count) for mid, row in obj["media"].items() for w, count in row["hosts"].items()}
        media = {mid: MediaEdge(int(row["events"]), event(row["first"]), event(row["last"]))
                 for mid, row in obj["media"].items()}
        return cls(int(obj["frames"]), int(obj["progress_events"]), int(obj["progress_decode_errors"]), hosts, pairs,
                   media)


def progress_events_of(events: Iterable[Tuple[int, int, bytes]], dialect: str = "protobufjs"):
    """``(per media its (index, host, status, progress) events in the order given, decode errors)`` of
    ``(index, topic, body)`` triples, decoded with the service's codec; frames of other topics are
    passed over."""
    replay._check_dialect(dialect)
    decode = ops.codec_for(replay._types()[1], dialect).decode
    per_media: Dict[str, List[Event]] = {}
    errors = 0
    for i, topic, body in events:
        if topic != PROGRESS_ID:
            continue
        try:
            m = decode(body)
        except proto.DecodeError:
            errors += 1
            continue
        per_media.setdefault(m.mediaId, []).append((i, m.host, m.status, m.progress))
    return per_media, errors


def hosts_events(events: Iterable[Tuple[int, int, bytes]], dialect: str = "protobufjs") -> HostReport:
    """The definition, over ``(index, topic, body)`` triples in stream order. ``frames`` is left to
    the caller."""
    per_media, errors = progress_events_of(events, dialect)
    names = replay.status_names()
    report = HostReport(progress_decode_errors=errors)
    for mid, run in per_media.items():
        report.add_course(mid, *course_of(run, names))
    return report


def hosts_cpu(data, dialect: str = "protobufjs") -> HostReport:
    """The hosts of a framed stream, written plainly: the oracle and the ``--device cpu`` path.
    Raises ``ValueError`` for broken framing, as ``extract_cpu`` does."""
    frames = 0

    def events() -> Iterator[Tuple[int, int, bytes]]:
        nonlocal frames
        for i, (topic, body) in enumerate(iter_frames(data)):
            frames = i + 1
            yield i, topic, body
    report = hosts_events(events(), dialect)
    report.frames = frames
    return report


def hosts_gpu(data, device="cuda", dialect: str = "protobufjs", hash_mask: Optional[int] = None) -> HostReport:
    """The same :class:`HostReport` as :func:`hosts_cpu`, computed on ``device``: the host indexes the
    frame headers; the device decodes the progress frames, numbers the media and the workers, sorts
    the events stably by media, counts the events per (media, worker) pair and walks every media's
    run (``ops/gpu_hosts.py``). Only one row per worker, per media and per pair comes back. ``data``
    must be below 2^31 bytes (:func:`hosts_file` cuts chunks). Raises if the HIP library or the
    device is missing."""
    from .ops import gpu_hosts
    replay._check_dialect(dialect)
    return gpu_hosts.hosts(data, device=device, dialect=dialect, hash_mask=hash_mask)[0]


def hosts_file(path, device: str = "cpu", dialect: str = "protobufjs",
               chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES) -> Tuple[HostReport, int]:
    """The hosts of the file at ``path`` (or an open binary file) chunk by chunk, each chunk cut at a
    frame boundary (``replay.iter_chunks``), merged on the CPU as ``transitions_file`` does.
    ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``). Returns ``(HostReport,
    host_frames)``: the frames that a device run left to the CPU."""
    replay._check_dialect(dialect)

    def on_device(device):
        from .ops import gpu_hosts
        return lambda chunk: gpu_hosts.hosts(chunk, device=device, dialect=dialect)
    cut = capture_io.per_chunk(device, lambda chunk: hosts_cpu(chunk, dialect), on_device)
    return replay.merge_chunks(path, chunk_bytes, HostReport(), cut)
