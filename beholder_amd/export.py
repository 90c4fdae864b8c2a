"""Write every frame of a framed stream as one NDJSON row, read in the service's dialect: the way out
for jq, DuckDB, pandas and grep.

Every other capture command answers one fixed question or cuts a capture into another capture.
``export`` decodes: a status or progress frame that the codec reads becomes a row with its fields,
every other frame is carried losslessly as base64, and each row holds the frame's index in the whole
input, the one ``summarise`` reports as ``last_status_index`` and every ``--indices`` file lists.
:func:`export_cpu` is the definition; :func:`export_gpu` computes the same :class:`Exported` on the
device (``ops/hip/telemetry_export.hip``, ``ops/gpu_export.py``). ``decode`` stays the debugging stub
it is: it reads through ``google.protobuf.json_format`` whatever the dialect and names no index.

A row is ``json.dumps(obj, ensure_ascii=False, separators=(",", ":"))`` in UTF-8 and ends in ``\\n``;
its keys come in exactly this order:

* a decoded status event (topic 1, ``api.TelemetryStatus`` through ``ops.codec_for(type, dialect)``):
  ``{"i":I,"topic":"v1.telemetry.status","json":{"mediaId":S,"status":N},"name":NAME}``
* a decoded progress event (topic 2, ``api.TelemetryProgress``):
  ``{"i":I,"topic":"v1.telemetry.progress","json":{"mediaId":S,"status":N,"progress":P,"host":H},"name":NAME}``
* an undecoded frame (the codec raises, or another topic byte): ``{"i":I,"topic":T,"b64":B}``

``I`` is ``base`` plus the frame's index in ``data``. ``S`` and ``H`` are the decoded strings (U+FFFD
for invalid UTF-8 under protobufjs, ``""`` when absent), ``N`` and ``P`` the raw int32 values; every
field is present, defaults included. ``NAME`` is the ``TelemetryStatusEntry`` name of ``N`` or
``null``: one column of one type. ``T`` is the queue name for topic bytes 1 and 2 and the topic byte
as a number otherwise. ``B`` is the standard base64 of the body with padding.

The rows have the shape ``transport.framing.ndjson_line_to_frame`` reads (``topic`` + ``json``, or
``topic`` + ``b64``), so for a capture of the two topics ``ndjson_to_frames(export(x))`` is
``normalise(x)`` (``tests/test_export.py``): an export is NDJSON input to the service.

``Policy.undecoded`` is ``normalise``'s: ``drop`` writes no row for an undecoded frame.

Results merge by concatenation where the later one's ``base`` continues the earlier one's frames (a
row carries its index), which is how :func:`export_file` handles a file of any size in chunks, each
written before the next is read.
"""
from __future__ import annotations

import base64
import dataclasses
import json
from typing import Callable, List

from . import capture_io, ops, replay
from .capture_io import frame_spans
from .coalesce import DROP
from .models import proto
from .normalise import Policy, _check_policy
from .topics import PROGRESS_ID, STATUS_ID, topic_name

DEFAULT_CHUNK_BYTES = 64 << 20  # the rows take three to five times the input's bytes
MAX_BASE = 2 ** 62              # the device adds the frame's number to it in 64 bits

__all__ = ["DROP", "Policy", "Exported", "row_of", "decoded_row_of", "export_cpu", "export_gpu", "export_file"]


def _check_base(base) -> None:
    if isinstance(base, bool) or not isinstance(base, int) or not 0 <= base <= MAX_BASE:
        raise ValueError(f"base is an int in 0..2^62, not {base!r}")


def decoded_row_of(policy: Policy = Policy(), dialect: str = "protobufjs") -> Callable[[int, int, bytes], tuple]:
    """``row(index, topic, body)`` for ``policy``: ``(the row's bytes or DROP, whether the frame is a
    decoded event)``. :func:`row_of` with the count that :class:`Exported` keeps."""
    _check_policy(policy)
    replay._check_dialect(dialect)
    status_type, progress_type = replay._types()
    codecs = {STATUS_ID: ops.codec_for(status_type, dialect), PROGRESS_ID: ops.codec_for(progress_type, dialect)}
    names = replay.status_names()
    drop = policy.undecoded == "drop"

    def dumps(obj) -> bytes:
        return (json.dumps(obj, ensure_ascii=False, separators=(",", ":")) + "\n").encode("utf-8")

    def row(index: int, topic: int, body: bytes):
        codec = codecs.get(topic)
        if codec is not None:
            try:
                m = codec.decode(body)
            except proto.DecodeError:
                m = None
            if m is not None:
                fields = {"mediaId": m.mediaId, "status": m.status}
                if topic == PROGRESS_ID:
                    fields["progress"] = m.progress
                    fields["host"] = m.host
                return dumps({"i": index, "topic": topic_name(topic), "json": fields, "name": names.get(m.status)}), True
        if drop:
            return DROP, False
        return dumps({"i": index, "topic": topic_name(topic) or topic,
                      "b64": base64.b64encode(body).decode("ascii")}), False
    return row


def row_of(policy: Policy = Policy(), dialect: str = "protobufjs") -> Callable[[int, int, bytes], object]:
    """``row(index, topic, body)`` for ``policy``: the row's bytes, newline included, or ``DROP``. The
    definition of what :func:`export_cpu` writes, and what the device path asks about the frames it
    leaves to the host."""
    row = decoded_row_of(policy, dialect)
    return lambda index, topic, body: row(index, topic, body)[0]


@dataclasses.dataclass
class Exported:
    data: bytes = b""            # the rows, each ending in a newline, in stream order
    indices: List[int] = dataclasses.field(default_factory=list)  # the rows' ``i``, ascending
    frames: int = 0              # the input's frame count
    events: int = 0              # the input's decoded events
    base: int = 0                # the index of the input's first frame
    dialect: str = "protobufjs"  # what the frames were read as
    undecoded: str = "keep"

    def merge(self, later: "Exported") -> "Exported":
        """The result for this one's input followed by ``later``'s: concatenation. A row carries its
        index, so ``later`` must have been exported with ``base = self.base + self.frames``;
        ``ValueError`` otherwise. Neither operand changes."""
        if (later.dialect, later.undecoded) != (self.dialect, self.undecoded):
            raise ValueError(f"cannot merge dialect={self.dialect!r} undecoded={self.undecoded!r} with "
                             f"dialect={later.dialect!r} undecoded={later.undecoded!r}")
        if later.base != self.base + self.frames:
            raise ValueError(f"cannot merge rows from index {later.base} after {self.frames} frames from index "
                             f"{self.base}: export the later part with base={self.base + self.frames}")
        return Exported(self.data + later.data, self.indices + later.indices, self.frames + later.frames,
                        self.events + later.events, self.base, self.dialect, self.undecoded)


def export_cpu(data, policy: Policy = Policy(), dialect: str = "protobufjs", base: int = 0) -> Exported:
    """The rows, written plainly: the oracle and the ``--device cpu`` path. Raises ``ValueError`` for
    broken framing, as ``extract_cpu`` does."""
    _check_base(base)
    row = decoded_row_of(policy, dialect)
    view = memoryview(data)
    spans = list(frame_spans(view))
    parts, indices = [], []
    events = 0
    for k, (a, b) in enumerate(spans):
        r, decoded = row(base + k, view[a + 4], bytes(view[a + 5:b]))
        events += decoded
        if r is DROP:
            continue
        parts.append(r)
        indices.append(base + k)
    return Exported(b"".join(parts), indices, len(spans), events, base, dialect, policy.undecoded)


def export_gpu(data, policy: Policy = Policy(), device="cuda", dialect: str = "protobufjs", base: int = 0) -> Exported:
    """The same :class:`Exported` as :func:`export_cpu`, computed on ``device``: the host indexes the
    frame headers; the device decodes every frame into a plan, sizes its row, scans the sizes and
    writes the rows' bytes (``ops/gpu_export.py``). The rows of ``data`` must stay below 2^31 bytes
    (:func:`export_file` cuts chunks). Raises if the HIP library or the device is missing."""
    from .ops import gpu_export
    _check_policy(policy)
    replay._check_dialect(dialect)
    _check_base(base)
    return gpu_export.export(data, policy, device=device, dialect=dialect, base=base)[0]


def export_file(path, out, policy: Policy = Policy(), device: str = "cpu", dialect: str = "protobufjs",
                chunk_bytes: int = DEFAULT_CHUNK_BYTES, indices_out=None) -> dict:
    """Export the file at ``path`` (or an open binary file) chunk by chunk into the binary file
    ``out``: each chunk is cut at a frame boundary (``replay.iter_chunks``), exported on its own from
    the index its first frame has in the file, and written before the next chunk is read, so memory
    stays at the chunk size. A stream that ends inside a frame leaves whole rows only, and then
    raises.

    ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``). ``indices_out``, a text
    file, gets the rows' indices, one per line.
    Returns ``{frames, rows, out_bytes, in_bytes, events, undecoded, host_frames}``: ``undecoded``
    counts the input's frames that are no decoded event, ``host_frames`` the frames a device run left
    to the host."""
    _check_policy(policy)
    replay._check_dialect(dialect)
    counts = {"frames": 0, "rows": 0, "out_bytes": 0, "in_bytes": 0, "events": 0, "undecoded": 0, "host_frames": 0}

    # a chunk's rows start at the index its first frame has in the file: the frames counted so far
    def on_device(device):
        from .ops import gpu_export
        return capture_io.with_chunk_bytes_hint(gpu_export.TooLarge, lambda chunk: gpu_export.export(
            chunk, policy, device=device, dialect=dialect, base=counts["frames"]))
    rows = capture_io.per_chunk(device, lambda chunk: export_cpu(chunk, policy, dialect, counts["frames"]), on_device)
    with capture_io.open_source(path) as f:
        for chunk, part, host_frames in capture_io.chunk_parts(f, chunk_bytes, replay.iter_chunks, rows):
            out.write(part.data)
            if indices_out is not None:
                capture_io.write_indices(indices_out, part.indices)  # absolute already
            counts["frames"] += part.frames
            counts["rows"] += len(part.indices)
            counts["out_bytes"] += len(part.data)
            counts["in_bytes"] += len(chunk)
            counts["events"] += part.events
            counts["undecoded"] += part.frames - part.events
            counts["host_frames"] += host_frames
    return counts
