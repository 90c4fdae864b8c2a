"""Read NDJSON rows back into a framed stream: the inverse of ``export``, and the way back for a
capture that was filtered or repaired as text with jq, DuckDB, pandas or grep.

``import`` is a Python keyword, so the module is ``import_rows``; the command is ``import``.
:func:`import_cpu` is the definition; :func:`import_gpu` computes the same :class:`Imported` on the
device (``ops/hip/telemetry_import.hip``, ``ops/gpu_import.py``). ``transport/framing.py`` keeps its
line reader for the service's NDJSON source: it takes the two queue names only, so it cannot read an
export that holds another topic byte.

**Lines.** The input is bytes and is cut at ``\\n`` only (a raw U+2028 inside a string is legal JSON,
and ``json.dumps(ensure_ascii=False)`` writes it raw). A last line without a newline is a line. The
bytes space, ``\\t`` and ``\\r`` are stripped from both ends of a line, so CRLF files work; a line
that is then empty is blank: it makes no frame and is no error. Every line has a 0-based number, the
blank ones included: ``base`` plus its position in the input.

**Rows.** A row is strict UTF-8 and a JSON object. Of its keys only ``topic``, ``b64`` and ``json``
are read; ``i``, ``name`` and every other key are ignored whatever their value, rows are taken in input
order, and ``name`` is not checked against ``status``.

* ``topic`` is one of the two queue names (``topics.TOPIC_IDS``), or an ``int`` (no ``bool``) in
  0..255, the topic byte: ``export`` writes a number for every other topic, and 1 and 2 are accepted
  as numbers too.
* ``b64``, where present, wins, as in ``ndjson_line_to_frame``: a ``str`` that
  ``base64.b64decode(s, validate=True)`` accepts. The body is the decoded bytes, verbatim.
* otherwise ``json`` is a ``dict`` and the topic byte is 1 or 2. Its keys are a subset of ``mediaId``
  and ``status`` for topic 1, and of ``mediaId``, ``status``, ``progress`` and ``host`` for topic 2.
  ``mediaId`` and ``host`` are ``str`` that encode to UTF-8; ``status`` is an int32 ``int`` (no
  ``bool``) or a ``str`` whose ``.upper()`` is a ``TelemetryStatusEntry`` name; ``progress`` is an int32
  ``int`` (no ``bool``). A float is malformed, even ``1.0``. An absent key takes the default. The
  body is the canonical body that ``normalise.py`` writes out, built by the service's own encoder
  (``ops.codec_for(type, dialect).encode``); it reads the same in either dialect, so there is no
  ``--dialect``.

Everything else is a malformed row (:class:`MalformedRow`). ``Policy.malformed`` is ``fail`` (the
first malformed line in input order raises ``ValueError`` with its line number and the reason) or
``skip`` (it makes no frame and is counted).

The law (``tests/test_import.py``): for any capture ``x`` in either dialect,
``import(export(x, undecoded=keep)) == normalise(x, undecoded=keep)`` byte for byte, other topics and
undecodable frames included.

Results merge by concatenation where the later one's ``base`` continues the earlier one's lines, which
is how :func:`import_file` handles a file of any size in chunks, each written before the next is read.
"""
from __future__ import annotations

import base64
import dataclasses
import json
from typing import Callable, List, Tuple

from . import capture_io, ops, replay
from .export import _check_base
from .normalise import frame_of
from .topics import PROGRESS_ID, STATUS_ID, TOPIC_IDS

DEFAULT_CHUNK_BYTES = 256 << 20  # the frames take less than the rows
MALFORMED_MODES = ("fail", "skip")
BLANK = b" \t\r"                 # what is stripped from both ends of a line
INT32 = range(-2 ** 31, 2 ** 31)
_KEYS = {STATUS_ID: ("mediaId", "status"), PROGRESS_ID: ("mediaId", "status", "progress", "host")}

__all__ = ["Policy", "Imported", "MalformedRow", "frame_of_row", "import_cpu", "import_gpu", "import_file"]


class MalformedRow(ValueError):
    """A line that is no row; the text is the reason."""


@dataclasses.dataclass(frozen=True)
class Policy:
    """What happens to a malformed row: ``fail`` raises at the first one in input order, ``skip``
    leaves it out and counts it."""
    malformed: str = "fail"

    def __post_init__(self):
        if not isinstance(self.malformed, str):
            raise TypeError(f"malformed is a string, not {type(self.malformed).__name__}")
        if self.malformed not in MALFORMED_MODES:
            raise ValueError(f"unknown malformed policy {self.malformed!r} ({'|'.join(MALFORMED_MODES)})")


def _check_policy(policy) -> None:
    if not isinstance(policy, Policy):
        raise TypeError(f"policy is an import_rows.Policy, not {type(policy).__name__}")
    if policy.malformed not in MALFORMED_MODES:
        raise ValueError(f"unknown malformed policy {policy.malformed!r} ({'|'.join(MALFORMED_MODES)})")


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def decided_frame_of_row(policy: Policy = Policy()) -> Callable[[bytes], Tuple[bytes, bool]]:
    """``frame(line)`` for a stripped, non-blank line: ``(the frame's bytes, whether it came from
    b64)``, or :class:`MalformedRow`. :func:`frame_of_row` with the count that :class:`Imported`
    keeps."""
    _check_policy(policy)
    status_type, progress_type = replay._types()
    # the canonical form reads the same in either dialect (tests/test_normalise.py), so either encoder does
    encoders = {STATUS_ID: ops.codec_for(status_type, "protobufjs").encode,
                PROGRESS_ID: ops.codec_for(progress_type, "protobufjs").encode}
    numbers = {name: number for number, name in replay.status_names().items()}

    def text_field(key: str, v) -> str:
        if not isinstance(v, str):
            raise MalformedRow(f"{key} is a string, not {type(v).__name__}")
        try:
            v.encode("utf-8")
        except UnicodeEncodeError:
            raise MalformedRow(f"{key} does not encode to UTF-8 (a lone surrogate)") from None
        return v

    def int_field(key: str, v) -> int:
        if not _is_int(v) or v not in INT32:
            raise MalformedRow(f"{key} is an int32, not {v!r}")
        return v

    def frame(line: bytes):
        try:
            rec = json.loads(bytes(line).decode("utf-8"))
        except UnicodeDecodeError:
            raise MalformedRow("not UTF-8") from None
        except (ValueError, RecursionError) as e:
            raise MalformedRow(f"not JSON ({e})") from None
        if not isinstance(rec, dict):
            raise MalformedRow(f"a row is a JSON object, not {type(rec).__name__}")
        topic = rec.get("topic")
        if isinstance(topic, str) and topic in TOPIC_IDS:
            topic = TOPIC_IDS[topic]
        elif not _is_int(topic) or not 0 <= topic <= 255:
            raise MalformedRow(f"unknown topic {topic!r}")
        if "b64" in rec:
            text = rec["b64"]
            if not isinstance(text, str):
                raise MalformedRow(f"b64 is a string, not {type(text).__name__}")
            try:
                return frame_of(topic, base64.b64decode(text, validate=True)), True
            except ValueError as e:  # binascii.Error is one; so is a str that is not ASCII
                raise MalformedRow(f"b64 is not base64 ({e})") from None
        if "json" not in rec:
            raise MalformedRow("a row needs 'b64' or 'json'")
        obj = rec["json"]
        if not isinstance(obj, dict):
            raise MalformedRow(f"json is an object, not {type(obj).__name__}")
        if topic not in _KEYS:
            raise MalformedRow(f"topic {topic} has no message type: its rows carry b64")
        fields = {}
        for key, v in obj.items():
            if key not in _KEYS[topic]:
                raise MalformedRow(f"unknown field {key!r} for topic {topic}")
            if key in ("mediaId", "host"):
                fields[key] = text_field(key, v)
            elif key == "status" and isinstance(v, str):
                if v.upper() not in numbers:
                    raise MalformedRow(f"unknown status {v!r}")
                fields[key] = numbers[v.upper()]
            else:
                fields[key] = int_field(key, v)
        return frame_of(topic, bytes(encoders[topic](fields))), False
    return frame


def frame_of_row(policy: Policy = Policy()) -> Callable[[bytes], bytes]:
    """``frame(line_bytes)`` for a stripped, non-blank line: the frame's bytes
    (``normalise.frame_of(topic, body)``), or :class:`MalformedRow` with a reason. The definition of
    what :func:`import_cpu` writes, and what the device path asks about the rows it leaves to the
    host."""
    frame = decided_frame_of_row(policy)
    return lambda line: frame(line)[0]


@dataclasses.dataclass
class Imported:
    data: bytes = b""            # the framed stream
    lines: List[int] = dataclasses.field(default_factory=list)  # the rows that became frames, by line number
    line_count: int = 0          # lines in the input, blank ones included
    events: int = 0              # frames made from json rows
    carried: int = 0             # frames made from b64 rows
    skipped: List[int] = dataclasses.field(default_factory=list)  # the line numbers left out under ``skip``
    base: int = 0                # the number of the input's first line
    malformed: str = "fail"

    def merge(self, later: "Imported") -> "Imported":
        """The result for this one's input followed by ``later``'s: concatenation. A line has its
        number, so ``later`` must have been imported with ``base = self.base + self.line_count``;
        ``ValueError`` otherwise. Neither operand changes."""
        if later.malformed != self.malformed:
            raise ValueError(f"cannot merge malformed={self.malformed!r} with malformed={later.malformed!r}")
        if later.base != self.base + self.line_count:
            raise ValueError(f"cannot merge lines from {later.base} after {self.line_count} lines from {self.base}: "
                             f"import the later part with base={self.base + self.line_count}")
        return Imported(self.data + later.data, self.lines + later.lines, self.line_count + later.line_count,
                        self.events + later.events, self.carried + later.carried, self.skipped + later.skipped,
                        self.base, self.malformed)


def split_lines(data) -> List[bytes]:
    """The lines of ``data``, cut at ``\\n`` only; a last line without a newline is a line."""
    lines = bytes(data).split(b"\n")
    if not lines[-1]:
        lines.pop()
    return lines


def malformed_line(number: int, reason) -> ValueError:
    return ValueError(f"line {number}: malformed row: {reason}")


def import_cpu(data, policy: Policy = Policy(), base: int = 0) -> Imported:
    """The frames, written plainly: the oracle and the ``--device cpu`` path."""
    _check_base(base)
    frame = decided_frame_of_row(policy)
    rows = split_lines(data)
    parts, lines, skipped = [], [], []
    events = carried = 0
    for k, line in enumerate(rows):
        line = line.strip(BLANK)
        if not line:
            continue
        try:
            f, from_b64 = frame(line)
        except MalformedRow as e:
            if policy.malformed == "fail":
                raise malformed_line(base + k, e) from None
            skipped.append(base + k)
            continue
        parts.append(f)
        lines.append(base + k)
        carried += from_b64
        events += not from_b64
    return Imported(b"".join(parts), lines, len(rows), events, carried, skipped, base, policy.malformed)


def import_gpu(data, policy: Policy = Policy(), device="cuda", base: int = 0) -> Imported:
    """The same :class:`Imported` as :func:`import_cpu`, computed on ``device``: the device finds the
    lines, reads every row into a plan, sizes its frame, scans the sizes and writes the frames' bytes
    (``ops/gpu_import.py``). ``data`` must stay below 2^31 bytes (:func:`import_file` cuts chunks).
    Raises if the HIP library or the device is missing."""
    from .ops import gpu_import
    _check_policy(policy)
    _check_base(base)
    return gpu_import.import_rows(data, policy, device=device, base=base)[0]


def iter_line_chunks(f, chunk_bytes: int):
    """Pieces of the binary file ``f`` that end after a ``\\n``: each is cut after the last newline
    within ``chunk_bytes``, and runs on to the next newline where one line alone is longer. The last
    piece may end without one."""
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, int) or chunk_bytes < 1:
        raise ValueError("chunk_bytes is a positive int")
    held, more = b"", True
    while True:
        if more and len(held) < chunk_bytes:
            piece = f.read(chunk_bytes - len(held))
            more = bool(piece)
            held += piece
        if not held:
            return
        cut = held.rfind(b"\n", 0, chunk_bytes)
        while cut < 0:  # one line alone is longer than the chunk: on to its newline
            cut = held.find(b"\n", chunk_bytes)
            if cut >= 0 or not more:
                break
            searched = len(held)
            piece = f.read(chunk_bytes)
            more = bool(piece)
            held += piece
            cut = held.find(b"\n", searched)
        if cut < 0:
            yield held
            return
        yield held[:cut + 1]
        held = held[cut + 1:]


def import_file(path, out, policy: Policy = Policy(), device: str = "cpu", chunk_bytes: int = DEFAULT_CHUNK_BYTES,
                lines_out=None) -> dict:
    """Import the file at ``path`` (or an open binary file) chunk by chunk into the binary file
    ``out``: each chunk ends after a newline (:func:`iter_line_chunks`), is imported on its own from
    the number its first line has in the file, and is written before the next chunk is read, so
    memory stays at the chunk size plus one line. Under ``fail`` the whole frames of the chunks before
    the malformed row's stay written, and then it raises.

    ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``). ``lines_out``, a text
    file, gets the line numbers of the rows that became frames, one per line.
    Returns ``{lines, rows, frames, events, carried, skipped, blank, in_bytes, out_bytes, host_rows}``:
    ``rows`` counts the lines that are not blank, ``host_rows`` the rows a device run left to the
    host."""
    _check_policy(policy)
    counts = {"lines": 0, "rows": 0, "frames": 0, "events": 0, "carried": 0, "skipped": 0, "blank": 0, "in_bytes": 0,
              "out_bytes": 0, "host_rows": 0}

    # a chunk's lines are numbered from the number its first line has in the file: the lines counted so far
    def on_device(device):
        from .ops import gpu_import
        return capture_io.with_chunk_bytes_hint(gpu_import.TooLarge, lambda chunk: gpu_import.import_rows(
            chunk, policy, device=device, base=counts["lines"]))
    frames = capture_io.per_chunk(device, lambda chunk: import_cpu(chunk, policy, counts["lines"]), on_device)
    with capture_io.open_source(path) as f:
        for chunk, part, host_rows in capture_io.chunk_parts(f, chunk_bytes, iter_line_chunks, frames):
            out.write(part.data)
            if lines_out is not None:
                capture_io.write_indices(lines_out, part.lines)  # absolute already
            rows = len(part.lines) + len(part.skipped)
            counts["lines"] += part.line_count
            counts["rows"] += rows
            counts["frames"] += len(part.lines)
            counts["events"] += part.events
            counts["carried"] += part.carried
            counts["skipped"] += len(part.skipped)
            counts["blank"] += part.line_count - rows
            counts["in_bytes"] += len(chunk)
            counts["out_bytes"] += len(part.data)
            counts["host_rows"] += host_rows
    return counts
