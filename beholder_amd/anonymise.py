"""Replace every ``mediaId`` and ``host`` of a framed stream by a keyed pseudonym; the result is a
framed stream again, fit to leave its owner's hands.

A dead-letter capture is what one attaches to a bug report or hands to someone else to replay, and
it carries every media id of the library and every worker host name in clear text. Every report
(``summarise``, ``transitions``, ``hosts``, ``stages``) groups by ``mediaId`` and ``host``, so a
replacement must be stable: ``anonymise`` writes every decoded status and progress event in the
service's canonical encoding (``normalise``) with the chosen strings replaced by pseudonyms that
depend on the key, the field and the string alone. The same key gives the same pseudonym in every
chunk, run and capture; the reports of the output are those of the input up to renaming; nobody
without the key gets back to the names. :func:`anonymise_cpu` is the definition;
:func:`anonymise_gpu` computes the same :class:`Anonymised` on the device
(``ops/hip/telemetry_anonymise.hip``, ``ops/gpu_anonymise.py``).

The pseudonym, :func:`pseudonym_of`:

* ``""`` maps to ``""``: proto3 does not tell an absent string from an empty one, and an absent
  field stays absent;
* otherwise it is ``hashlib.blake2s(text.encode("utf-8"), key=key, digest_size=16,
  person=PERSON[field]).hexdigest()``, 32 lowercase hex characters, with ``PERSON = {"mediaId":
  b"bh.media", "host": b"bh.host"}``: a media and a host of one name get different pseudonyms;
* ``key`` is 16 to 32 bytes;
* the hash runs over the *decoded* string. Under protobufjs that is after U+FFFD substitution, so two
  spellings of one string get one pseudonym and ``anonymise(normalise(x)) == anonymise(x)``.

Frames are read as ``normalise`` reads them (``normalise.canon_of``): a frame it treats as a decoded
event becomes the codec's ``encode`` of the decoded message with the chosen strings replaced; fields
are in ascending number, defaults omitted, and unknown fields are gone, which is wanted here: they may
hold anything. Every other frame is **undecoded**, and ``Policy.undecoded`` drops it (the default,
unlike ``normalise``: such a frame may hold names in any form) or keeps it byte for byte. Frames stay
in stream order. ``Policy.fields`` chooses the strings to replace; a string outside it is written as
``normalise`` writes it.

What the output still tells is in docs/OPERATIONS.md: the numbers, the order and the counts, and how
often each pseudonym occurs.

Results merge by concatenation: every frame is decided on its own, which is how
:func:`anonymise_file` handles a file of any size in chunks, each written before the next is read. A
result never holds the key; it holds ``key_id``, eight hex characters that depend on the key alone,
so that results under different keys refuse to merge.
"""
from __future__ import annotations

import dataclasses
import functools
import hashlib
from typing import Callable, FrozenSet, List

from . import capture_io, ops, replay
from .capture_io import frame_spans
from .coalesce import DROP, KEEP, UNDECODED_MODES
from .models import proto
from .normalise import frame_of
from .topics import PROGRESS_ID, STATUS_ID

__all__ = ["DROP", "KEEP", "PERSON", "FIELDS", "Policy", "Anonymised", "pseudonym_of", "anon_of", "anonymise_cpu",
           "anonymise_gpu", "anonymise_file"]

PERSON = {"mediaId": b"bh.media", "host": b"bh.host"}
FIELDS = frozenset(PERSON)
KEY_BYTES = (16, 32)  # the least and the most


def _check_key(key) -> None:
    if not isinstance(key, bytes):
        raise TypeError(f"key is bytes, not {type(key).__name__}")
    if not KEY_BYTES[0] <= len(key) <= KEY_BYTES[1]:
        raise ValueError(f"key has {KEY_BYTES[0]} to {KEY_BYTES[1]} bytes, not {len(key)}")


def pseudonym_of(key: bytes, field: str, text: str) -> str:
    """The pseudonym of ``text`` as a ``field`` (``mediaId`` or ``host``) under ``key``."""
    _check_key(key)
    if field not in PERSON:
        raise ValueError(f"unknown field {field!r} ({'|'.join(PERSON)})")
    if text == "":
        return ""
    return hashlib.blake2s(text.encode("utf-8"), key=key, digest_size=16, person=PERSON[field]).hexdigest()


@dataclasses.dataclass(frozen=True)
class Policy:
    """``key`` makes the pseudonyms. ``undecoded`` is what happens to the frames that are no decoded
    event: ``drop`` removes them, ``keep`` copies them byte for byte, names included. ``fields`` are
    the strings to replace, a non-empty subset of ``mediaId`` and ``host``."""
    key: bytes = dataclasses.field(repr=False)
    undecoded: str = "drop"
    fields: FrozenSet[str] = FIELDS

    def __post_init__(self):
        _check_key(self.key)
        if not isinstance(self.undecoded, str):
            raise TypeError(f"undecoded is a string, not {type(self.undecoded).__name__}")
        if self.undecoded not in UNDECODED_MODES:
            raise ValueError(f"unknown undecoded policy {self.undecoded!r} ({'|'.join(UNDECODED_MODES)})")
        if isinstance(self.fields, str):
            raise TypeError("fields is a set of field names, not a string")
        fields = frozenset(self.fields)
        if not fields or not fields <= FIELDS:
            raise ValueError(f"fields is a non-empty subset of {sorted(FIELDS)}, not {sorted(map(str, fields))}")
        object.__setattr__(self, "fields", fields)

    @property
    def key_id(self) -> str:
        """Eight hex characters that depend on the key alone and give nothing of it away."""
        return hashlib.blake2s(self.key, digest_size=16, person=b"bh.keyid").hexdigest()[:8]


def _check_policy(policy) -> None:
    if not isinstance(policy, Policy):
        raise TypeError(f"policy is an anonymise.Policy, not {type(policy).__name__}")


def anon_of(policy: Policy, dialect: str = "protobufjs") -> Callable[[int, bytes], object]:
    """``anon(topic, body)`` for ``policy``: ``KEEP`` (the frame stays as it is), ``DROP``, or the new
    body bytes of a decoded event. The definition of what :func:`anonymise_cpu` writes, and what the
    device path asks about the frames it leaves to the host."""
    _check_policy(policy)
    replay._check_dialect(dialect)
    status_type, progress_type = replay._types()
    codecs = {STATUS_ID: ops.codec_for(status_type, dialect), PROGRESS_ID: ops.codec_for(progress_type, dialect)}
    undecoded = KEEP if policy.undecoded == "keep" else DROP

    def renamer(field: str):
        if field not in policy.fields:
            return str  # in clear
        # a capture repeats its names; the cache changes no answer
        return functools.lru_cache(maxsize=1 << 16)(functools.partial(pseudonym_of, policy.key, field))
    media, host = renamer("mediaId"), renamer("host")

    def anon(topic: int, body: bytes):
        codec = codecs.get(topic)
        if codec is None:
            return undecoded
        try:
            m = codec.decode(body)
        except proto.DecodeError:
            return undecoded
        if topic == STATUS_ID:
            return bytes(codec.encode((media(m.mediaId), m.status)))
        return bytes(codec.encode((media(m.mediaId), m.status, m.progress, host(m.host))))
    return anon


@dataclasses.dataclass
class Anonymised:
    data: bytes = b""            # the output frames, headers included, in stream order
    indices: List[int] = dataclasses.field(default_factory=list)  # their indices in the input, ascending
    frames: int = 0              # the input's frame count
    events: int = 0              # the input's decoded events
    dialect: str = "protobufjs"  # what the frames were read as
    undecoded: str = "drop"
    fields: FrozenSet[str] = FIELDS  # the strings that were replaced
    key_id: str = ""             # Policy.key_id of the key: never the key

    def merge(self, later: "Anonymised") -> "Anonymised":
        """The result for this one's input followed by ``later``'s: every frame is decided on its
        own, so this is concatenation with ``later``'s indices shifted. Neither operand changes."""
        mine = (self.dialect, self.undecoded, self.fields, self.key_id)
        theirs = (later.dialect, later.undecoded, later.fields, later.key_id)
        if mine != theirs:
            raise ValueError("cannot merge dialect={!r} undecoded={!r} fields={} key_id={!r} with dialect={!r} "
                             "undecoded={!r} fields={} key_id={!r}".format(
                                 mine[0], mine[1], sorted(mine[2]), mine[3], theirs[0], theirs[1], sorted(theirs[2]),
                                 theirs[3]))
        return Anonymised(self.data + later.data, self.indices + [i + self.frames for i in later.indices],
                          self.frames + later.frames, self.events + later.events, self.dialect, self.undecoded,
                          self.fields, self.key_id)


def result_for(policy: Policy, dialect: str, data: bytes = b"", indices=None, frames: int = 0,
               events: int = 0) -> Anonymised:
    """An :class:`Anonymised` with what ``policy`` and ``dialect`` say of it."""
    return Anonymised(data, [] if indices is None else indices, frames, events, dialect, policy.undecoded,
                      policy.fields, policy.key_id)


def anonymise_cpu(data, policy: Policy, dialect: str = "protobufjs") -> Anonymised:
    """The anonymised stream, written plainly: the oracle and the ``--device cpu`` path. Raises
    ``ValueError`` for broken framing, as ``normalise_cpu`` does."""
    anon = anon_of(policy, dialect)
    view = memoryview(data)
    spans = list(frame_spans(view))
    parts, indices = [], []
    events = 0
    for i, (a, b) in enumerate(spans):
        topic = view[a + 4]
        c = anon(topic, bytes(view[a + 5:b]))
        if c is DROP:
            continue
        if c is KEEP:
            parts.append(view[a:b])
        else:
            events += 1
            parts.append(frame_of(topic, c))
        indices.append(i)
    return result_for(policy, dialect, b"".join(parts), indices, len(spans), events)


def anonymise_gpu(data, policy: Policy, device="cuda", dialect: str = "protobufjs") -> Anonymised:
    """The same :class:`Anonymised` as :func:`anonymise_cpu`, computed on ``device``: the host indexes
    the frame headers; the device decodes every frame into a plan, hashes the chosen strings, sizes
    the output frames, scans the sizes and writes the output bytes (``ops/gpu_anonymise.py``). The key
    does not go to the device. ``data`` must leave room for its growth below 2^31 bytes
    (:func:`anonymise_file` cuts chunks). Raises if the HIP library or the device is missing."""
    from .ops import gpu_anonymise
    _check_policy(policy)
    replay._check_dialect(dialect)
    return gpu_anonymise.anonymise(data, policy, device=device, dialect=dialect)[0]


def anonymise_file(path, out, policy: Policy, device: str = "cpu", dialect: str = "protobufjs",
                   chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES, indices_out=None) -> dict:
    """Anonymise the file at ``path`` (or an open binary file) chunk by chunk into the binary file
    ``out``: each chunk is cut at a frame boundary (``replay.iter_chunks``), anonymised on its own and
    written before the next chunk is read, so memory stays at the chunk size. Every frame is decided
    on its own and a pseudonym depends on the key and the string alone, so the cuts do not show. A
    stream that ends inside a frame leaves whole frames only, and then raises.

    ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``). ``indices_out``, a text
    file, gets the input indices of the output's frames, one per line.
    Returns ``{frames, kept, kept_bytes, in_bytes, events, undecoded, host_frames}``: ``undecoded``
    counts the input's frames that are no decoded event, ``host_frames`` the frames a device run left
    to the host."""
    _check_policy(policy)
    replay._check_dialect(dialect)

    def on_device(device):
        from .ops import gpu_anonymise
        return capture_io.with_chunk_bytes_hint(gpu_anonymise.TooLarge, lambda chunk: gpu_anonymise.anonymise(
            chunk, policy, device=device, dialect=dialect))
    cut = capture_io.per_chunk(device, lambda chunk: anonymise_cpu(chunk, policy, dialect), on_device)
    counts = {"frames": 0, "kept": 0, "kept_bytes": 0, "in_bytes": 0, "events": 0, "undecoded": 0, "host_frames": 0}
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
            counts["undecoded"] += part.frames - part.events
            counts["host_frames"] += host_frames
    return counts
