"""Salvage the frames of a damaged capture: the framed stream that is left once the spans that fit
no frame are cut out.

Every capture command walks the ``u32 L | u8 topic | body`` framing and gives up at the first header
that does not fit (``capture_io.frame_spans``, ``replay.iter_chunks``). A writer killed inside its
last frame, two partial files joined or one overwritten block leave a capture that none of them
reads. A frame stream carries no sync marker, so the way back is to ask at every byte offset "could
a frame start here?". :func:`recover_cpu` is the definition; :func:`recover_gpu` computes the same
:class:`Recovered` on the device (``ops/hip/telemetry_recover.hip``, ``ops/gpu_recover.py``).

Over a buffer of ``n`` bytes, with ``Policy.max_frame``:

* ``well_framed(p)``: ``p + 4 <= n``, the little-endian ``L`` at ``p`` has ``1 <= L <= max_frame``,
  and ``end(p) = p + 4 + L <= n``.
* ``anchor(q)``: ``well_framed(q)``; the topic byte is status or progress; the body decodes with
  ``ops.codec_for(type, dialect)`` without ``DecodeError``; the decoded ``mediaId`` is not empty; and
  ``end(q) == n`` or ``well_framed(end(q))``.
* The walk starts in sync at ``p = 0``. In sync at ``p < n``: a well-framed ``p`` is a recovered
  frame as it is, and the walk goes on at ``end(p)``; a capture legitimately holds other topics and
  bodies that do not decode, so framing alone decides here. Otherwise a gap opens at ``p``: it runs
  to the smallest ``q > p`` with ``anchor(q)``, whose frame is recovered, and the walk goes on in
  sync at ``end(q)``; where there is no such ``q`` the gap runs to ``n`` and the walk ends.

**The frame just before a gap is the one to distrust.** A damaged length that is still well framed
is accepted like any other, and is only found out by what follows it: the walk lands inside a body,
a gap opens there, and the frame before the gap may be made of the bytes of several.

Chunks: ``recover_cpu(..., final=False)`` takes no decision at an offset ``> n - H`` with
``H = 2 * (4 + max_frame)``, neither in sync nor as a resync candidate, so every decision it takes
has all its bytes in hand and the ``== n`` clause never applies. It stops at such an offset and
returns it as ``consumed``, with ``resync`` true where a gap was open; the open gap's bytes up to
``consumed`` are a gap that :meth:`Recovered.merge` joins with the next part's leading gap.
``resync=True`` on entry starts the walk with a gap open at 0, where offset 0 is a candidate itself.
:func:`recover_file` at any legal ``chunk_bytes`` gives byte for byte what :func:`recover_cpu` gives
for the whole file: ``data``, ``offsets`` and ``gaps``.
"""
from __future__ import annotations

import bisect
import dataclasses
import json
import struct
from typing import Callable, List, Tuple

from . import capture_io, ops, replay
from .models import proto
from .topics import PROGRESS_ID, STATUS_ID

MAX_FRAME_LIMIT = 16 << 20  # the service reader's own limit (ops/csrc/py_ingest.cpp)


@dataclasses.dataclass(frozen=True)
class Policy:
    """``max_frame``: the longest ``L`` a frame header may hold, ``1 .. 16 << 20``."""
    max_frame: int = 1 << 20

    def __post_init__(self):
        if isinstance(self.max_frame, bool) or not isinstance(self.max_frame, int):
            raise TypeError(f"max_frame is an int, not {type(self.max_frame).__name__}")
        if not 1 <= self.max_frame <= MAX_FRAME_LIMIT:
            raise ValueError(f"max_frame must be in 1..{MAX_FRAME_LIMIT}")


def _check_policy(policy) -> None:
    if not isinstance(policy, Policy):
        raise TypeError(f"policy is a recover.Policy, not {type(policy).__name__}")


def horizon(policy: Policy) -> int:
    """``H``: a part that is not the last takes no decision in its last ``H - 1`` offsets."""
    return 2 * (4 + policy.max_frame)


def decided_end(n: int, policy: Policy, final: bool) -> int:
    """The offsets below this one are decided in a buffer of ``n`` bytes."""
    return n if final else max(0, n - horizon(policy) + 1)


def rules_of(data, policy: Policy = Policy(), dialect: str = "protobufjs") -> Tuple[Callable, Callable]:
    """``(frame_end, anchor)`` over ``data``: ``frame_end(p)`` is ``end(p)`` where ``p`` is well
    framed and 0 where it is not; ``anchor(q)`` is the resync rule."""
    _check_policy(policy)
    replay._check_dialect(dialect)
    view = memoryview(data)
    n, max_frame = len(view), policy.max_frame
    status_type, progress_type = replay._types()
    decoders = {STATUS_ID: ops.codec_for(status_type, dialect).decode,
                PROGRESS_ID: ops.codec_for(progress_type, dialect).decode}

    def frame_end(p: int) -> int:
        if p + 4 > n:
            return 0
        (length,) = struct.unpack_from("<I", view, p)
        if not 1 <= length <= max_frame or p + 4 + length > n:
            return 0
        return p + 4 + length

    def anchor(q: int) -> bool:
        end = frame_end(q)
        if not end or (end != n and not frame_end(end)):
            return False
        decode = decoders.get(view[q + 4])
        if decode is None:
            return False
        try:
            return decode(bytes(view[q + 5:end])).mediaId != ""
        except proto.DecodeError:
            return False
    return frame_end, anchor


@dataclasses.dataclass
class Recovered:
    data: bytes = b""            # the input's first ``consumed`` bytes with the gap ranges removed
    offsets: List[int] = dataclasses.field(default_factory=list)  # input offset of every recovered frame, ascending
    gaps: List[Tuple[int, int]] = dataclasses.field(default_factory=list)  # (offset, length): ascending, disjoint
    in_bytes: int = 0            # the input bytes accounted for: ``consumed``
    frames: int = 0              # len(offsets)
    anchors: int = 0             # the frames among them found by resynchronising
    consumed: int = 0            # where the walk stopped; the buffer's length for a final part
    resync: bool = False         # a gap was open there
    dialect: str = "protobufjs"
    max_frame: int = 1 << 20
    base: int = 0                # the input offset of this part's first byte; offsets and gaps include it

    @property
    def intact(self) -> bool:
        return not self.gaps

    def merge(self, later: "Recovered") -> "Recovered":
        """The result for this one's input followed by ``later``'s, which was entered with this one's
        ``resync``: concatenation, ``later``'s offsets shifted to follow this one's ``in_bytes``, and
        two gaps that touch joined. Neither operand changes."""
        if (later.dialect, later.max_frame) != (self.dialect, self.max_frame):
            raise ValueError(f"cannot merge dialect={self.dialect!r} max_frame={self.max_frame} with "
                             f"dialect={later.dialect!r} max_frame={later.max_frame}")
        shift = self.base + self.in_bytes - later.base
        gaps = list(self.gaps)
        for offset, length in later.gaps:
            offset += shift
            if gaps and gaps[-1][0] + gaps[-1][1] == offset:
                gaps[-1] = (gaps[-1][0], gaps[-1][1] + length)
            else:
                gaps.append((offset, length))
        return Recovered(self.data + later.data, self.offsets + [o + shift for o in later.offsets], gaps,
                         self.in_bytes + later.in_bytes, self.frames + later.frames, self.anchors + later.anchors,
                         self.in_bytes + later.consumed, later.resync, self.dialect, self.max_frame, self.base)


def assemble(data, offsets: List[int], gaps: List[Tuple[int, int]], anchors: int, consumed: int, resync: bool,
             policy: Policy, dialect: str, base: int = 0) -> Recovered:
    """The :class:`Recovered` of a walk's lists (local offsets): cuts the gaps out of ``data[:consumed]``.
    Between gaps the frames are contiguous, so nothing is copied frame by frame."""
    view = memoryview(data)
    parts, at = [], 0
    for offset, length in gaps:
        parts.append(view[at:offset])
        at = offset + length
    parts.append(view[at:consumed])
    return Recovered(b"".join(parts), [base + o for o in offsets], [(base + o, length) for o, length in gaps],
                     consumed, len(offsets), anchors, consumed, resync, dialect, policy.max_frame, base)


def _check_entry(final, resync, base) -> None:
    if not isinstance(final, bool) or not isinstance(resync, bool):
        raise TypeError("final and resync are bools")
    if isinstance(base, bool) or not isinstance(base, int) or base < 0:
        raise ValueError("base is an int >= 0")


def recover_cpu(data, policy: Policy = Policy(), dialect: str = "protobufjs", final: bool = True,
                resync: bool = False, base: int = 0) -> Recovered:
    """The recovered stream, written plainly: the oracle and the ``--device cpu`` path. ``base`` is
    the input offset of ``data``'s first byte."""
    frame_end, anchor = rules_of(data, policy, dialect)
    _check_entry(final, resync, base)
    n = len(data)
    stop = decided_end(n, policy, final)
    offsets, gaps = [], []
    anchors = 0
    p, gap_at = 0, (0 if resync else None)
    first = 0  # the first resync candidate of an open gap: the offset after it, or 0 on entry
    while True:
        if gap_at is None:
            if p >= stop:
                break
            end = frame_end(p)
            if end:
                offsets.append(p)
                p = end
                continue
            gap_at, first = p, p + 1
        q = next((q for q in range(first, stop) if anchor(q)), None)
        if q is None:
            p = max(gap_at, stop)
            if p > gap_at:
                gaps.append((gap_at, p - gap_at))
            break
        if q > gap_at:
            gaps.append((gap_at, q - gap_at))
        offsets.append(q)
        anchors += 1
        p, gap_at = frame_end(q), None
    return assemble(data, offsets, gaps, anchors, p, gap_at is not None, policy, dialect, base)


def recover_gpu(data, policy: Policy = Policy(), device="cuda", dialect: str = "protobufjs", final: bool = True,
                resync: bool = False, base: int = 0) -> Recovered:
    """The same :class:`Recovered` as :func:`recover_cpu`, computed on ``device``: a candidate test
    per byte offset, a reverse min-scan to the next anchor, and the walk as pointer doubling
    (``ops/gpu_recover.py``). ``data`` holds at most ``gpu_recover.LIMIT`` bytes (:func:`recover_file`
    reads less). Raises if the HIP library or the device is missing."""
    from .ops import gpu_recover
    _check_policy(policy)
    replay._check_dialect(dialect)
    _check_entry(final, resync, base)
    return gpu_recover.recover(data, policy, device=device, dialect=dialect, final=final, resync=resync, base=base)[0]


def _read_exact(f, size: int) -> bytes:
    """``size`` bytes of ``f``, fewer only at its end."""
    parts, left = [], size
    while left > 0:
        block = f.read(left)
        if not block:
            break
        parts.append(block)
        left -= len(block)
    return parts[0] if len(parts) == 1 else b"".join(parts)


def recover_file(path, out, policy: Policy = Policy(), device: str = "cpu", dialect: str = "protobufjs",
                 chunk_bytes: int = replay.DEFAULT_CHUNK_BYTES, gaps_out=None, offsets_out=None) -> dict:
    """Recover the file at ``path`` (or an open binary file) into the binary file ``out``, part by
    part: a block is read behind what the last part left undecided, the part's ``data`` is written
    before the next block is read, and ``pending[consumed:]`` and ``resync`` are carried over. It
    does not use ``replay.iter_chunks``, which raises on exactly these inputs.

    ``chunk_bytes`` is at least ``2 * H``. ``device`` is ``cpu`` or a torch device string (``gpu``
    means ``cuda``); a device is never handed more than its limit, less is read instead.
    ``gaps_out``, a text file, gets one NDJSON row per gap, ``{"offset", "length", "after_frame"}``
    with the output index of the frame before the gap, or -1; ``offsets_out`` gets the input offset
    of every recovered frame, one per line. Returns ``{in_bytes, kept_bytes, frames, anchors, gaps,
    gap_bytes, largest_gap, intact, host_offsets}``: ``host_offsets`` counts the offsets a device run
    left to the host."""
    _check_policy(policy)
    replay._check_dialect(dialect)
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, int):
        raise TypeError("chunk_bytes is an int")
    if chunk_bytes < 2 * horizon(policy):
        raise ValueError(f"--chunk-bytes {chunk_bytes} is below {2 * horizon(policy)}, four times --max-frame "
                         f"{policy.max_frame} and its header: raise --chunk-bytes or lower --max-frame")
    device = capture_io.torch_device(device)
    if device == "cpu":
        def unit(pending, final, resync, base):
            return recover_cpu(pending, policy, dialect, final, resync, base), 0
    else:
        from .ops import gpu_recover
        if gpu_recover.LIMIT < 2 * horizon(policy):
            raise ValueError(f"--max-frame {policy.max_frame} needs pieces beyond the device's {gpu_recover.LIMIT} bytes")
        chunk_bytes = min(chunk_bytes, gpu_recover.LIMIT)

        def unit(pending, final, resync, base):
            return gpu_recover.recover(pending, policy, device=device, dialect=dialect, final=final, resync=resync,
                                       base=base)
    counts = {"in_bytes": 0, "kept_bytes": 0, "frames": 0, "anchors": 0, "gaps": 0, "gap_bytes": 0, "largest_gap": 0,
              "intact": True, "host_offsets": 0}
    open_gap = None  # [offset, length, after_frame]: the last gap so far, which the next part may lengthen

    def close_gap():
        counts["gaps"] += 1
        counts["gap_bytes"] += open_gap[1]
        counts["largest_gap"] = max(counts["largest_gap"], open_gap[1])
        if gaps_out is not None:
            gaps_out.write(json.dumps({"offset": open_gap[0], "length": open_gap[1], "after_frame": open_gap[2]}) + "\n")
    with capture_io.open_source(path) as f:
        pending, resync, final = b"", False, False
        while not final:
            want = chunk_bytes - len(pending)
            block = _read_exact(f, want)
            final = len(block) < want
            pending = pending + block if pending else block
            part, host_offsets = unit(pending, final, resync, counts["in_bytes"])
            out.write(part.data)
            if offsets_out is not None:
                capture_io.write_indices(offsets_out, part.offsets)
            for offset, length in part.gaps:
                if open_gap is not None and open_gap[0] + open_gap[1] == offset:
                    open_gap[1] += length
                    continue
                if open_gap is not None:
                    close_gap()
                open_gap = [offset, length, counts["frames"] + bisect.bisect_left(part.offsets, offset) - 1]
            counts["in_bytes"] += part.consumed
            counts["kept_bytes"] += len(part.data)
            counts["frames"] += part.frames
            counts["anchors"] += part.anchors
            counts["host_offsets"] += host_offsets
            pending, resync = pending[part.consumed:], part.resync
    if open_gap is not None:
        close_gap()
    counts["intact"] = counts["gaps"] == 0
    return counts
