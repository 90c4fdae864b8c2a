"""Put two framed streams side by side: which frames are in both, which only in one, and whether
the common ones come in the same order.

Every other capture command takes one capture. The questions an operator has afterwards take two:
"I published A and recorded what the consumers got as B: what was lost, what was redelivered?", "I
sharded A into N files: do they together hold exactly A's frames?", "what did ``thin`` remove, and
is the rest still in order?". :func:`compare_cpu` answers them and is the definition;
:func:`compare_gpu` computes the same :class:`Comparison` on the device
(``ops/hip/telemetry_compare.hip``, ``ops/gpu_compare.py``).

A frame's **content** is the dedupe's: its topic byte and body. Nothing is decoded, so there is no
dialect, and two encodings of one event are two contents (:mod:`beholder_amd.normalise`, run first on
both captures, gives every event one encoding). With ``topics`` only frames of those topic bytes
take part; every other frame is **skipped**: it is counted, it is in neither output, and it equals
nothing.

The comparison is of **multisets**, not of sets. Content cannot tell "the same event again" from
"the same state reached again" (two reports of one progress percentage are equal frames), so a set
difference would let one ``progress 40%`` in B erase both ``progress 40%`` frames of A. Here the
occurrences are paired instead. For a content that occurs at ``a_0 < a_1 < ...`` in A and at
``b_0 < b_1 < ...`` in B:

* frame ``a_k`` is **matched** with ``b_k`` for every ``k < min(|a|, |b|)``;
* every other participating frame of A is **only in A**, and likewise for B.

Two in A and one in B leave one in "only in A", and nothing is claimed about why. The surplus
occurrences are the *last* ones: under at-least-once delivery those are the redelivered copies.

``order_breaks``: take A's matched frames in A's order; each has a partner index in B. The number
of matched frames whose partner lies before the previous matched frame's partner (adjacent
descents) is ``order_breaks``. It is 0 iff the common frames come in the same order in both captures.

The definition is symmetric: ``compare(b, a)`` is ``compare(a, b)`` with the sides swapped. The one
field that is counted from A's side is ``order_breaks``: a permutation and its inverse need not have
equally many adjacent descents (``2 4 1 3`` has one, its inverse ``3 1 4 2`` two), so swapped it may
be another number, but it is 0 on both sides or on neither.
"""
from __future__ import annotations

import dataclasses
import os
from typing import FrozenSet, List, Optional

from . import capture_io
from .capture_io import frame_spans

SHARD_ROUTE = ("shard both captures with the same `shard --shards N` and compare shard by shard: "
               "equal contents land in equal shard numbers, so the per-shard counts add up exactly")


@dataclasses.dataclass(frozen=True)
class Policy:
    """The topic bytes whose frames take part (``None``: all of them)."""
    topics: Optional[FrozenSet[int]] = None

    def __post_init__(self):
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
        raise TypeError(f"policy is a compare.Policy, not {type(policy).__name__}")


@dataclasses.dataclass
class Side:
    data: bytes = b""            # the frames only in this capture, headers included, in stream order
    indices: List[int] = dataclasses.field(default_factory=list)  # their indices in this capture, ascending
    frames: int = 0              # this capture's frame count
    skipped: int = 0             # its frames that do not take part
    distinct: int = 0            # its distinct participating contents


@dataclasses.dataclass
class Comparison:
    a: Side = dataclasses.field(default_factory=Side)
    b: Side = dataclasses.field(default_factory=Side)
    matched: int = 0             # the number of pairs
    common: int = 0              # the contents that occur on both sides
    order_breaks: int = 0        # matched frames of A whose partner lies before the previous one's
    topics: Optional[FrozenSet[int]] = None

    @property
    def equal(self) -> bool:
        """Both captures hold the same participating frames, each as often: nothing is only in one."""
        return not self.a.indices and not self.b.indices

    def counts(self, host_frames: int = 0) -> dict:
        """What :func:`compare_file` returns and the command prints."""
        return {"frames_a": self.a.frames, "frames_b": self.b.frames,
                "skipped_a": self.a.skipped, "skipped_b": self.b.skipped, "matched": self.matched,
                "only_a": len(self.a.indices), "only_b": len(self.b.indices),
                "only_a_bytes": len(self.a.data), "only_b_bytes": len(self.b.data),
                "distinct_a": self.a.distinct, "distinct_b": self.b.distinct, "distinct_common": self.common,
                "order_breaks": self.order_breaks, "equal": self.equal, "host_frames": host_frames}


def order_breaks(partners) -> int:
    """Adjacent descents of ``partners``, the partner index of every matched frame in its own side's order."""
    return sum(1 for p, q in zip(partners, partners[1:]) if q < p)


def _occurrences(view, spans, policy: Policy) -> dict:
    """content -> its frames' indices, ascending, over the frames that take part."""
    where = {}
    for i, (a, b) in enumerate(spans):
        if policy.takes_part(view[a + 4]):
            where.setdefault(bytes(view[a + 4:b]), []).append(i)
    return where


def _spans_of(data, side: str):
    view = memoryview(data)
    try:
        return view, list(frame_spans(view))
    except ValueError as e:
        raise ValueError(f"capture {side}: {e}") from None


def compare_cpu(a, b, policy: Policy = Policy()) -> Comparison:
    """The comparison, written plainly: the oracle and the ``--device cpu`` path. Raises
    ``ValueError`` for broken framing and names the side."""
    _check_policy(policy)
    view_a, spans_a = _spans_of(a, "A")
    view_b, spans_b = _spans_of(b, "B")
    in_a = _occurrences(view_a, spans_a, policy)
    in_b = _occurrences(view_b, spans_b, policy)
    partner = {}  # a matched frame of A -> its partner in B
    only_a, only_b = [], []
    for content, mine in in_a.items():
        theirs = in_b.get(content, ())
        pairs = min(len(mine), len(theirs))
        partner.update(zip(mine[:pairs], theirs[:pairs]))
        only_a.extend(mine[pairs:])
    for content, theirs in in_b.items():
        only_b.extend(theirs[len(in_a.get(content, ())):])
    only_a.sort()
    only_b.sort()

    def side(view, spans, only, where) -> Side:
        taking_part = sum(map(len, where.values()))
        return Side(b"".join(view[spans[i][0]:spans[i][1]] for i in only), only, len(spans),
                    len(spans) - taking_part, len(where))
    return Comparison(side(view_a, spans_a, only_a, in_a), side(view_b, spans_b, only_b, in_b), len(partner),
                      sum(1 for content in in_a if content in in_b),
                      order_breaks([partner[i] for i in sorted(partner)]), policy.topics)


def compare_gpu(a, b, policy: Policy = Policy(), device="cuda", hash_mask: Optional[int] = None) -> Comparison:
    """The same :class:`Comparison` as :func:`compare_cpu`, computed on ``device``: the host indexes
    both captures' frame headers, the device hashes every frame's content, groups equal contents of
    both captures in one table whose key compare walks the bytes, sorts the frames by content,
    pairs the k-th occurrence on one side with the k-th on the other, counts the order breaks and
    gathers each side's unmatched frames (``ops/gpu_compare.py``). The two captures together must be
    below 2^31 bytes. Raises if the HIP library or the device is missing."""
    from .ops import gpu_compare
    return gpu_compare.compare(a, b, policy, device=device, hash_mask=hash_mask)[0]


def _read(path) -> bytes:
    with capture_io.open_source(path) as f:
        return f.read()


def device_limit_error(bytes_a: int, bytes_b: int, frames: Optional[int] = None) -> Optional[str]:
    """Why two captures of these sizes do not fit one device comparison, or None where they do."""
    from .ops.gpu_transitions import MAX_SLOTS
    if bytes_a + bytes_b >= 2 ** 31:
        return (f"the two captures hold {bytes_a + bytes_b} bytes together and the device compares below 2^31: "
                + SHARD_ROUTE)
    if frames is not None and frames > MAX_SLOTS // 2:
        return (f"the two captures hold {frames} frames together and the device's table takes {MAX_SLOTS // 2}: "
                + SHARD_ROUTE)
    return None


def compare_file(path_a, path_b, only_a_out=None, only_b_out=None, policy: Policy = Policy(), device: str = "cpu",
                 indices_a_out=None, indices_b_out=None) -> dict:
    """Compare the files at ``path_a`` and ``path_b`` (or open binary files); the frames only in A go
    to the binary file ``only_a_out``, those only in B to ``only_b_out``, their indices in their own
    capture to the text files ``indices_a_out`` and ``indices_b_out``, one per line. Each of the four
    may be ``None``.

    Both captures are read whole. There is no chunking, because a comparison does not merge from
    parts: whether a frame of A's first chunk is matched depends on every chunk of B, and
    ``order_breaks`` on the pairs across all of them. It does not need to, either: ``shard_of``
    depends on the mediaId alone, so ``shard --shards N`` of A and of B with the same ``N`` puts equal
    contents into equal shard numbers (undecoded frames go to shard 0 on both sides), and comparing
    shard by shard is exact: every count but ``order_breaks`` is the sum of the shards'. On the
    device A and B together must stay below 2^31 bytes and their frames must fit the table of
    ``gpu_transitions.MAX_SLOTS`` slots; beyond either, ``ValueError`` names that route.

    ``device`` is ``cpu`` or a torch device string (``gpu`` means ``cuda``). Broken framing raises
    ``ValueError``, names the side and writes nothing.
    Returns ``{frames_a, frames_b, skipped_a, skipped_b, matched, only_a, only_b, only_a_bytes,
    only_b_bytes, distinct_a, distinct_b, distinct_common, order_breaks, equal, host_frames}``;
    ``host_frames`` counts the frames a device run left to the host."""
    _check_policy(policy)
    device = capture_io.torch_device(device)
    if device != "cpu":
        sizes = []
        for path in (path_a, path_b):
            if isinstance(path, (str, bytes)) or hasattr(path, "__fspath__"):
                sizes.append(os.path.getsize(path))
        if len(sizes) == 2:  # known before either is read
            error = device_limit_error(*sizes)
            if error:
                raise ValueError(error)
    a, b = _read(path_a), _read(path_b)
    if device == "cpu":
        result, host_frames = compare_cpu(a, b, policy), 0
    else:
        from .ops import gpu_compare
        result, host_frames = gpu_compare.compare(a, b, policy, device=device)
    for side, out, indices_out in ((result.a, only_a_out, indices_a_out), (result.b, only_b_out, indices_b_out)):
        if out is not None:
            out.write(side.data)
        if indices_out is not None:
            capture_io.write_indices(indices_out, side.indices)
    return result.counts(host_frames)
