"""What every capture command's ``*_file`` function shares: opening the source, naming the device,
the framing walk, the per-chunk callable, the chunk loop and the index lines.

Plain functions over the standard library alone: neither ``replay`` nor torch is imported here, so
the command modules and ``replay`` itself can all build on it. What is a command's own stays in its
module: its counters, its cross-chunk state and what it does with a chunk's part.
"""
from __future__ import annotations

import contextlib
import struct
from typing import Callable, Iterator, Tuple


@contextlib.contextmanager
def open_source(source):
    """The open binary file of ``source``: a path (``str``, ``bytes``, ``os.PathLike``) is opened and
    closed again; an open file is passed through and left open."""
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        with open(source, "rb") as f:
            yield f
    else:
        yield source


def torch_device(device: str) -> str:
    """The torch device string of a ``--device`` value: ``gpu`` means ``cuda``."""
    return "cuda" if device == "gpu" else device


def frame_spans(data) -> Iterator[Tuple[int, int]]:
    """``(start, end)`` of every frame of a framed stream. Raises ``ValueError`` for broken framing,
    as ``iter_frames`` does."""
    view = memoryview(data)
    i, n = 0, len(view)
    while i < n:
        if n - i < 4:
            raise ValueError("truncated frame header")
        (length,) = struct.unpack_from("<I", view, i)
        if length == 0 or n - i - 4 < length:
            raise ValueError("truncated or empty frame")
        yield i, i + 4 + length
        i += 4 + length


def per_chunk(device: str, on_cpu: Callable, on_device: Callable) -> Callable:
    """``cut(chunk) -> (part, host_frames)`` for ``device``. On ``cpu`` that is ``on_cpu(chunk)`` and no
    host frames. For any other device it is what ``on_device(torch device string)`` returns: the
    caller imports its ``ops.gpu_*`` module in there, so a CPU run never loads it."""
    device = torch_device(device)
    if device == "cpu":
        return lambda chunk: (on_cpu(chunk), 0)
    return on_device(device)


def with_chunk_bytes_hint(too_large, cut: Callable) -> Callable:
    """``cut``, with the device's ``too_large`` reworded into a ``ValueError`` that names the way out."""
    def hinted(chunk):
        try:
            return cut(chunk)
        except too_large as e:
            raise ValueError(f"{e}; cut smaller pieces with --chunk-bytes") from None
    return hinted


def chunk_parts(f, chunk_bytes: int, chunker: Callable, cut: Callable):
    """``(chunk, part, host_frames)`` of every piece that ``chunker(f, chunk_bytes)`` cuts from the
    open file ``f`` (``replay.iter_chunks``, or ``import_rows.iter_line_chunks``), one at a time:
    the next piece is read when the caller comes back for it."""
    for chunk in chunker(f, chunk_bytes):
        part, host_frames = cut(chunk)
        yield chunk, part, host_frames


def write_indices(f, indices, base: int = 0) -> None:
    """``base + i`` for every ``i`` of ``indices`` to the text file ``f``, one per line, in one write
    (an empty one where there are none)."""
    f.write("".join(f"{base + i}\n" for i in indices))
