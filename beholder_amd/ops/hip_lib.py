"""The gfx950 extension (``ops/hip/libbeholder_hip.so``) as Python sees it: where it lies, how it is
loaded, and what its callers share: the launch helper, the argument checks and the reader of the
overflow list (``ops/gpu_decode.py``, ``ops/gpu_fold.py``, ``ops/gpu_extract.py``,
``ops/gpu_coalesce.py``, ``ops/gpu_shard.py``, ``ops/gpu_dedupe.py``, ``ops/gpu_transitions.py``,
``ops/gpu_thin.py``, ``ops/gpu_hosts.py``, ``ops/gpu_stages.py``, ``ops/gpu_normalise.py``,
``ops/gpu_compare.py``, ``ops/gpu_export.py``, ``ops/gpu_anonymise.py``, ``ops/gpu_import.py``,
``ops/gpu_recover.py``, and ``ops/gpu_rewrite.py`` for what the rewriting four of them share).

The library is built in-tree by ``beholder_amd._build.build_hip`` (hipcc, gfx950) and loaded with
ctypes after ``import torch``. torch's HIP runtime has the same soname, so the kernels launch on
torch's runtime and stream. A missing library raises; there is no CPU fallback behind it.
"""
from __future__ import annotations

import ctypes
import os

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip", "libbeholder_hip.so")
DIALECT_IDS = {"upb": 0, "protobufjs": 1}  # DIALECT_* of hip/telemetry_readers.hpp
ALL_ONES = 0xFFFFFFFFFFFFFFFF
_lib = None


def lib() -> ctypes.CDLL:
    """The HIP extension with its entry points declared (raises if it was not built: no silent
    fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m beholder_amd.ops.build`")
        import torch  # noqa: F401  load torch's libamdhip64 first so the kernels share its runtime
        so = ctypes.CDLL(LIB_PATH)
        p, i = ctypes.c_void_p, ctypes.c_int
        so.bh_decode_telemetry.argtypes = [p, p, i, p, i, p]
        so.bh_decode_telemetry.restype = i
        so.bh_fold_telemetry.argtypes = [p, p, i, i, ctypes.c_ulonglong, ctypes.c_ulonglong] + [p] * 6 + \
                                        [ctypes.c_longlong, i, p]
        so.bh_fold_telemetry.restype = i
        # telemetry_select.hip (ops/gpu_extract.py): mark, scan, gather
        so.bh_select_mark.argtypes = [p, p, i, i] + [p] * 7
        so.bh_select_mark.restype = i
        so.bh_select_scan.argtypes = [p, i] + [p] * 6
        so.bh_select_scan.restype = i
        so.bh_select_gather.argtypes = [p, p, i, p, p, p, p, i, i, p, i, p]
        so.bh_select_gather.restype = i
        # telemetry_coalesce.hip (ops/gpu_coalesce.py): classify, claim, mark
        so.bh_coalesce_mark.argtypes = [p, p, i, i] + [p] * 9 + [i, p]
        so.bh_coalesce_mark.restype = i
        # telemetry_shard.hip (ops/gpu_shard.py): route, partition
        so.bh_shard_route.argtypes = [p, p, i, i] + [p] * 5
        so.bh_shard_route.restype = i
        so.bh_shard_partition.argtypes = [p, p, i, i] + [p] * 6 + [i, i, p]
        so.bh_shard_partition.restype = i
        # telemetry_dedupe.hip (ops/gpu_dedupe.py): hash, claim, mark
        so.bh_dedupe_mark.argtypes = [p, p, i] + [p] * 8 + [i, p]
        so.bh_dedupe_mark.restype = i
        # telemetry_transitions.hip (ops/gpu_transitions.py): classify, claim, compact, sort pass, pairs
        so.bh_transitions_classify.argtypes = [p, p, i, i] + [p] * 5
        so.bh_transitions_classify.restype = i
        so.bh_transitions_claim.argtypes = [p, p, i, ctypes.c_ulonglong, p, p, p, ctypes.c_longlong, p]
        so.bh_transitions_claim.restype = i
        so.bh_transitions_compact.argtypes = [p] * 4 + [i, p, p, p]
        so.bh_transitions_compact.restype = i
        so.bh_transitions_sort_pass.argtypes = [p, p, i, i] + [p] * 4 + [i, p]
        so.bh_transitions_sort_pass.restype = i
        so.bh_transitions_pairs.argtypes = [p, p, i, i, ctypes.c_ulonglong] + [p] * 7
        so.bh_transitions_pairs.restype = i
        # telemetry_thin.hip (ops/gpu_thin.py): classify, mark
        so.bh_thin_classify.argtypes = [p, p, i, i, i] + [p] * 7
        so.bh_thin_classify.restype = i
        so.bh_thin_mark.argtypes = [p, p, i, i, i] + [p] * 4
        so.bh_thin_mark.restype = i
        # telemetry_hosts.hip (ops/gpu_hosts.py): classify, number, pairs, walk
        so.bh_hosts_classify.argtypes = [p, p, i, i] + [p] * 7
        so.bh_hosts_classify.restype = i
        so.bh_hosts_number.argtypes = [p, i, i, p, p, ctypes.c_longlong] + [p] * 4
        so.bh_hosts_number.restype = i
        so.bh_hosts_pairs.argtypes = [p, p, i, ctypes.c_ulonglong, p, p, p, ctypes.c_longlong, p]
        so.bh_hosts_pairs.restype = i
        so.bh_hosts_walk.argtypes = [p, p, p, p, i, i, i, ctypes.c_ulonglong] + [p] * 4
        so.bh_hosts_walk.restype = i
        # telemetry_stages.hip (ops/gpu_stages.py): classify, carry, settle
        so.bh_stages_classify.argtypes = [p, p, i, i] + [p] * 6
        so.bh_stages_classify.restype = i
        so.bh_stages_carry.argtypes = [p, p, i, i] + [p] * 8
        so.bh_stages_carry.restype = i
        so.bh_stages_settle.argtypes = [p] * 6 + [i, i, ctypes.c_ulonglong] + [p] * 4
        so.bh_stages_settle.restype = i
        # telemetry_normalise.hip (ops/gpu_normalise.py): classify, emit
        so.bh_normalise_classify.argtypes = [p, p, i, i, i] + [p] * 5
        so.bh_normalise_classify.restype = i
        so.bh_normalise_emit.argtypes = [p, p, i] + [p] * 5
        so.bh_normalise_emit.restype = i
        # telemetry_compare.hip (ops/gpu_compare.py): classify, bounds, match, breaks
        so.bh_compare_classify.argtypes = [p, p, i, i] + [p] * 9
        so.bh_compare_classify.restype = i
        so.bh_compare_bounds.argtypes = [p, p, i, i] + [p] * 4
        so.bh_compare_bounds.restype = i
        so.bh_compare_match.argtypes = [p, p, i, i, p, i] + [p] * 9
        so.bh_compare_match.restype = i
        so.bh_compare_breaks.argtypes = [p, i, p, i, p, p]
        so.bh_compare_breaks.restype = i
        # telemetry_export.hip (ops/gpu_export.py): classify, emit
        so.bh_export_classify.argtypes = [p, p, i, i, i, ctypes.c_longlong] + [p] * 5
        so.bh_export_classify.restype = i
        so.bh_export_emit.argtypes = [p, i, ctypes.c_longlong] + [p] * 4
        so.bh_export_emit.restype = i
        # telemetry_anonymise.hip (ops/gpu_anonymise.py): classify (the key is host memory), emit
        so.bh_anonymise_classify.argtypes = [p, p, i, i, i, i, ctypes.c_char_p, i] + [p] * 5
        so.bh_anonymise_classify.restype = i
        so.bh_anonymise_emit.argtypes = [p, i] + [p] * 4
        so.bh_anonymise_emit.restype = i
        # telemetry_import.hip (ops/gpu_import.py): count, starts, classify, emit
        so.bh_import_count.argtypes = [p, ctypes.c_longlong, p, p]
        so.bh_import_count.restype = i
        so.bh_import_starts.argtypes = [p, ctypes.c_longlong, p, i, p, p]
        so.bh_import_starts.restype = i
        so.bh_import_classify.argtypes = [p, p, i] + [p] * 5
        so.bh_import_classify.restype = i
        so.bh_import_emit.argtypes = [p, i] + [p] * 4
        so.bh_import_emit.restype = i
        # telemetry_recover.hip (ops/gpu_recover.py): candidates, next, reach, mark, resolve
        so.bh_recover_candidates.argtypes = [p, ctypes.c_longlong, i, i, i, i] + [p] * 5
        so.bh_recover_candidates.restype = i
        so.bh_recover_next.argtypes = [p, p, i, i] + [p] * 5
        so.bh_recover_next.restype = i
        so.bh_recover_reach.argtypes = [p] * 4 + [i, i, p]
        so.bh_recover_reach.restype = i
        so.bh_recover_mark.argtypes = [p, i, i, p, p]
        so.bh_recover_mark.restype = i
        so.bh_recover_resolve.argtypes = [p, i] + [p] * 5
        so.bh_recover_resolve.restype = i
        _lib = so
    return _lib


def call(name: str, anchor, *args) -> None:
    """Launches entry point ``name`` with ``args`` and, as its last argument, the current torch
    stream of ``anchor``'s device (a tensor the kernels read or write). ``RuntimeError`` for a
    ``hipError_t`` that is not 0."""
    import torch
    entry = getattr(lib(), name)
    with torch.cuda.device(anchor.device):
        err = entry(*args, torch.cuda.current_stream().cuda_stream)
    if err:
        raise RuntimeError(f"{name} launch failed: hipError {err}")


def require_gpu(device, what: str) -> None:
    """``ValueError`` where ``device`` is no GPU; ``what`` names the entry point."""
    import torch
    if torch.device(device).type != "cuda":
        raise ValueError(f"{what} needs a GPU device, not {device!r}")


def check_hash_mask(hash_mask) -> int:
    """The 64-bit mask the kernels AND onto every hash: all ones for ``None``, else an ``int`` (no
    ``bool``) in ``0 .. 2**64 - 1``."""
    if hash_mask is None:
        return ALL_ONES
    if isinstance(hash_mask, bool) or not isinstance(hash_mask, int) or not 0 <= hash_mask <= ALL_ONES:
        raise ValueError("hash_mask is 64-bit")
    return hash_mask


def check_dialect(dialect: str) -> int:
    """The kernels' number for ``dialect``; ``ValueError`` for one they do not read."""
    if dialect not in DIALECT_IDS:
        raise ValueError(f"unknown dialect {dialect!r} ({'|'.join(DIALECT_IDS)})")
    return DIALECT_IDS[dialect]


def check_device_tensors(buf_dev, offs_dev, n: int) -> None:
    """What both kernels need of their input: a uint8 ``buf_dev`` and the int32 ``offs_dev`` of
    ``n + 1`` boundaries, contiguous and on one GPU."""
    import torch
    if buf_dev.dtype != torch.uint8 or offs_dev.dtype != torch.int32 or offs_dev.numel() != n + 1:
        raise ValueError("the kernels need a uint8 buf and int32 offs of n + 1")
    if not (buf_dev.is_cuda and offs_dev.is_cuda and buf_dev.is_contiguous() and offs_dev.is_contiguous()
            and buf_dev.device == offs_dev.device):
        raise ValueError("the kernels need contiguous tensors on one device")


def check_stream(buf_dev, offs_dev, n: int, what: str) -> None:
    """What every command over a framed stream needs before it allocates: :func:`check_device_tensors`,
    at least one frame, and a stream that int32 offsets reach. ``what`` names the command."""
    check_device_tensors(buf_dev, offs_dev, n)
    if n < 1:
        raise ValueError(f"{what} needs n >= 1")
    if buf_dev.numel() >= 2 ** 31:
        raise ValueError("stream too large for int32 offsets")


def overflow_frames(overflow, count: int, data, offs):
    """The frames the device left to the host: ``(frames, events)``, the first ``count`` entries of
    the device's ``overflow`` list as a sorted int array, and an iterator of ``(frame, topic, body)``
    over them from the host's own copy of the stream."""
    import numpy as np
    frames = np.sort(overflow[:count].cpu().numpy())
    view = memoryview(data)

    def events():
        for i in frames.tolist():
            a, b = int(offs[i]), int(offs[i + 1])
            yield i, view[a + 4], bytes(view[a + 5:b])
    return frames, events()
