"""The plumbing every ``ops/gpu_*.py`` shares (ops/hip_lib.py), without a GPU and without the
library: the launch helper against a stand-in for the library and for torch, and the mask check."""
from __future__ import annotations

import contextlib
import sys
import types

import pytest

from beholder_amd.ops import hip_lib

STREAM = 0x5EED


class _Anchor:
    device = "cuda:1"


def _stand_ins(monkeypatch, returns: int):
    """A library whose every entry point records its arguments and returns ``returns``, and a torch
    whose current stream is ``STREAM`` inside ``torch.cuda.device(...)`` and nowhere else."""
    seen = types.SimpleNamespace(calls=[], devices=[], inside=False)

    class Library:
        def __getattr__(self, name):
            def entry(*args):
                seen.calls.append((name, args))
                return returns
            return entry

    @contextlib.contextmanager
    def device(dev):
        seen.devices.append(dev)
        seen.inside = True
        try:
            yield
        finally:
            seen.inside = False

    def current_stream():
        assert seen.inside, "the stream is looked up under the anchor's device"
        return types.SimpleNamespace(cuda_stream=STREAM)

    torch = types.SimpleNamespace(cuda=types.SimpleNamespace(device=device, current_stream=current_stream))
    monkeypatch.setitem(sys.modules, "torch", torch)
    library = Library()
    monkeypatch.setattr(hip_lib, "lib", lambda: library)
    return seen


def test_call_passes_the_stream_last(monkeypatch):
    seen = _stand_ins(monkeypatch, 0)
    assert hip_lib.call("bh_some_entry", _Anchor(), 1, 2, 3) is None
    assert seen.calls == [("bh_some_entry", (1, 2, 3, STREAM))]
    assert seen.devices == ["cuda:1"] and not seen.inside
    hip_lib.call("bh_no_arguments", _Anchor())
    assert seen.calls[-1] == ("bh_no_arguments", (STREAM,))


def test_call_raises_for_a_hip_error(monkeypatch):
    seen = _stand_ins(monkeypatch, 719)
    with pytest.raises(RuntimeError) as err:
        hip_lib.call("bh_some_entry", _Anchor(), 1)
    assert str(err.value) == "bh_some_entry launch failed: hipError 719"
    assert seen.calls == [("bh_some_entry", (1, STREAM))]


def test_check_hash_mask():
    assert hip_lib.check_hash_mask(None) == hip_lib.ALL_ONES == 2 ** 64 - 1
    assert hip_lib.check_hash_mask(0) == 0
    assert hip_lib.check_hash_mask(hip_lib.ALL_ONES) == hip_lib.ALL_ONES
    assert hip_lib.check_hash_mask(0x3) == 0x3
    for bad in (-1, 1 << 64, True, False, 1.0, "3"):
        with pytest.raises(ValueError):
            hip_lib.check_hash_mask(bad)
