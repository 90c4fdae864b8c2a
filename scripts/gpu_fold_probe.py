"""Price the stream fold on the GPU against the CPU fold, stage by stage (MI355X box).

``python -m beholder_amd summarise --device gpu`` folds a captured stream with
ops/hip/telemetry_fold.hip (beholder_amd/replay.py defines the fold). This script times one stream
size and one media population per run:

* frame_index: the host's one pass over the length headers (the only per-event host work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``fold_gpu`` does it;
* pass_a / pass_b: decode + hash + count, and grouping by mediaId (HIP events, tables zeroed outside);
* collect: compaction with torch on the device plus the copy back;
* finish: id strings and the Summary on the host;
* fold_gpu_wall: the whole of ``gpu_fold.fold`` as the command runs it, allocation included.

It checks the result against ``replay.fold_cpu``, times that too, and compares both with
59 ns/message, the CPU decode cost on record in docs/DESIGN.md: the floor any CPU fold pays.

Usage: ``gpu_fold_probe.py --events 262144 --media 10000`` (sizes on record: 16k, 262k and 4M events;
16 media, where every atomic lands on 16 groups, and 10,000). Output: one JSON object (stdout).
docs/DESIGN.md "The fold: where the device does win" cites it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from beholder_amd import replay  # noqa: E402
from beholder_amd.bench.generator import Workload  # noqa: E402
from beholder_amd.ops import gpu_fold  # noqa: E402

CPU_DECODE_NS = 59.0  # docs/DESIGN.md, the offload table's cpu_decode_ns


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", type=int, default=262_144)
    ap.add_argument("--media", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    dev = "cuda:0"
    w = Workload(n_media=a.media, seed=1)
    data = b"".join(w.framed(min(65536, a.events - k)) for k in range(0, a.events, 65536))
    n_events = a.events
    mask = gpu_fold.known_mask(replay.status_names())
    sync = torch.cuda.synchronize

    cpu_s, want = timed(lambda: replay.fold_cpu(data))
    wall_cold, (got, host_frames) = timed(lambda: gpu_fold.fold(data, dev))  # loads the module: not a figure
    assert got == want, "the GPU fold disagrees with fold_cpu"

    best = {}

    def keep(name, seconds):
        best[name] = min(best.get(name, seconds), seconds)

    for _ in range(a.reps):
        t, (n, offs) = timed(lambda: gpu_fold.index(data))
        keep("frame_index", t)

        def h2d():
            out = gpu_fold.upload(data, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        tables = gpu_fold.allocate(buf, offs_dev, n)
        sync()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        gpu_fold.launch(tables, "protobufjs", mask, passes=1)
        e[1].record()
        gpu_fold.launch(tables, "protobufjs", mask, passes=2)
        e[2].record()
        e[2].synchronize()
        keep("pass_a", e[0].elapsed_time(e[1]) * 1e-3)
        keep("pass_b", e[1].elapsed_time(e[2]) * 1e-3)
        t, collected = timed(lambda: gpu_fold.collect(tables))
        keep("collect", t)
        t, summary = timed(lambda: gpu_fold.finish(data, offs, n, collected))
        keep("finish", t)
        assert summary == want
        del tables, buf, offs_dev
        t, _ = timed(lambda: gpu_fold.fold(data, dev))
        keep("fold_gpu_wall", t)

    stages = ("frame_index", "h2d", "pass_a", "pass_b", "collect", "finish")
    total = sum(best[s] for s in stages)
    out = {
        "device": torch.cuda.get_device_name(0), "events": n_events, "media": a.media, "bytes": len(data),
        "groups": len(want.media), "host_frames": host_frames,
        "stages_us": {s: round(best[s] * 1e6, 1) for s in stages},
        "stages_ns_per_event": {s: round(best[s] / n_events * 1e9, 2) for s in stages},
        "stage_sum_ns_per_event": round(total / n_events * 1e9, 2),
        "fold_gpu_wall_ms": round(best["fold_gpu_wall"] * 1e3, 3),
        "fold_gpu_wall_ns_per_event": round(best["fold_gpu_wall"] / n_events * 1e9, 2),
        "fold_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "fold_cpu_ms": round(cpu_s * 1e3, 1),
        "fold_cpu_ns_per_event": round(cpu_s / n_events * 1e9, 1),
        "cpu_decode_floor_ns_per_event": CPU_DECODE_NS,
        "wall_vs_fold_cpu": round(best["fold_gpu_wall"] / cpu_s, 4),
        "wall_vs_cpu_decode_floor": round(best["fold_gpu_wall"] / n_events * 1e9 / CPU_DECODE_NS, 3),
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
