"""Price ``shard`` on the GPU against the CPU shard and the extract's scan, stage by stage (MI355X box).

``python -m beholder_amd shard --device gpu`` splits a captured stream by media into N streams with
ops/hip/telemetry_shard.hip (beholder_amd/shard.py defines the result). This script times, for each
stream size, each stream and each shard count, under ``undecoded=first``:

* frame_index: the host's one pass over the length headers (the only per-event host work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``shard_gpu`` does it;
* route: the kernel that decides every frame's shard, by HIP events;
* host_decide: the overflow count read back, and the host's decisions where there are any;
* count / totals / apply: the three launches of the partition, by HIP events, each a launch of its
  own; apply once per in-block method (``apply_walk``, ``apply_ballot``);
* boundaries: the ``shards + 1`` words read back, the last of which sizes the output;
* gather_walk / gather_search: the extract's copy over the partition's arrays, both shapes;
* d2h: the output bytes and the indices back to the host, split into shards;
* shard_gpu_wall: the whole of ``gpu_shard.shard`` as the command runs it, allocation included.

The yardsticks: ``shard_cpu`` on the same input, and the extract's ``scan`` and ``gather`` over the
same stream with every frame kept (``x_scan``, ``x_gather_walk``, ``x_gather_search``): the
partition does S-way what that scan does one-way.

Streams: Workload events over 10,000 media, and ``corpus``, the fold corpus mix
(tests/telemetry_corpus.py ``fold_corpus``, repeated up to the stream size), which has malformed
bodies and non-ASCII ids that go to the host. Every run is checked for equality with ``shard_cpu``.

Usage: ``gpu_shard_probe.py [--events 16384,262144,4194304] [--shards 2,8,64,256] [--out profiles/box_shard/probe.jsonl]``.
Output: one JSON object per (size, stream, shards) on stdout and appended to ``--out``.
docs/DESIGN.md "The shard" cites it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # telemetry_corpus

import torch  # noqa: E402

from beholder_amd.bench.generator import Workload  # noqa: E402
from beholder_amd.extract import Selector  # noqa: E402
from beholder_amd.ops import gpu_extract as gx, gpu_fold, gpu_shard as gs  # noqa: E402
from beholder_amd.shard import Policy, Sharded, shard_cpu  # noqa: E402
from beholder_amd.transport.framing import iter_frames  # noqa: E402

STAGES = ("frame_index", "h2d", "route", "host_decide", "count", "totals", "apply", "boundaries", "gather", "d2h")
YARDSTICKS = ("x_scan", "x_gather_walk", "x_gather_search")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def corpus_stream(events: int) -> bytes:
    from beholder_amd.ops import frame
    from telemetry_corpus import fold_corpus
    pieces = [frame(t, b) for t, b in iter_frames(fold_corpus())]
    reps = -(-events // len(pieces))
    return b"".join((pieces * reps)[:events])


def between(fn):
    """Seconds of device time that ``fn``'s launches take, by HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def extract_yardsticks(data: bytes, reps: int, dev: str) -> dict:
    """The extract's scan and both gathers over ``data`` with every frame kept."""
    best = {}
    n, offs = gpu_fold.index(data)
    buf, offs_dev = gpu_fold.upload(data, offs, dev)
    table, blob = gx.build_media_table([])
    t = gx.allocate(buf, offs_dev, n, table, blob)
    gx.mark(t, gx.select_params(Selector(), len(table)))
    gx.decide_on_host(t, data, offs, Selector())
    torch.cuda.synchronize()
    for _ in range(reps + 1):  # the first loads the kernels
        seconds, _ = between(lambda: gx.scan(t))
        best["x_scan"] = min(best.get("x_scan", seconds), seconds)
        kept, kept_bytes = gx.totals(t)
        assert kept == n and kept_bytes == len(data)
        for shape in ("walk", "search"):
            seconds, out = between(lambda: gx.gather(t, kept, kept_bytes, shape))
            best[f"x_gather_{shape}"] = min(best.get(f"x_gather_{shape}", seconds), seconds)
            del out
    return best


def probe(data: bytes, policy: Policy, label: str, events: int, reps: int, dev: str, yard: dict) -> dict:
    sync = torch.cuda.synchronize
    cpu_s, want = timed(lambda: shard_cpu(data, policy))
    wall_cold, (got, host_frames) = timed(lambda: gs.shard(data, policy, dev))  # loads the module: not a figure
    assert got == want, "the GPU shard disagrees with shard_cpu"
    best = {}

    def keep(name, seconds):
        best[name] = min(best.get(name, seconds), seconds)

    for _ in range(reps):
        t, (n, offs) = timed(lambda: gpu_fold.index(data))
        keep("frame_index", t)

        def h2d():
            out = gpu_fold.upload(data, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        tables = gs.allocate(buf, offs_dev, n, policy.shards)
        params = gs.shard_params(policy)
        sync()
        keep("route", between(lambda: gs.route(tables, params))[0])
        t, _ = timed(lambda: gs.decide_on_host(tables, data, offs, policy))
        keep("host_decide", t)
        keep("count", between(lambda: gs.partition(tables, stages=gs.STAGE_COUNT))[0])
        keep("totals", between(lambda: gs.partition(tables, stages=gs.STAGE_TOTALS))[0])
        for method in gs.METHODS:  # both write the same arrays
            keep(f"apply_{method}", between(lambda: gs.partition(tables, method, gs.STAGE_APPLY))[0])
        t, (first, starts) = timed(lambda: gs.boundaries(tables))
        keep("boundaries", t)
        kept, kept_bytes = int(first[-1]), int(starts[-1])
        for shape in ("search", "walk"):
            t, out = between(lambda: gx.gather(tables.select, kept, kept_bytes, shape))
            keep(f"gather_{shape}", t)
            t, (out_data, indices) = timed(lambda: gs.collect(tables, out, first, starts))
            keep("d2h", t)
            assert Sharded(policy.shards, out_data, indices, n) == want, shape
        del tables, buf, offs_dev, out
        for method in gs.METHODS:
            t, (again, _) = timed(lambda: gs.shard(data, policy, dev, method=method))
            assert again == want, method
            keep(f"shard_gpu_wall_{method}", t)

    best["apply"] = best[f"apply_{gs.DEFAULT_METHOD}"]
    best["gather"] = best[f"gather_{gx.DEFAULT_GATHER}"]
    best["shard_gpu_wall"] = best[f"shard_gpu_wall_{gs.DEFAULT_METHOD}"]
    total = sum(best[s] for s in STAGES)
    partition = best["count"] + best["totals"] + best["apply"]
    extra = [f"apply_{m}" for m in gs.METHODS] + ["gather_walk", "gather_search"]
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "shards": policy.shards, "method": gs.DEFAULT_METHOD, "gather_shape": gx.DEFAULT_GATHER,
        "kept": sum(map(len, want.indices)), "host_frames": host_frames,
        "largest_shard_frames": max(map(len, want.indices)),
        "stages_us": {s: round(best[s] * 1e6, 1) for s in STAGES + tuple(extra)},
        "stages_ns_per_event": {s: round(best[s] / events * 1e9, 2) for s in STAGES},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "yardsticks_us": {k: round(yard[k] * 1e6, 1) for k in YARDSTICKS},
        "partition_us": round(partition * 1e6, 1),
        "partition_vs_x_scan": round(partition / yard["x_scan"], 2),
        "gather_walk_vs_x_gather_walk": round(best["gather_walk"] / yard["x_gather_walk"], 2),
        "gather_search_vs_x_gather_search": round(best["gather_search"] / yard["x_gather_search"], 2),
        "shard_gpu_wall_ms": {m: round(best[f"shard_gpu_wall_{m}"] * 1e3, 3) for m in gs.METHODS},
        "shard_gpu_wall_ns_per_event": round(best["shard_gpu_wall"] / events * 1e9, 2),
        "shard_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "shard_cpu_ms": round(cpu_s * 1e3, 1),
        "shard_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_shard_cpu": round(best["shard_gpu_wall"] / cpu_s, 4),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,4194304", help="stream sizes, comma-separated")
    ap.add_argument("--shards", default="2,8,64,256", help="shard counts, comma-separated")
    ap.add_argument("--media", type=int, default=10000, help="media count of the Workload stream")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_shard", "probe.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a", encoding="utf-8") as log:
        for events in (int(x) for x in a.events.split(",")):
            w = Workload(n_media=a.media, seed=1)
            cases = [(f"media-{a.media}", lambda w=w: b"".join(w.framed(min(65536, events - k))
                                                               for k in range(0, events, 65536))),
                     ("corpus", lambda: corpus_stream(events))]
            for label, make in cases:
                data = make()
                yard = extract_yardsticks(data, a.reps, "cuda:0")
                for shards in (int(x) for x in a.shards.split(",")):
                    line = json.dumps(probe(data, Policy(shards), label, events, a.reps, "cuda:0", yard))
                    print(line, flush=True)
                    log.write(line + "\n")
                    log.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
