"""Price ``coalesce`` on the GPU against the CPU coalesce, stage by stage (MI355X box).

``python -m beholder_amd coalesce --device gpu`` cuts a captured stream down to the frames that set
its end state with ops/hip/telemetry_coalesce.hip (beholder_amd/coalesce.py defines the result). This
script times, for each stream size and each media count, under the default policy:

* frame_index: the host's one pass over the length headers (the only per-event host work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``coalesce_gpu`` does it;
* classify / claim / mark: the three kernels, by HIP events, each a launch of its own;
* host_decide: the overflow count read back, and the host's decisions where there are any;
* scan / gather: the extract's kernels over this ``keep_len``, by HIP events;
* totals: the one word read back to size the output;
* d2h: the output bytes, the kept indices and their keyed flags back to the host;
* keys: ``key_of`` over the kept keyed frames, one decode per distinct key;
* coalesce_gpu_wall: the whole of ``gpu_coalesce.coalesce`` as the command runs it, allocation included.

Streams: Workload events over 16 media (every claim lands on 32 keys: the hot-key case) and over
10,000 media, and ``corpus``, the fold corpus mix (tests/telemetry_corpus.py ``fold_corpus``, repeated
up to the stream size), which has malformed bodies and non-ASCII ids that go to the host. Every run
is checked for equality with ``coalesce_cpu``, which is timed too.

Usage: ``gpu_coalesce_probe.py [--events 16384,262144,4194304] [--out profiles/box_coalesce/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The coalesce" cites it.
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
from beholder_amd.coalesce import Policy, coalesce_cpu  # noqa: E402
from beholder_amd.ops import gpu_coalesce as gc, gpu_extract as gx, gpu_fold  # noqa: E402
from beholder_amd.transport.framing import iter_frames  # noqa: E402

STAGES = ("frame_index", "h2d", "classify", "claim", "mark", "host_decide", "scan", "totals", "gather", "d2h", "keys")
KERNELS = ("classify", "claim", "mark", "scan", "gather")


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


def probe(data: bytes, policy: Policy, label: str, events: int, reps: int, dev: str) -> dict:
    sync = torch.cuda.synchronize
    cpu_s, want = timed(lambda: coalesce_cpu(data, policy))
    wall_cold, (got, host_frames) = timed(lambda: gc.coalesce(data, policy, dev))  # loads the module: not a figure
    assert got == want, "the GPU coalesce disagrees with coalesce_cpu"
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
        tables = gc.allocate(buf, offs_dev, n)
        params = gc.coalesce_params(policy, tables.slots)
        sync()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
        for k, stage in enumerate((gc.STAGE_CLASSIFY, gc.STAGE_CLAIM, gc.STAGE_MARK)):
            e[2 * k].record()
            gc.launch(tables, params, stages=stage)
            e[2 * k + 1].record()
        e[5].synchronize()
        t, _ = timed(lambda: gc.decide_on_host(tables, data, offs, policy))
        keep("host_decide", t)
        e[6].record()
        gx.scan(tables.select)
        e[7].record()
        e[7].synchronize()
        t, (kept, kept_bytes) = timed(lambda: gx.totals(tables.select))
        keep("totals", t)
        e[8].record()
        out = gx.gather(tables.select, kept, kept_bytes)
        e[9].record()
        e[9].synchronize()
        for k, name in enumerate(KERNELS):
            keep(name, e[2 * k].elapsed_time(e[2 * k + 1]) * 1e-3)
        t, (out_bytes, indices, flags) = timed(lambda: gc.collect(tables, out, kept))
        keep("d2h", t)
        t, keys = timed(lambda: gc.finish(data, offs, indices, flags, policy))
        keep("keys", t)
        assert out_bytes == want.data and indices == want.indices and keys == want.keys
        del tables, buf, offs_dev, out
        t, _ = timed(lambda: gc.coalesce(data, policy, dev))
        keep("coalesce_gpu_wall", t)

    total = sum(best[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "kept": len(want.indices), "kept_bytes": len(want.data), "keys": sum(k is not None for k in want.keys),
        "host_frames": host_frames,
        "stages_us": {s: round(best[s] * 1e6, 1) for s in STAGES},
        "stages_ns_per_event": {s: round(best[s] / events * 1e9, 2) for s in STAGES},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "coalesce_gpu_wall_ms": round(best["coalesce_gpu_wall"] * 1e3, 3),
        "coalesce_gpu_wall_ns_per_event": round(best["coalesce_gpu_wall"] / events * 1e9, 2),
        "coalesce_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "coalesce_cpu_ms": round(cpu_s * 1e3, 1),
        "coalesce_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_coalesce_cpu": round(best["coalesce_gpu_wall"] / cpu_s, 4),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,4194304", help="stream sizes, comma-separated")
    ap.add_argument("--media", default="16,10000", help="media counts of the Workload streams, comma-separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_coalesce", "probe.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a", encoding="utf-8") as log:
        for events in (int(x) for x in a.events.split(",")):
            cases = []
            for media in (int(x) for x in a.media.split(",")):
                w = Workload(n_media=media, seed=1)
                cases.append((f"media-{media}", lambda w=w: b"".join(w.framed(min(65536, events - k))
                                                                     for k in range(0, events, 65536))))
            cases.append(("corpus", lambda: corpus_stream(events)))
            for label, make in cases:
                line = json.dumps(probe(make(), Policy(), label, events, a.reps, "cuda:0"))
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
