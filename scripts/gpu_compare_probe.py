"""Price ``compare`` on the GPU against the CPU compare, stage by stage (MI355X box).

``python -m beholder_amd compare --device gpu`` matches two captured streams frame for frame with
ops/hip/telemetry_compare.hip and the transitions' claim and sort (beholder_amd/compare.py defines
the result). This script times, for each joined size and each pair of streams, all topics:

* frame_index: the host's pass over both captures' length headers;
* h2d: both captures into one device tensor, and the joined offsets, from pageable memory as
  ``compare_gpu`` does it;
* classify, claim, rank (the two scans), compact, sort, bounds, match, scan_matched, breaks, scan_a,
  scan_b, gather_a, gather_b: the kernels by HIP events, each stage a launch or a few of its own;
* claim_dedupe_wide: ``dedupe_claim`` in its ``wide`` form over the same joined stream, after the
  dedupe's own hash launch: what the claim costs where the key compare walks 8 bytes a step and not
  one, as ``tr_claim`` does;
* counts, host_pair, totals: the words the host reads back between the launches, and the host's
  pairing of the frames above the cap where there are any;
* d2h: both outputs and their indices back to the host;
* compare_gpu_wall: the whole of ``gpu_compare.compare`` as the command runs it, allocation included;
* dedupe_gpu_wall: ``gpu_dedupe.dedupe`` over the joined stream, the nearest existing call (the same
  hash, a claim, one scan and one gather);
* compare_cpu: the definition on the same inputs.

Pairs, at N joined events (A has N / 2): ``itself``, A against A, Workload events over 10,000 media;
``shuffled``, A against its shuffle; ``deduped``, A against ``dedupe_cpu(A)`` (fewer than N joined
events); ``hot``, the dedupe probe's hot stream against itself: 128 events over 16 media repeated,
so at 4,194,304 joined events every content's run is 32,768 long. Every run is checked for equality
with ``compare_cpu``.

Usage: ``gpu_compare_probe.py [--events 16384,262144,4194304] [--out profiles/box_compare/probe.jsonl]``.
Output: one JSON object per (size, pair) on stdout and appended to ``--out``.
docs/DESIGN.md "The compare" cites it.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from beholder_amd import dedupe as dd  # noqa: E402
from beholder_amd.bench.generator import Workload  # noqa: E402
from beholder_amd.compare import Policy, compare_cpu  # noqa: E402
from beholder_amd.ops import frame, gpu_compare as gc, gpu_dedupe as gd, gpu_extract as gx, gpu_fold  # noqa: E402
from beholder_amd.ops import gpu_transitions as gt  # noqa: E402
from beholder_amd.transport.framing import iter_frames  # noqa: E402

HOST_STAGES = ("frame_index", "h2d", "counts", "host_pair", "totals", "d2h")
KERNELS = ("classify", "claim", "rank", "compact", "sort", "bounds", "match", "scan_matched", "breaks", "scan_a",
           "scan_b", "gather_a", "gather_b")
ASIDE = ("claim_dedupe_wide",)  # measured, not part of the chain


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def workload_stream(media: int, events: int) -> bytes:
    w = Workload(n_media=media, seed=1)
    return b"".join(w.framed(min(65536, events - k)) for k in range(0, events, 65536))


def shuffled(data: bytes) -> bytes:
    pieces = [frame(t, b) for t, b in iter_frames(data)]
    random.Random(5).shuffle(pieces)
    return b"".join(pieces)


def pairs_of(events: int):
    half = events // 2
    a = workload_stream(10000, half)
    yield "itself", a, a
    yield "shuffled", a, shuffled(a)
    yield "deduped", a, dd.dedupe_cpu(a).data
    hot = Workload(n_media=16, seed=1).framed(128) * (half // 128)
    yield "hot", hot, hot


def probe(a: bytes, b: bytes, label: str, events: int, reps: int, dev: str) -> dict:
    sync = torch.cuda.synchronize
    policy = Policy()
    cpu_s, want = timed(lambda: compare_cpu(a, b, policy))
    wall_cold, (got, host_frames) = timed(lambda: gc.compare(a, b, policy, dev))  # loads the module: not a figure
    assert got == want, "the GPU compare disagrees with compare_cpu"
    joined = a + b  # for the dedupe yardstick only; compare_gpu never builds it
    best = {}

    def keep(name, seconds):
        best[name] = min(best.get(name, seconds), seconds)

    def event():
        return torch.cuda.Event(enable_timing=True)

    for _ in range(reps):
        t, ((n_a, offs_a), (n_b, offs_b)) = timed(lambda: (gpu_fold.index(a), gpu_fold.index(b)))
        keep("frame_index", t)
        n = n_a + n_b
        offs = gc.join_offsets(offs_a, offs_b, len(a))

        def h2d():
            out = gc.upload(a, b, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        tb = gc.allocate(buf, offs_dev, n, n_a)
        params = gc.params_of(policy, tb.t.slots)
        marks = {}

        def kernel(name, launch):
            marks[name] = (event(), event())
            marks[name][0].record()
            out = launch()
            marks[name][1].record()
            return out

        sync()
        kernel("classify", lambda: gc.classify(tb, params))
        kernel("claim", lambda: gt.claim(tb.t))
        kernel("rank", lambda: gt.rank(tb.t))
        sync()
        t, (groups, device_events) = timed(lambda: gt.counts(tb.t))
        keep("counts", t)
        s = kernel("compact", lambda: gt.compact(tb.t, groups, device_events))
        s = kernel("sort", lambda: gt.sort(s))
        bounds = kernel("bounds", lambda: gc.bounds(s))
        kernel("match", lambda: gc.match(tb, s, bounds))
        sync()
        t, (counters, host) = timed(lambda: gc.pair_on_host(tb, a, b, offs))
        keep("host_pair", t)
        kernel("scan_matched", lambda: gx.scan(tb.matched_scan))
        sync()
        matched = gx.totals(tb.matched_scan)[0]
        kernel("breaks", lambda: gc.hip_lib.call("bh_compare_breaks", tb.partner, tb.matched_scan.indices.data_ptr(),
                                                 matched, tb.partner.data_ptr(), n, tb.t.counters.data_ptr()))
        kernel("scan_a", lambda: gx.scan(tb.select_a))
        kernel("scan_b", lambda: gx.scan(tb.select_b))
        sync()
        t, sizes = timed(lambda: (gx.totals(tb.select_a), gx.totals(tb.select_b)))
        keep("totals", t)
        out_a = kernel("gather_a", lambda: gx.gather(tb.select_a, *sizes[0]))
        out_b = kernel("gather_b", lambda: gx.gather(tb.select_b, *sizes[1]))
        sync()
        t, (side_a, side_b) = timed(lambda: (gx.collect(tb.select_a, out_a, sizes[0][0]),
                                             gx.collect(tb.select_b, out_b, sizes[1][0])))
        keep("d2h", t)
        assert side_a == (want.a.data, want.a.indices) and side_b[0] == want.b.data
        assert matched == want.matched and int(tb.t.counters[gc.C_BREAKS].item()) == want.order_breaks
        # the dedupe's own claim over the same joined stream, its wide compare
        dt = gd.allocate(buf, offs_dev, n)
        dparams = gd.dedupe_params(dd.Policy(), dt.slots, method="wide")
        gd.launch(dt, dparams, stages=gd.STAGE_HASH)
        sync()
        kernel("claim_dedupe_wide", lambda: gd.launch(dt, dparams, stages=gd.STAGE_CLAIM))
        sync()
        for name, (e0, e1) in marks.items():
            keep(name, e0.elapsed_time(e1) * 1e-3)
        del tb, dt, s, bounds, buf, offs_dev, out_a, out_b
        t, (again, _) = timed(lambda: gc.compare(a, b, policy, dev))
        keep("compare_gpu_wall", t)
        assert again == want
        t, _ = timed(lambda: gd.dedupe(joined, dd.Policy(), dev))
        keep("dedupe_gpu_wall", t)

    chain = HOST_STAGES + KERNELS
    total = sum(best[s] for s in chain)
    wall = best["compare_gpu_wall"]
    joined_events = want.a.frames + want.b.frames
    return {
        "device": torch.cuda.get_device_name(0), "pair": label, "events": events, "joined_events": joined_events,
        "bytes": len(joined), "mean_content_bytes": round((len(joined) - 4 * joined_events) / joined_events, 1),
        "matched": want.matched, "only_a": len(want.a.indices), "only_b": len(want.b.indices),
        "distinct_common": want.common, "order_breaks": want.order_breaks, "host_frames": host_frames,
        "stages_us": {s: round(best[s] * 1e6, 1) for s in chain + ASIDE},
        "stages_ns_per_event": {s: round(best[s] / joined_events * 1e9, 2) for s in chain + ASIDE},
        "stage_sum_ns_per_event": round(total / joined_events * 1e9, 2),
        "compare_gpu_wall_ms": round(wall * 1e3, 3),
        "compare_gpu_wall_ns_per_event": round(wall / joined_events * 1e9, 2),
        "compare_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "dedupe_gpu_wall_ms": round(best["dedupe_gpu_wall"] * 1e3, 3),
        "compare_cpu_ms": round(cpu_s * 1e3, 1),
        "compare_cpu_ns_per_event": round(cpu_s / joined_events * 1e9, 1),
        "wall_vs_compare_cpu": round(wall / cpu_s, 4),
        "wall_vs_dedupe_gpu": round(wall / best["dedupe_gpu_wall"], 3),
        "claim_vs_claim_dedupe_wide": round(best["claim"] / best["claim_dedupe_wide"], 3),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,4194304", help="joined sizes, comma-separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_compare", "probe.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a", encoding="utf-8") as log:
        for events in (int(x) for x in a.events.split(",")):
            for label, one, other in pairs_of(events):
                line = json.dumps(probe(one, other, label, events, a.reps, "cuda:0"))
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
