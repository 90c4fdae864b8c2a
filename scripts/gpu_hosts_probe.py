"""Price ``hosts`` on the GPU against the CPU definition and the thin, stage by stage (MI355X box).

``python -m beholder_amd hosts --device gpu`` counts what every worker host did with
ops/hip/telemetry_hosts.hip (beholder_amd/hosts.py defines the result). This script times, for each
stream size and each stream:

* frame_index: the CPU's one pass over the length headers (the only per-event CPU work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``hosts_gpu`` does it;
* classify / claim / rank / compact / sort / number / pairs / walk: the kernels of each stage, by HIP
  events (``claim`` and ``rank`` cover the id table and the worker table; ``claim_ids`` and
  ``rank_ids`` are the id table's share, which is what the thin runs; ``compact`` and ``sort`` are the
  transitions' stages called as they are; ``sort_again`` is the same sort of the same events once
  more, with its scratch tensors already in torch's cache; ``pairs`` includes the scan over the pair
  table);
* counts: the three words ``(groups, events, workers)`` read back, which decide the sort passes;
* collect: one row per worker, per media and per pair, the counters and the overflow list back to
  the CPU;
* finish: the report built on the CPU, the overflow frames decoded there;
* hosts_gpu_wall: the whole of ``gpu_hosts.hosts`` as the command runs it, allocation included.

The yardsticks, in the same process and on the same input: ``hosts_cpu``; ``gpu_thin.thin``, whole
(``thin_gpu_wall``), which shares the claim, the scans and the sort; and ``tr_pairs``, the
transitions' pairs kernel over the same sorted events, which has the walk's layout and one LDS
atomic per element.

Streams: ``workers-N``, Workload events over 10,000 media, half of them progress events, each from
one of N workers picked at random (4: the stream ``media-10000`` of ``gpu_thin_probe.py``; 1000; and
``workers-div8``, as many workers as events divided by 8), and ``corpus``, the fold corpus mix
(tests/telemetry_corpus.py ``fold_corpus``, repeated up to the stream size), which has malformed
bodies and non-ASCII ids and hosts that go to the CPU. Every run is checked for equality with
``hosts_cpu``.

Every (size, stream) runs in a fresh child process under its own time limit (``--limit`` seconds);
the first one that fails or runs out of time ends the probe, and nothing more is started.

Usage: ``gpu_hosts_probe.py [--events 16384,262144,2097152] [--workers 4,1000,div8] [--reps 3]
[--limit 300] [--out profiles/box_hosts/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The hosts" cites it.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # telemetry_corpus

STAGES = ("frame_index", "h2d", "classify", "claim", "rank", "counts", "compact", "sort", "number", "pairs", "walk",
          "collect", "finish")
EXTRA = ("claim_ids", "rank_ids", "sort_again", "tr_pairs")
MEDIA = 10000


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def corpus_stream(events: int) -> bytes:
    from beholder_amd.ops import frame
    from beholder_amd.transport.framing import iter_frames
    from telemetry_corpus import fold_corpus
    pieces = [frame(t, b) for t, b in iter_frames(fold_corpus())]
    reps = -(-events // len(pieces))
    return b"".join((pieces * reps)[:events])


def make_stream(label: str, events: int) -> bytes:
    from beholder_amd.bench.generator import Workload
    if label == "corpus":
        return corpus_stream(events)
    count = label.split("-")[1]
    count = max(1, events // 8) if count == "div8" else int(count)
    if count == 4:
        w = Workload(n_media=MEDIA, seed=1, progress_fraction=0.5)  # its own four: three names and the empty one
    else:
        w = Workload(n_media=MEDIA, seed=1, progress_fraction=0.5, hosts=[f"worker-{k}" for k in range(count)])
    return b"".join(w.framed(min(65536, events - k)) for k in range(0, events, 65536))


def probe(data: bytes, label: str, events: int, reps: int, dev: str) -> dict:
    import torch

    from beholder_amd import replay
    from beholder_amd.hosts import hosts_cpu
    from beholder_amd.ops import gpu_extract, gpu_fold, gpu_hosts as gh, gpu_thin as gth, gpu_transitions as gt
    from beholder_amd.thin import Policy
    sync = torch.cuda.synchronize
    mask = gpu_fold.known_mask(replay.status_names())

    def between(fn):
        """Seconds of device time that ``fn``'s launches take, by HIP events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    cpu_s, want = timed(lambda: hosts_cpu(data))
    wall_cold, (got, host_frames) = timed(lambda: gh.hosts(data, dev))  # loads the module: not a figure
    assert got == want, "the GPU hosts disagree with hosts_cpu"
    gth.thin(data, Policy(), dev)
    best = {}

    def keep(name, seconds):
        best[name] = min(best.get(name, seconds), seconds)

    groups = progress_events = workers = 0
    for _ in range(reps):
        t, (n, offs) = timed(lambda: gpu_fold.index(data))
        keep("frame_index", t)

        def h2d():
            out = gpu_fold.upload(data, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        tb = gh.allocate(buf, offs_dev, n)
        sync()
        keep("classify", between(lambda: gh.classify(tb))[0])
        ids = between(lambda: gt.claim(tb.t))[0]
        keep("claim_ids", ids)
        keep("claim", ids + between(lambda: gt.claim(tb.w))[0])
        ids = between(lambda: gt.rank(tb.t))[0]
        keep("rank_ids", ids)
        keep("rank", ids + between(lambda: gpu_extract.scan(tb.w.slot_scan))[0])
        t, (groups, progress_events, workers) = timed(lambda: gh.counts(tb))
        keep("counts", t)
        s = k = None
        if not progress_events:  # nothing to sort: the stages are not reached
            best.update(compact=0.0, sort=0.0, sort_again=0.0, number=0.0, pairs=0.0, walk=0.0, tr_pairs=0.0)
        else:
            t, s = between(lambda: gt.compact(tb.t, groups, progress_events))
            keep("compact", t)
            unsorted = s
            t, s = between(lambda: gt.sort(unsorted))
            keep("sort", t)
            keep("sort_again", between(lambda: gt.sort(unsorted))[0])  # the same sort once more, its scratch cached
            k = gh.prepare(tb, s, workers)
            sync()
            keep("number", between(lambda: gh.number(tb, s, k))[0])
            keep("pairs", between(lambda: gh.pairs(tb, s, k))[0])
            keep("walk", between(lambda: gh.walk(s, k, mask))[0])
            keep("tr_pairs", between(lambda: gt.pairs(s, mask))[0])  # the yardstick: s.matrix and s.changes are zero
        t, c = timed(lambda: gh.collect(tb, s, k))
        keep("collect", t)
        t, report = timed(lambda: gh.finish(data, offs, n, c, s, k))
        keep("finish", t)
        assert report == want
        del tb, buf, offs_dev, s, k, c
        t, (again, _) = timed(lambda: gh.hosts(data, dev))
        assert again == want
        keep("hosts_gpu_wall", t)
        keep("thin_gpu_wall", timed(lambda: gth.thin(data, Policy(), dev))[0])

    total = sum(best[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "progress_events": progress_events, "media": groups, "workers": workers, "pairs": len(want.pairs),
        "passes": gt.sort_passes(groups), "host_frames": host_frames,
        "handovers": want.handovers, "rewinds": want.rewinds, "lds_workers": gh.LDS_WORKERS,
        "stages_us": {s: round(best[s] * 1e6, 1) for s in STAGES + EXTRA},
        "stages_ns_per_event": {s: round(best[s] / events * 1e9, 2) for s in STAGES},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "walk_vs_tr_pairs": round(best["walk"] / best["tr_pairs"], 2) if best["tr_pairs"] else None,
        "hosts_gpu_wall_ms": round(best["hosts_gpu_wall"] * 1e3, 3),
        "hosts_gpu_wall_ns_per_event": round(best["hosts_gpu_wall"] / events * 1e9, 2),
        "hosts_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "thin_gpu_wall_ms": round(best["thin_gpu_wall"] * 1e3, 3),
        "wall_vs_thin_gpu": round(best["hosts_gpu_wall"] / best["thin_gpu_wall"], 2),
        "hosts_cpu_ms": round(cpu_s * 1e3, 1),
        "hosts_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_hosts_cpu": round(best["hosts_gpu_wall"] / cpu_s, 4),
    }


def one(a: argparse.Namespace) -> int:
    """The child: one (size, stream), one JSON line on stdout."""
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    label, events = a.one.rsplit(":", 1)
    print(json.dumps(probe(make_stream(label, int(events)), label, int(events), a.reps, "cuda:0")), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,2097152", help="stream sizes, comma-separated")
    ap.add_argument("--workers", default="4,1000,div8", help="worker counts of the Workload streams (div8: events / 8)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds each (size, stream) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_hosts", "probe.jsonl"))
    ap.add_argument("--one", metavar="STREAM:EVENTS", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    cases = [(label, events) for events in (int(x) for x in a.events.split(","))
             for label in ["corpus"] + [f"workers-{m}" for m in a.workers.split(",")]]
    with open(a.out, "a", encoding="utf-8") as log:
        for label, events in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{label}:{events}", "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps({"error": f"{label}:{events} ran past {a.limit} s; nothing more is started"}),
                      flush=True)
                return 1
            if r.returncode != 0:
                print(json.dumps({"error": f"{label}:{events} exited {r.returncode}; nothing more is started",
                                  "stderr": r.stderr[-2000:]}), flush=True)
                return 1
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
