"""Price ``stages`` on the GPU against the CPU definition and the transitions' pairs, stage by stage
(MI355X box).

``python -m beholder_amd stages --device gpu`` joins both topics per media with
ops/hip/telemetry_stages.hip (beholder_amd/stages.py defines the result). This script times, for each
stream size and each stream:

* frame_index: the CPU's one pass over the length headers (the only per-event CPU work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``stages_gpu`` does it;
* classify / claim / rank / compact / sort / carry / settle / leads: the kernels of each stage, by HIP
  events (``claim``, ``rank``, ``compact`` and ``sort`` are the transitions' stages called as they are,
  over the events of both topics; ``carry`` is its three launches; ``leads`` is the extract's scan
  over the lead flags and the read-back of the lead events);
* counts: the two words ``(groups, events)`` read back, which decide the sort passes;
* collect: the tables, one row per media, the counters and the overflow list back to the CPU;
* finish: the report built on the CPU, the overflow frames decoded there;
* stages_gpu_wall: the whole of ``gpu_stages.stages`` as the command runs it, allocation included.

The yardsticks, in the same process and on the same input: ``stages_cpu``; and ``tr_pairs``, the
transitions' pairs kernel over the same sorted events, which has the settle's layout and one LDS
atomic per element.

Streams: ``media-N``, Workload events over N media, half of them progress events (64: long runs; 10000:
the stream ``media-10000`` of ``gpu_thin_probe.py``), and ``corpus``, the fold corpus mix
(tests/telemetry_corpus.py ``fold_corpus``, repeated up to the stream size), which has malformed
bodies and non-ASCII ids that go to the CPU. Every run is checked for equality with ``stages_cpu``.

Every (size, stream) runs in a fresh child process under its own time limit (``--limit`` seconds);
the first one that fails or runs out of time ends the probe, and nothing more is started.

Usage: ``gpu_stages_probe.py [--events 16384,262144,2097152] [--media 64,10000] [--reps 3]
[--limit 300] [--out profiles/box_stages/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The stages" cites it.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # telemetry_corpus

STAGES = ("frame_index", "h2d", "classify", "claim", "rank", "counts", "compact", "sort", "carry", "settle", "leads",
          "collect", "finish")
EXTRA = ("tr_pairs",)


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
    w = Workload(n_media=int(label.split("-")[1]), seed=1, progress_fraction=0.5)
    return b"".join(w.framed(min(65536, events - k)) for k in range(0, events, 65536))


def probe(data: bytes, label: str, events: int, reps: int, dev: str) -> dict:
    import torch

    from beholder_amd import replay
    from beholder_amd.ops import gpu_fold, gpu_stages as gs, gpu_transitions as gt
    from beholder_amd.stages import stages_cpu
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

    cpu_s, want = timed(lambda: stages_cpu(data))
    wall_cold, (got, host_frames) = timed(lambda: gs.stages(data, dev))  # loads the module: not a figure
    assert got == want, "the GPU stages disagree with stages_cpu"
    del got
    # `want` stays for the equality checks, which the command does not keep: without this the collector
    # walks its objects again during every timed call (10,000 media: 84 ms for a call of 18 ms)
    gc.collect()
    gc.freeze()
    best = {}

    def keep(name, seconds):
        best[name] = min(best.get(name, seconds), seconds)

    groups = device_events = 0
    for _ in range(reps):
        t, (n, offs) = timed(lambda: gpu_fold.index(data))
        keep("frame_index", t)

        def h2d():
            out = gpu_fold.upload(data, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        tb = gs.allocate(buf, offs_dev, n)
        sync()
        keep("classify", between(lambda: gs.classify(tb))[0])
        keep("claim", between(lambda: gt.claim(tb.t))[0])
        keep("rank", between(lambda: gt.rank(tb.t))[0])
        t, (groups, device_events) = timed(lambda: gt.counts(tb.t))
        keep("counts", t)
        s = k = lead_rows = None
        if not device_events:  # nothing to sort: the stages are not reached
            best.update(compact=0.0, sort=0.0, carry=0.0, settle=0.0, leads=0.0, tr_pairs=0.0)
        else:
            t, s = between(lambda: gt.compact(tb.t, groups, device_events))
            keep("compact", t)
            unsorted = s
            t, s = between(lambda: gt.sort(unsorted))
            keep("sort", t)
            k = gs.prepare(tb, s)
            sync()
            keep("carry", between(lambda: gs.carry(tb, s, k))[0])
            keep("settle", between(lambda: gs.settle(s, k, mask))[0])
            t, lead_rows = timed(lambda: gs.leads(s, k))
            keep("leads", t)
            keep("tr_pairs", between(lambda: gt.pairs(s, mask))[0])  # the yardstick: s.matrix and s.changes are zero
        t, c = timed(lambda: gs.collect(tb, s, k, lead_rows))
        keep("collect", t)
        t, report = timed(lambda: gs.finish(data, offs, n, c, s, k))
        keep("finish", t)
        assert report == want
        del tb, buf, offs_dev, s, k, c, report
        t, (again, _) = timed(lambda: gs.stages(data, dev))
        assert again == want
        del again
        keep("stages_gpu_wall", t)

    total = sum(best[s] for s in STAGES)

    def ratio(name):
        return round(best[name] / best["tr_pairs"], 2) if best["tr_pairs"] else None
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "device_events": device_events, "media": groups, "passes": gt.sort_passes(groups), "host_frames": host_frames,
        "status_events": want.status_events, "progress_events": want.progress_events, "lead_events": want.lead_events,
        "disagree": want.disagree, "closed": sum(want.closed.values()), "warmup": 1, "reps": reps,
        "stages_us": {s: round(best[s] * 1e6, 1) for s in STAGES + EXTRA},
        "stages_ns_per_event": {s: round(best[s] / events * 1e9, 2) for s in STAGES},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "carry_vs_tr_pairs": ratio("carry"), "settle_vs_tr_pairs": ratio("settle"),
        "stages_gpu_wall_ms": round(best["stages_gpu_wall"] * 1e3, 3),
        "stages_gpu_wall_ns_per_event": round(best["stages_gpu_wall"] / events * 1e9, 2),
        "stages_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "stages_cpu_ms": round(cpu_s * 1e3, 1),
        "stages_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_stages_cpu": round(best["stages_gpu_wall"] / cpu_s, 4),
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
    ap.add_argument("--media", default="64,10000", help="media counts of the Workload streams")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds each (size, stream) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_stages", "probe.jsonl"))
    ap.add_argument("--one", metavar="STREAM:EVENTS", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    cases = [(label, events) for events in (int(x) for x in a.events.split(","))
             for label in ["corpus"] + [f"media-{m}" for m in a.media.split(",")]]
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
