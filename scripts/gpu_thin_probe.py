"""Price ``thin`` on the GPU against the CPU definition and the transitions, stage by stage (MI355X box).

``python -m beholder_amd thin --device gpu`` drops the progress events that repeat their media's step
with ops/hip/telemetry_thin.hip (beholder_amd/thin.py defines the result). This script times, for
each stream size and each stream:

* frame_index: the host's one pass over the length headers (the only per-event host work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``thin_gpu`` does it;
* classify / claim / rank / compact / sort / mark: the kernels of each stage, by HIP events
  (``claim``, ``rank``, ``compact`` and ``sort`` are the transitions' stages called as they are;
  ``sort_again`` is the same sort of the same events once more, with its scratch tensors already in
  torch's cache, which is how ``gpu_transitions_probe.py`` meets its ``sort``);
* counts: the two words ``(groups, events)`` read back, which decide the sort passes;
* host: ``decide_on_host``, which reads the counters and decides the frames left to the host;
* scan / gather: the extract's launches over ``keep_len``, by HIP events; ``totals`` is the one word
  read back between them;
* d2h: the kept bytes and indices back to the host;
* thin_gpu_wall: the whole of ``gpu_thin.thin`` as the command runs it, allocation included.

The yardsticks, on the same input: ``thin_cpu``, and ``gpu_transitions.transitions``
(``transitions_gpu_wall``), which shares the claim, the scans and the sort.

Streams: Workload events, half of them progress events, over 200, 10,000 and 200,000 media (which
need one, two and, at the larger sizes, three passes), and ``corpus``, the fold corpus mix
(tests/telemetry_corpus.py ``fold_corpus``, repeated up to the stream size), which has malformed
bodies and non-ASCII ids that go to the host. Every run is checked for equality with ``thin_cpu``.

Every (size, stream) runs in a fresh child process under its own time limit (``--limit`` seconds);
the first one that fails or runs out of time ends the probe, and nothing more is started.

Usage: ``gpu_thin_probe.py [--events 16384,262144,2097152] [--media 200,10000,200000] [--step 10]
[--keep last] [--reps 3] [--limit 240] [--out profiles/box_thin/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The thin" cites it.
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

STAGES = ("frame_index", "h2d", "classify", "claim", "rank", "counts", "compact", "sort", "mark", "host", "scan",
          "totals", "gather", "d2h")
EXTRA = ("sort_again",)


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


def probe(data: bytes, label: str, events: int, reps: int, dev: str, policy) -> dict:
    import torch

    from beholder_amd.ops import gpu_extract, gpu_fold, gpu_thin as gth, gpu_transitions as gt
    from beholder_amd.thin import thin_cpu
    sync = torch.cuda.synchronize

    def between(fn):
        """Seconds of device time that ``fn``'s launches take, by HIP events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    cpu_s, want = timed(lambda: thin_cpu(data, policy))
    wall_cold, (got, host_frames) = timed(lambda: gth.thin(data, policy, dev))  # loads the module: not a figure
    assert got == want, "the GPU thin disagrees with thin_cpu"
    gt.transitions(data, dev)
    best = {}

    def keep(name, seconds):
        best[name] = min(best.get(name, seconds), seconds)

    groups = progress_events = 0
    for _ in range(reps):
        t, (n, offs) = timed(lambda: gpu_fold.index(data))
        keep("frame_index", t)

        def h2d():
            out = gpu_fold.upload(data, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        tb = gth.allocate(buf, offs_dev, n)
        sync()
        keep("classify", between(lambda: gth.classify(tb, policy))[0])
        keep("claim", between(lambda: gt.claim(tb.t))[0])
        keep("rank", between(lambda: gt.rank(tb.t))[0])
        t, (groups, progress_events) = timed(lambda: gt.counts(tb.t))
        keep("counts", t)
        s = None
        if not progress_events:  # nothing to sort: the stages are not reached
            best.update(compact=0.0, sort=0.0, sort_again=0.0, mark=0.0)
        else:
            t, s = between(lambda: gt.compact(tb.t, groups, progress_events))
            keep("compact", t)
            unsorted = s
            t, s = between(lambda: gt.sort(unsorted))
            keep("sort", t)
            keep("sort_again", between(lambda: gt.sort(unsorted))[0])  # the same sort once more, its scratch cached
            keep("mark", between(lambda: gth.mark(tb, s, policy))[0])
        keep("host", timed(lambda: gth.decide_on_host(tb, s, data, offs, policy))[0])
        keep("scan", between(lambda: gpu_extract.scan(tb.select))[0])
        t, (kept, kept_bytes) = timed(lambda: gpu_extract.totals(tb.select))
        keep("totals", t)
        t, out = between(lambda: gpu_extract.gather(tb.select, kept, kept_bytes))
        keep("gather", t)
        t, (out_bytes, indices) = timed(lambda: gpu_extract.collect(tb.select, out, kept))
        keep("d2h", t)
        assert out_bytes == want.data and indices == want.indices
        del tb, buf, offs_dev, s, out
        t, (again, _) = timed(lambda: gth.thin(data, policy, dev))
        assert again == want
        keep("thin_gpu_wall", t)
        keep("transitions_gpu_wall", timed(lambda: gt.transitions(data, dev))[0])

    total = sum(best[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "step": policy.step, "keep": policy.keep,
        "progress_events": progress_events, "media": groups, "passes": gt.sort_passes(groups),
        "host_frames": host_frames,
        "kept": len(want.indices), "dropped": want.frames - len(want.indices),
        "stages_us": {s: round(best[s] * 1e6, 1) for s in STAGES + EXTRA},
        "stages_ns_per_event": {s: round(best[s] / events * 1e9, 2) for s in STAGES},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "thin_gpu_wall_ms": round(best["thin_gpu_wall"] * 1e3, 3),
        "thin_gpu_wall_ns_per_event": round(best["thin_gpu_wall"] / events * 1e9, 2),
        "thin_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "transitions_gpu_wall_ms": round(best["transitions_gpu_wall"] * 1e3, 3),
        "wall_vs_transitions_gpu": round(best["thin_gpu_wall"] / best["transitions_gpu_wall"], 2),
        "thin_cpu_ms": round(cpu_s * 1e3, 1),
        "thin_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_thin_cpu": round(best["thin_gpu_wall"] / cpu_s, 4),
    }


def one(a: argparse.Namespace) -> int:
    """The child: one (size, stream), one JSON line on stdout."""
    import torch

    from beholder_amd.thin import Policy
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    label, events = a.one.rsplit(":", 1)
    result = probe(make_stream(label, int(events)), label, int(events), a.reps, "cuda:0", Policy(a.step, a.keep))
    print(json.dumps(result), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,2097152", help="stream sizes, comma-separated")
    ap.add_argument("--media", default="200,10000,200000", help="media counts of the Workload streams")
    ap.add_argument("--step", type=int, default=10)
    ap.add_argument("--keep", choices=["last", "first"], default="last")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds each (size, stream) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_thin", "probe.jsonl"))
    ap.add_argument("--one", metavar="STREAM:EVENTS", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    cases = [(label, events) for events in (int(x) for x in a.events.split(","))
             for label in ["corpus"] + [f"media-{int(m)}" for m in a.media.split(",")]]
    with open(a.out, "a", encoding="utf-8") as log:
        for label, events in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{label}:{events}", "--step", str(a.step),
                   "--keep", a.keep, "--reps", str(a.reps)]
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
