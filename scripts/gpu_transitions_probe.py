"""Price ``transitions`` on the GPU against the CPU definition and the fold, stage by stage (MI355X box).

``python -m beholder_amd transitions --device gpu`` counts a captured stream's per-media status moves
with ops/hip/telemetry_transitions.hip (beholder_amd/transitions.py defines the result). This script
times, for each stream size and each stream:

* frame_index: the host's one pass over the length headers (the only per-event host work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``transitions_gpu`` does it;
* classify / claim / rank / compact / pairs: the kernels of each stage, by HIP events (``rank`` is
  the extract's scan twice: over the table's slots and over the frames);
* counts: the two words ``(groups, events)`` read back, which decide the sort passes;
* sort: the passes the stream needs, by HIP events, and apart from that the sort forced to 1, 2
  and 3 passes (``sort_1``, ``sort_2``, ``sort_3``: more passes than needed change nothing) and one
  pass split into its three launches (``pass_count``, ``pass_totals``, ``pass_apply``);
* finish: the matrix, the counters and the per-media rows back to the host, and the ``Transitions``
  built from them (the host's frames included);
* transitions_gpu_wall: the whole of ``gpu_transitions.transitions`` as the command runs it,
  allocation included.

The yardsticks, on the same input: ``transitions_cpu``, and ``gpu_fold.fold`` (``fold_gpu_wall``),
the nearest existing reduction: the difference is the price of order.

Streams: Workload events, half of them status events, over 200, 10,000 and 200,000 media (which
need one, two and, at the larger sizes, three passes), and ``corpus``, the fold corpus mix
(tests/telemetry_corpus.py ``fold_corpus``, repeated up to the stream size), which has malformed
bodies and non-ASCII ids that go to the host. Every run is checked for equality with
``transitions_cpu``.

Usage: ``gpu_transitions_probe.py [--events 16384,262144,2097152] [--media 200,10000,200000] [--out profiles/box_transitions/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The transitions" cites it.
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

from beholder_amd import replay  # noqa: E402
from beholder_amd.bench.generator import Workload  # noqa: E402
from beholder_amd.ops import gpu_fold, gpu_transitions as gt  # noqa: E402
from beholder_amd.transitions import transitions_cpu  # noqa: E402
from beholder_amd.transport.framing import iter_frames  # noqa: E402

STAGES = ("frame_index", "h2d", "classify", "claim", "rank", "counts", "compact", "sort", "pairs", "finish")
EXTRA = ("sort_1", "sort_2", "sort_3", "pass_count", "pass_totals", "pass_apply")


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


def probe(data: bytes, label: str, events: int, reps: int, dev: str) -> dict:
    sync = torch.cuda.synchronize
    mask = gpu_fold.known_mask(replay.status_names())
    cpu_s, want = timed(lambda: transitions_cpu(data))
    wall_cold, (got, host_frames) = timed(lambda: gt.transitions(data, dev))  # loads the module: not a figure
    assert got == want, "the GPU transitions disagree with transitions_cpu"
    gpu_fold.fold(data, dev)
    best = {}

    def keep(name, seconds):
        best[name] = min(best.get(name, seconds), seconds)

    groups = status_events = 0
    for _ in range(reps):
        t, (n, offs) = timed(lambda: gpu_fold.index(data))
        keep("frame_index", t)

        def h2d():
            out = gpu_fold.upload(data, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        tables = gt.allocate(buf, offs_dev, n)
        sync()
        keep("classify", between(lambda: gt.classify(tables))[0])
        keep("claim", between(lambda: gt.claim(tables))[0])
        keep("rank", between(lambda: gt.rank(tables))[0])
        t, (groups, status_events) = timed(lambda: gt.counts(tables))
        keep("counts", t)
        t, s = between(lambda: gt.compact(tables, groups, status_events))
        keep("compact", t)
        for passes in (1, 2, 3):
            keep(f"sort_{passes}", between(lambda: gt.sort(s, passes))[0])
        keys_b, vals_b, totals, base = gt.sort_scratch(s)
        for name, stage in (("pass_count", gt.STAGE_COUNT), ("pass_totals", gt.STAGE_TOTALS), ("pass_apply", gt.STAGE_APPLY)):
            keep(name, between(lambda: gt.sort_pass(s.keys, s.vals, s.events, 0, totals, base, keys_b, vals_b, stage))[0])
        del keys_b, vals_b, totals, base
        t, done = between(lambda: gt.sort(s))
        keep("sort", t)
        keep("pairs", between(lambda: gt.pairs(done, mask))[0])
        t, again = timed(lambda: gt.finish(data, offs, n, gt.collect(tables, done), done))
        keep("finish", t)
        assert again == want
        del tables, buf, offs_dev, s, done
        t, (again, _) = timed(lambda: gt.transitions(data, dev))
        assert again == want
        keep("transitions_gpu_wall", t)
        keep("fold_gpu_wall", timed(lambda: gpu_fold.fold(data, dev))[0])

    total = sum(best[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "status_events": status_events, "media": groups, "passes": gt.sort_passes(groups), "host_frames": host_frames,
        "transitions": want.transitions, "changes": want.changes,
        "stages_us": {s: round(best[s] * 1e6, 1) for s in STAGES + EXTRA},
        "stages_ns_per_event": {s: round(best[s] / events * 1e9, 2) for s in STAGES},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "transitions_gpu_wall_ms": round(best["transitions_gpu_wall"] * 1e3, 3),
        "transitions_gpu_wall_ns_per_event": round(best["transitions_gpu_wall"] / events * 1e9, 2),
        "transitions_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "fold_gpu_wall_ms": round(best["fold_gpu_wall"] * 1e3, 3),
        "wall_vs_fold_gpu": round(best["transitions_gpu_wall"] / best["fold_gpu_wall"], 2),
        "transitions_cpu_ms": round(cpu_s * 1e3, 1),
        "transitions_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_transitions_cpu": round(best["transitions_gpu_wall"] / cpu_s, 4),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,2097152", help="stream sizes, comma-separated")
    ap.add_argument("--media", default="200,10000,200000", help="media counts of the Workload streams")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_transitions", "probe.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a", encoding="utf-8") as log:
        for events in (int(x) for x in a.events.split(",")):
            cases = [("corpus", lambda: corpus_stream(events))]
            for media in (int(x) for x in a.media.split(",")):
                w = Workload(n_media=media, seed=1, progress_fraction=0.5)
                cases.append((f"media-{media}", lambda w=w: b"".join(w.framed(min(65536, events - k))
                                                                     for k in range(0, events, 65536))))
            for label, make in cases:
                line = json.dumps(probe(make(), label, events, a.reps, "cuda:0"))
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
