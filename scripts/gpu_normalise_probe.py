"""Price ``normalise`` on the GPU against the extract that keeps everything, stage by stage (MI355X box).

``python -m beholder_amd normalise --device gpu`` rewrites every decodable event in canonical form
with ops/hip/telemetry_normalise.hip (beholder_amd/normalise.py defines the result). Nothing else in
the project writes an event, so the yardstick is existing code on the same stream in the same
process: ``extract`` with a selector that keeps every frame (``select_mark``, the scan,
``gather_walk``), which reads every frame once and copies every byte once; ``normalise`` does that
and synthesises the bytes. This script times, for each stream size and each stream:

* frame_index: the host's one pass over the length headers;
* h2d: the stream and its offsets to HBM, from pageable memory as ``normalise_gpu`` does it;
* classify against select_mark, and emit against gather_walk: the kernels, by HIP events;
* host: ``decide_on_host``, which reads the counters and encodes the frames left to the host;
* scan: the extract's launches over ``keep_len``, by HIP events; totals: the one word read back;
* d2h: the output and the indices back to the host, the host's frames spliced in;
* normalise_gpu_wall and extract_gpu_wall: the whole calls as the commands run them, allocation
  included; normalise_cpu: the definition, once.

Every figure is the median of ``--reps`` repeats after one warm-up call that loads the module, with
the least and the most next to it (``*_spread``). Every run is checked for equality with
``normalise_cpu``.

Streams, in the protobufjs dialect: Workload events, half of them progress events, over 200, 10,000
and 200,000 media, which are canonical already (emit writes what it read); and ``corpus``, the fold
corpus mix (tests/telemetry_corpus.py ``fold_corpus``, repeated up to the stream size), which has
malformed bodies, events to rewrite and non-ASCII ids that go to the host.

Every (size, stream) runs in a fresh child process under its own time limit (``--limit`` seconds);
the first one that fails or runs out of time ends the probe, and nothing more is started.

Usage: ``gpu_normalise_probe.py [--events 16384,262144,2097152] [--media 200,10000,200000]
[--undecoded keep] [--reps 7] [--limit 240] [--out profiles/box_normalise/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The normalise" cites it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # telemetry_corpus

STAGES = ("frame_index", "h2d", "classify", "host", "scan", "totals", "emit", "d2h")
YARDSTICKS = ("select_mark", "gather_walk")
WALLS = ("normalise_gpu_wall", "extract_gpu_wall")


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

    from beholder_amd.extract import Selector
    from beholder_amd.normalise import normalise_cpu
    from beholder_amd.ops import gpu_extract as gx, gpu_fold, gpu_normalise as gn
    sync = torch.cuda.synchronize
    dialect = "protobufjs"
    everything = Selector()

    def between(fn):
        """Seconds of device time that ``fn``'s launches take, by HIP events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    cpu_s, want = timed(lambda: normalise_cpu(data, policy, dialect))
    wall_cold, (got, host_frames) = timed(lambda: gn.normalise(data, policy, dev, dialect))  # loads the module: no figure
    assert got == want, "the GPU normalise disagrees with normalise_cpu"
    copy, _ = gx.extract(data, everything, dev, dialect)
    assert copy.data == bytes(data) and copy.frames == want.frames
    seen = {}

    def keep(name, seconds):
        seen.setdefault(name, []).append(seconds)

    params = gx.select_params(everything, gx.table_slots(0))
    table, blob = gx.build_media_table([], params.hash_mask)
    for _ in range(reps):
        t, (n, offs) = timed(lambda: gpu_fold.index(data))
        keep("frame_index", t)

        def h2d():
            out = gpu_fold.upload(data, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        # the yardstick and the new kernels alternate on one upload
        x = gx.allocate(buf, offs_dev, n, table, blob)
        tb = gn.allocate(buf, offs_dev, n)
        sync()
        keep("select_mark", between(lambda: gx.mark(x, params, dialect))[0])
        keep("classify", between(lambda: gn.classify(tb, policy, dialect))[0])
        gx.decide_on_host(x, data, offs, everything, dialect)
        t, host = timed(lambda: gn.decide_on_host(tb, data, offs, policy, dialect))
        keep("host", t)
        gx.scan(x)
        x_kept, x_bytes = gx.totals(x)
        keep("scan", between(lambda: gx.scan(tb.select))[0])
        t, (kept, kept_bytes) = timed(lambda: gx.totals(tb.select))
        keep("totals", t)
        t, x_out = between(lambda: gx.gather(x, x_kept, x_bytes, "walk"))
        keep("gather_walk", t)
        t, out = between(lambda: gn.emit(tb, kept, kept_bytes))
        keep("emit", t)
        t, (out_bytes, indices) = timed(lambda: gn.collect(tb, out, kept, host))
        keep("d2h", t)
        assert out_bytes == want.data and indices == want.indices
        del x, tb, buf, offs_dev, out, x_out
        t, (again, _) = timed(lambda: gn.normalise(data, policy, dev, dialect))
        assert again == want
        keep("normalise_gpu_wall", t)
        keep("extract_gpu_wall", timed(lambda: gx.extract(data, everything, dev, dialect))[0])

    mid = {name: statistics.median(v) for name, v in seen.items()}
    total = sum(mid[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "dialect": dialect, "undecoded": policy.undecoded, "reps": reps,
        "decoded_events": want.events, "rewritten": want.rewritten, "host_frames": host_frames,
        "out_frames": len(want.indices), "out_bytes": len(want.data),
        "stages_us": {s: round(mid[s] * 1e6, 1) for s in STAGES + YARDSTICKS},
        "stages_us_spread": {s: [round(min(seen[s]) * 1e6, 1), round(max(seen[s]) * 1e6, 1)] for s in STAGES + YARDSTICKS},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "classify_vs_select_mark": round(mid["classify"] / mid["select_mark"], 2),
        "emit_vs_gather_walk": round(mid["emit"] / mid["gather_walk"], 2),
        "normalise_gpu_wall_ms": round(mid["normalise_gpu_wall"] * 1e3, 3),
        "normalise_gpu_wall_ms_spread": [round(f(seen["normalise_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "normalise_gpu_wall_ns_per_event": round(mid["normalise_gpu_wall"] / events * 1e9, 2),
        "normalise_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "extract_gpu_wall_ms": round(mid["extract_gpu_wall"] * 1e3, 3),
        "extract_gpu_wall_ms_spread": [round(f(seen["extract_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "wall_vs_extract_gpu": round(mid["normalise_gpu_wall"] / mid["extract_gpu_wall"], 2),
        "normalise_cpu_ms": round(cpu_s * 1e3, 1),
        "normalise_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_normalise_cpu": round(mid["normalise_gpu_wall"] / cpu_s, 4),
    }


def one(a: argparse.Namespace) -> int:
    """The child: one (size, stream), one JSON line on stdout."""
    import torch

    from beholder_amd.normalise import Policy
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    label, events = a.one.rsplit(":", 1)
    result = probe(make_stream(label, int(events)), label, int(events), a.reps, "cuda:0", Policy(a.undecoded))
    print(json.dumps(result), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,2097152", help="stream sizes, comma-separated")
    ap.add_argument("--media", default="200,10000,200000", help="media counts of the Workload streams")
    ap.add_argument("--undecoded", choices=["keep", "drop"], default="keep")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds each (size, stream) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_normalise", "probe.jsonl"))
    ap.add_argument("--one", metavar="STREAM:EVENTS", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    cases = [(label, events) for events in (int(x) for x in a.events.split(","))
             for label in ["corpus"] + [f"media-{int(m)}" for m in a.media.split(",") if m]]
    with open(a.out, "a", encoding="utf-8") as log:
        for label, events in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{label}:{events}", "--undecoded", a.undecoded,
                   "--reps", str(a.reps)]
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
