"""Price ``export`` on the GPU against ``normalise`` on the same stream, stage by stage (MI355X box).

``python -m beholder_amd export --device gpu`` writes a capture as NDJSON rows with
ops/hip/telemetry_export.hip (beholder_amd/export.py defines the result). The nearest existing code
is the normalise (ops/hip/telemetry_normalise.hip): the same index, upload, classify, scan and emit
over the same frames, writing frames where the export writes text three to five times as long. This
script times, for each stream size and each stream:

* frame_index: the host's one pass over the length headers;
* h2d: the stream and its offsets to HBM, from pageable memory as ``export_gpu`` does it;
* classify against normalise_classify, and emit against normalise_emit: the kernels, by HIP events;
* host: ``decide_on_host``, which reads the counters and writes the rows of the frames left to the host;
* size: the reduction over ``keep_len`` that sizes the output before the scan;
* scan: the extract's launches over ``keep_len``, by HIP events; totals: the one word read back;
* d2h: the rows and the indices back to the host, the host's rows spliced in;
* export_gpu_wall and normalise_gpu_wall: the whole calls as the commands run them, allocation
  included; export_cpu and normalise_cpu: the definitions, once each.

Every figure is the median of ``--reps`` repeats after one warm-up call that loads the module, with
the least and the most next to it (``*_spread``). Every run is checked for equality with
``export_cpu``.

Streams, in the protobufjs dialect: Workload events, half of them progress events, over 200, 10,000
and 200,000 media; and ``corpus``, the fold corpus mix (tests/telemetry_corpus.py ``fold_corpus``,
repeated up to the stream size), which has malformed bodies that become base64 rows, strings with
escapes and non-ASCII ids that go to the host.

Every (size, stream) runs in a fresh child process under its own time limit (``--limit`` seconds);
the first one that fails or runs out of time ends the probe, and nothing more is started.

Usage: ``gpu_export_probe.py [--events 16384,262144,2097152] [--media 200,10000,200000]
[--undecoded keep] [--reps 7] [--limit 240] [--out profiles/box_export/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The export" cites it.
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

STAGES = ("frame_index", "h2d", "classify", "host", "size", "scan", "totals", "emit", "d2h")
YARDSTICKS = ("normalise_classify", "normalise_emit")
WALLS = ("export_gpu_wall", "normalise_gpu_wall")


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

    from beholder_amd.export import export_cpu
    from beholder_amd.normalise import normalise_cpu
    from beholder_amd.ops import gpu_export as gx, gpu_extract, gpu_fold, gpu_normalise as gn
    sync = torch.cuda.synchronize
    dialect = "protobufjs"

    def between(fn):
        """Seconds of device time that ``fn``'s launches take, by HIP events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    cpu_s, want = timed(lambda: export_cpu(data, policy, dialect))
    normalise_cpu_s, canonical = timed(lambda: normalise_cpu(data, policy, dialect))
    wall_cold, (got, host_frames) = timed(lambda: gx.export(data, policy, dev, dialect))  # loads the module: no figure
    assert got == want, "the GPU export disagrees with export_cpu"
    assert gn.normalise(data, policy, dev, dialect)[0] == canonical
    seen = {}

    def keep(name, seconds):
        seen.setdefault(name, []).append(seconds)

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
        y = gn.allocate(buf, offs_dev, n)
        tb = gx.allocate(buf, offs_dev, n)
        sync()
        keep("normalise_classify", between(lambda: gn.classify(y, policy, dialect))[0])
        keep("classify", between(lambda: gx.classify(tb, policy, dialect))[0])
        y_host = gn.decide_on_host(y, data, offs, policy, dialect)
        t, host = timed(lambda: gx.decide_on_host(tb, data, offs, policy, dialect))
        keep("host", t)
        keep("size", timed(lambda: gx.out_bytes(tb))[0])
        gpu_extract.scan(y.select)
        y_kept, y_bytes = gpu_extract.totals(y.select)
        keep("scan", between(lambda: gpu_extract.scan(tb.select))[0])
        t, (kept, kept_bytes) = timed(lambda: gpu_extract.totals(tb.select))
        keep("totals", t)
        t, y_out = between(lambda: gn.emit(y, y_kept, y_bytes))
        keep("normalise_emit", t)
        t, out = between(lambda: gx.emit(tb, kept, kept_bytes))
        keep("emit", t)
        t, (rows, indices) = timed(lambda: gx.collect(tb, out, kept, host))
        keep("d2h", t)
        assert rows == want.data and indices == want.indices
        del y, tb, buf, offs_dev, out, y_out, y_host
        t, (again, _) = timed(lambda: gx.export(data, policy, dev, dialect))
        assert again == want
        keep("export_gpu_wall", t)
        keep("normalise_gpu_wall", timed(lambda: gn.normalise(data, policy, dev, dialect))[0])

    mid = {name: statistics.median(v) for name, v in seen.items()}
    total = sum(mid[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "dialect": dialect, "undecoded": policy.undecoded, "reps": reps,
        "decoded_events": want.events, "host_frames": host_frames,
        "rows": len(want.indices), "out_bytes": len(want.data), "out_vs_in_bytes": round(len(want.data) / len(data), 2),
        "normalise_out_bytes": len(canonical.data),
        "stages_us": {s: round(mid[s] * 1e6, 1) for s in STAGES + YARDSTICKS},
        "stages_us_spread": {s: [round(min(seen[s]) * 1e6, 1), round(max(seen[s]) * 1e6, 1)] for s in STAGES + YARDSTICKS},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "classify_vs_normalise_classify": round(mid["classify"] / mid["normalise_classify"], 2),
        "emit_vs_normalise_emit": round(mid["emit"] / mid["normalise_emit"], 2),
        "emit_gb_per_s_written": round(len(want.data) / mid["emit"] * 1e-9, 2),
        "export_gpu_wall_ms": round(mid["export_gpu_wall"] * 1e3, 3),
        "export_gpu_wall_ms_spread": [round(f(seen["export_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "export_gpu_wall_ns_per_event": round(mid["export_gpu_wall"] / events * 1e9, 2),
        "export_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "normalise_gpu_wall_ms": round(mid["normalise_gpu_wall"] * 1e3, 3),
        "normalise_gpu_wall_ms_spread": [round(f(seen["normalise_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "wall_vs_normalise_gpu": round(mid["export_gpu_wall"] / mid["normalise_gpu_wall"], 2),
        "export_cpu_ms": round(cpu_s * 1e3, 1),
        "export_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "normalise_cpu_ms": round(normalise_cpu_s * 1e3, 1),
        "wall_vs_export_cpu": round(mid["export_gpu_wall"] / cpu_s, 4),
    }


def one(a: argparse.Namespace) -> int:
    """The child: one (size, stream), one JSON line on stdout."""
    import torch

    from beholder_amd.export import Policy
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_export", "probe.jsonl"))
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
