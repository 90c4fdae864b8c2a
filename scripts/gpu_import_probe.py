"""Price ``import`` on the GPU stage by stage, against ``import_cpu`` and against the export's stages
for the same capture (MI355X box).

``python -m beholder_amd import --device gpu`` reads NDJSON rows back into a framed stream with
ops/hip/telemetry_import.hip (beholder_amd/import_rows.py defines the result). Its input is the
export of a capture, so the nearest existing code is the export (ops/hip/telemetry_export.hip) run the
other way: it reads the frames and writes the text that the import reads to write the frames. This
script builds a capture, exports it, and times, for each capture size and each capture:

* h2d: the text to HBM, from pageable memory as ``import_gpu`` does it;
* split: the count, the scan over the tiles, the one word read back and the starts, by wall clock
  with a synchronise (it holds a readback); split_kernels: the same launches by HIP events, which hold
  the readback too;
* classify and emit: the kernels, by HIP events, against export_classify and export_emit for the
  capture the text came from;
* host: ``decide_on_host``, which reads the counters and builds the frames of the rows left to the host;
* scan: the extract's launches over ``keep_len``, by HIP events; totals: the one word read back;
* d2h: the frames and the line positions back to the host, the host's frames spliced in;
* import_gpu_wall and export_gpu_wall: the whole calls as the commands run them, allocation included;
  import_cpu and export_cpu: the definitions, once each.

Every figure is the median of ``--reps`` repeats after one warm-up call that loads the module, with
the least and the most next to it (``*_spread``). Every run is checked for equality with
``import_cpu``, and ``import_cpu``'s frames with ``normalise_cpu`` of the capture. No figure has a
threshold.

Captures, in the protobufjs dialect: Workload events, half of them progress events, over 10,000
media; and ``corpus``, the fold corpus mix (tests/telemetry_corpus.py ``fold_corpus``, repeated up to
the capture size), whose export has base64 rows, strings with escapes and non-ASCII rows that go to
the host.

Every (size, capture) runs in a fresh child process under its own time limit (``--limit`` seconds);
the first one that fails or runs out of time ends the probe, and nothing more is started.

Usage: ``gpu_import_probe.py [--events 16384,262144,2097152] [--media 10000] [--reps 7] [--limit 240]
[--out import_probe.jsonl]``.
Output: one JSON object per (size, capture) on stdout and appended to ``--out``.
docs/DESIGN.md "The import" cites it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # telemetry_corpus
sys.path.insert(2, os.path.join(ROOT, "scripts"))

from gpu_export_probe import make_stream, timed  # noqa: E402  the captures the export's probe prices

STAGES = ("h2d", "split", "classify", "host", "scan", "totals", "emit", "d2h")
YARDSTICKS = ("split_kernels", "export_classify", "export_emit")
WALLS = ("import_gpu_wall", "export_gpu_wall")


def probe(capture: bytes, label: str, events: int, reps: int, dev: str) -> dict:
    import torch

    from beholder_amd import export as ex, import_rows as im, normalise as nm
    from beholder_amd.ops import gpu_export as gx, gpu_extract, gpu_fold, gpu_import as gi
    sync = torch.cuda.synchronize
    dialect = "protobufjs"
    policy = im.Policy("fail")

    def between(fn):
        """Seconds of device time that ``fn``'s launches take, by HIP events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    export_cpu_s, exported = timed(lambda: ex.export_cpu(capture, ex.Policy(), dialect))
    text = exported.data
    cpu_s, want = timed(lambda: im.import_cpu(text, policy))
    assert want.data == nm.normalise_cpu(capture, nm.Policy(), dialect).data, "import of an export is not the normalise"
    wall_cold, (got, host_rows) = timed(lambda: gi.import_rows(text, policy, dev))  # loads the module: no figure
    assert got == want, "the GPU import disagrees with import_cpu"
    assert gx.export(capture, ex.Policy(), dev, dialect)[0] == exported
    seen = {}

    def keep(name, seconds):
        seen.setdefault(name, []).append(seconds)

    for _ in range(reps):
        def h2d():
            out = gi.upload(text, dev)
            sync()
            return out
        t, buf = timed(h2d)
        keep("h2d", t)

        def split():
            out = gi.split(buf)
            sync()
            return out
        t, lines = timed(split)
        keep("split", t)
        keep("split_kernels", between(lambda: gi.split(buf))[0])
        # the yardstick: the export's kernels over the capture the text came from
        n, offs = gpu_fold.index(capture)
        cap, offs_dev = gpu_fold.upload(capture, offs, dev)
        y = gx.allocate(cap, offs_dev, n)
        tb = gi.allocate(buf, lines.starts, lines.n)
        sync()
        keep("export_classify", between(lambda: gx.classify(y, ex.Policy(), dialect))[0])
        keep("classify", between(lambda: gi.classify(tb))[0])
        y_host = gx.decide_on_host(y, capture, offs, ex.Policy(), dialect)
        t, host = timed(lambda: gi.decide_on_host(tb, text, policy))
        keep("host", t)
        gpu_extract.scan(y.select)
        y_kept, y_bytes = gpu_extract.totals(y.select)
        keep("scan", between(lambda: gpu_extract.scan(tb.select))[0])
        t, (kept, kept_bytes) = timed(lambda: gpu_extract.totals(tb.select))
        keep("totals", t)
        t, y_out = between(lambda: gx.emit(y, y_kept, y_bytes))
        keep("export_emit", t)
        t, out = between(lambda: gi.emit(tb, kept, kept_bytes))
        keep("emit", t)
        t, (frames, positions) = timed(lambda: gi.collect(tb, out, kept, host))
        keep("d2h", t)
        assert frames == want.data and positions == want.lines
        del y, tb, buf, cap, offs_dev, out, y_out, y_host, lines
        t, (again, _) = timed(lambda: gi.import_rows(text, policy, dev))
        assert again == want
        keep("import_gpu_wall", t)
        keep("export_gpu_wall", timed(lambda: gx.export(capture, ex.Policy(), dev, dialect))[0])

    mid = {name: statistics.median(v) for name, v in seen.items()}
    total = sum(mid[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "capture": label, "events": events, "capture_bytes": len(capture),
        "text_bytes": len(text), "lines": want.line_count, "dialect": dialect, "reps": reps,
        "frames": len(want.lines), "from_json": want.events, "from_b64": want.carried, "host_rows": host_rows,
        "out_bytes": len(want.data), "out_vs_in_bytes": round(len(want.data) / len(text), 3),
        "stages_us": {s: round(mid[s] * 1e6, 1) for s in STAGES + YARDSTICKS},
        "stages_us_spread": {s: [round(min(seen[s]) * 1e6, 1), round(max(seen[s]) * 1e6, 1)] for s in STAGES + YARDSTICKS},
        "stage_sum_ns_per_line": round(total / want.line_count * 1e9, 2),
        "classify_vs_export_classify": round(mid["classify"] / mid["export_classify"], 2),
        "emit_vs_export_emit": round(mid["emit"] / mid["export_emit"], 2),
        "split_gb_per_s_read": round(2 * len(text) / mid["split_kernels"] * 1e-9, 2),
        "classify_gb_per_s_read": round(len(text) / mid["classify"] * 1e-9, 2),
        "import_gpu_wall_ms": round(mid["import_gpu_wall"] * 1e3, 3),
        "import_gpu_wall_ms_spread": [round(f(seen["import_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "import_gpu_wall_ns_per_line": round(mid["import_gpu_wall"] / want.line_count * 1e9, 2),
        "import_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "export_gpu_wall_ms": round(mid["export_gpu_wall"] * 1e3, 3),
        "export_gpu_wall_ms_spread": [round(f(seen["export_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "wall_vs_export_gpu": round(mid["import_gpu_wall"] / mid["export_gpu_wall"], 2),
        "import_cpu_ms": round(cpu_s * 1e3, 1),
        "import_cpu_ns_per_line": round(cpu_s / want.line_count * 1e9, 1),
        "export_cpu_ms": round(export_cpu_s * 1e3, 1),
        "wall_vs_import_cpu": round(mid["import_gpu_wall"] / cpu_s, 4),
    }


def one(a: argparse.Namespace) -> int:
    """The child: one (size, capture), one JSON line on stdout."""
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    label, events = a.one.rsplit(":", 1)
    print(json.dumps(probe(make_stream(label, int(events)), label, int(events), a.reps, "cuda:0")), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,2097152", help="capture sizes, comma-separated")
    ap.add_argument("--media", default="10000", help="media counts of the Workload captures")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds each (size, capture) may take")
    ap.add_argument("--out", default="import_probe.jsonl")
    ap.add_argument("--one", metavar="CAPTURE:EVENTS", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    cases = [(label, events) for events in (int(x) for x in a.events.split(","))
             for label in ["corpus"] + [f"media-{int(m)}" for m in a.media.split(",") if m]]
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
