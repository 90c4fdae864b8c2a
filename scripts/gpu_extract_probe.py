"""Price ``extract`` on the GPU against the CPU extract, stage by stage (MI355X box).

``python -m beholder_amd extract --device gpu`` cuts a captured stream with
ops/hip/telemetry_select.hip (beholder_amd/extract.py defines the result). This script times, for
each stream size and each of three selectivities:

* frame_index: the host's one pass over the length headers (the only per-event host work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``extract_gpu`` does it;
* table: the media table built on the host (its upload is part of ``allocate``, outside the stages);
* mark / scan / gather_search / gather_walk: the kernels, by HIP events; both gather shapes over
  the same scan;
* host_decide: the overflow count read back, and the host's decisions where there are any;
* totals: the one word read back to size the output;
* d2h: the output bytes and the kept indices back to the host;
* extract_gpu_wall: the whole of ``gpu_extract.extract`` as the command runs it, allocation included.

Selectivities: ``media`` is one media of the stream's 10,000; ``all`` is the empty selector, which
keeps every frame; ``error`` is ``--outcome error`` over the fold corpus mix (tests/telemetry_corpus.py
``fold_corpus``, repeated up to the stream size), since a Workload stream has no malformed bodies.
Every run is checked for equality with ``extract_cpu``, which is timed too.

Usage: ``gpu_extract_probe.py [--events 16384,262144,4194304] [--out profiles/box_extract/probe.jsonl]``.
Output: one JSON object per (size, selectivity) on stdout and appended to ``--out``.
docs/DESIGN.md "The extract" cites it.
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
from beholder_amd.extract import Selector, extract_cpu  # noqa: E402
from beholder_amd.ops import gpu_extract as gx, gpu_fold  # noqa: E402
from beholder_amd.transport.framing import iter_frames  # noqa: E402

STAGES = ("frame_index", "h2d", "table", "mark", "host_decide", "scan", "totals", "gather", "d2h")


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


def probe(data: bytes, selector: Selector, label: str, events: int, reps: int, dev: str) -> dict:
    sync = torch.cuda.synchronize
    cpu_s, want = timed(lambda: extract_cpu(data, selector))
    wall_cold, (got, host_frames) = timed(lambda: gx.extract(data, selector, dev))  # loads the module: not a figure
    assert got == want, "the GPU extract disagrees with extract_cpu"
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
        ids = gx.ascii_ids(selector.media)
        t, (table, blob) = timed(lambda: gx.build_media_table(ids))
        keep("table", t)
        params = gx.select_params(selector, len(table))
        tables = gx.allocate(buf, offs_dev, n, table, blob)
        sync()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        e[0].record()
        gx.mark(tables, params)
        e[1].record()
        e[1].synchronize()
        t, _ = timed(lambda: gx.decide_on_host(tables, data, offs, selector))
        keep("host_decide", t)
        e[2].record()
        gx.scan(tables)
        e[3].record()
        e[3].synchronize()
        t, (kept, kept_bytes) = timed(lambda: gx.totals(tables))
        keep("totals", t)
        outs = {}
        for k, shape in enumerate(sorted(gx.GATHER_SHAPES)):
            e[4 + 2 * k].record()
            outs[shape] = gx.gather(tables, kept, kept_bytes, shape)
            e[5 + 2 * k].record()
            e[5 + 2 * k].synchronize()
            keep("gather_" + shape, e[4 + 2 * k].elapsed_time(e[5 + 2 * k]) * 1e-3)
        keep("mark", e[0].elapsed_time(e[1]) * 1e-3)
        keep("scan", e[2].elapsed_time(e[3]) * 1e-3)
        for shape, out in outs.items():
            t, (out_bytes, indices) = timed(lambda: gx.collect(tables, out, kept))
            assert out_bytes == want.data and indices == want.indices, shape
        keep("d2h", t)
        del tables, buf, offs_dev, outs, out
        t, _ = timed(lambda: gx.extract(data, selector, dev))
        keep("extract_gpu_wall", t)

    best["gather"] = best["gather_" + gx.DEFAULT_GATHER]
    total = sum(best[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "selectivity": label, "events": events, "bytes": len(data),
        "kept": len(want.indices), "kept_bytes": len(want.data), "host_frames": host_frames,
        "default_gather": gx.DEFAULT_GATHER,
        "stages_us": {s: round(best[s] * 1e6, 1) for s in STAGES},
        "gather_us": {s: round(best["gather_" + s] * 1e6, 1) for s in sorted(gx.GATHER_SHAPES)},
        "stages_ns_per_event": {s: round(best[s] / events * 1e9, 2) for s in STAGES},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "extract_gpu_wall_ms": round(best["extract_gpu_wall"] * 1e3, 3),
        "extract_gpu_wall_ns_per_event": round(best["extract_gpu_wall"] / events * 1e9, 2),
        "extract_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "extract_cpu_ms": round(cpu_s * 1e3, 1),
        "extract_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_extract_cpu": round(best["extract_gpu_wall"] / cpu_s, 4),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,4194304", help="stream sizes, comma-separated")
    ap.add_argument("--media", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_extract", "probe.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a", encoding="utf-8") as log:
        for events in (int(x) for x in a.events.split(",")):
            w = Workload(n_media=a.media, seed=1)
            stream = b"".join(w.framed(min(65536, events - k)) for k in range(0, events, 65536))
            cases = (("media", stream, Selector(media={w.media[a.media // 2].id})),
                     ("error", corpus_stream(events), Selector(outcomes={"error"})),
                     ("all", stream, Selector()))
            for label, data, selector in cases:
                line = json.dumps(probe(data, selector, label, events, a.reps, "cuda:0"))
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
