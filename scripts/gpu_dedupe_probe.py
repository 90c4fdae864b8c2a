"""Price ``dedupe`` on the GPU against the CPU dedupe, stage by stage (MI355X box).

``python -m beholder_amd dedupe --device gpu`` drops the byte-identical repeat frames of a captured
stream with ops/hip/telemetry_dedupe.hip (beholder_amd/dedupe.py defines the result). This script
times, for each stream size and each stream, under the default policy (``last``, all topics):

* frame_index: the host's one pass over the length headers (the only per-event host work);
* h2d: the stream and its offsets to HBM, from pageable memory as ``dedupe_gpu`` does it;
* hash / claim: the two kernels whose loops walk the content, by HIP events, each a launch of its
  own, in both forms (``wide``: 8 bytes a step, ``bytes``: one);
* mark: the third kernel;
* host_decide: the overflow count read back, and the host's decisions where there are any;
* scan / gather: the extract's kernels over this ``keep_len``, by HIP events;
* totals: the one word read back to size the output;
* d2h: the output bytes, the kept indices and the kept frames' hashes back to the host;
* dedupe_gpu_wall: the whole of ``gpu_dedupe.dedupe`` as the command runs it, allocation included,
  in both forms.

Streams: ``distinct``, Workload events over 10,000 media with no forced repeats; ``half``, such a
stream of half the size followed by itself; ``hot``, 128 events over 16 media repeated to the size,
so at 4M events every content occurs tens of thousands of times and all of its lanes meet in one
slot; and ``corpus``, the fold corpus mix (tests/telemetry_corpus.py ``fold_corpus``, repeated up to
the stream size). Every run is checked for equality with ``dedupe_cpu``, which is timed too.

Usage: ``gpu_dedupe_probe.py [--events 16384,262144,4194304] [--out profiles/box_dedupe/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The dedupe" cites it.
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
from beholder_amd.dedupe import Policy, dedupe_cpu  # noqa: E402
from beholder_amd.ops import gpu_dedupe as gd, gpu_extract as gx, gpu_fold  # noqa: E402
from beholder_amd.transport.framing import iter_frames  # noqa: E402

HOST_STAGES = ("frame_index", "h2d", "host_decide", "totals", "d2h")
KERNELS = ("hash_wide", "hash_bytes", "claim_wide", "claim_bytes", "mark", "scan", "gather")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def workload_stream(media: int, events: int) -> bytes:
    w = Workload(n_media=media, seed=1)
    return b"".join(w.framed(min(65536, events - k)) for k in range(0, events, 65536))


def corpus_stream(events: int) -> bytes:
    from beholder_amd.ops import frame
    from telemetry_corpus import fold_corpus
    pieces = [frame(t, b) for t, b in iter_frames(fold_corpus())]
    reps = -(-events // len(pieces))
    return b"".join((pieces * reps)[:events])


def streams(events: int):
    yield "distinct", lambda: workload_stream(10000, events)
    yield "half", lambda: workload_stream(10000, events // 2) * 2
    yield "hot", lambda: Workload(n_media=16, seed=1).framed(128) * (events // 128)
    yield "corpus", lambda: corpus_stream(events)


def probe(data: bytes, policy: Policy, label: str, events: int, reps: int, dev: str) -> dict:
    sync = torch.cuda.synchronize
    cpu_s, want = timed(lambda: dedupe_cpu(data, policy))
    wall_cold, (got, host_frames) = timed(lambda: gd.dedupe(data, policy, dev))  # loads the module: not a figure
    assert got == want, "the GPU dedupe disagrees with dedupe_cpu"
    best = {}

    def keep(name, seconds):
        best[name] = min(best.get(name, seconds), seconds)

    def event():
        return torch.cuda.Event(enable_timing=True)

    for _ in range(reps):
        t, (n, offs) = timed(lambda: gpu_fold.index(data))
        keep("frame_index", t)

        def h2d():
            out = gpu_fold.upload(data, offs, dev)
            sync()
            return out
        t, (buf, offs_dev) = timed(h2d)
        keep("h2d", t)
        tables = gd.allocate(buf, offs_dev, n)
        pairs = {}

        def kernel(name, launch):
            pairs[name] = (event(), event())
            pairs[name][0].record()
            launch()
            pairs[name][1].record()

        for method in ("bytes", "wide"):  # the default form last: mark reads what it left
            params = gd.dedupe_params(policy, tables.slots, method=method)
            tables.cursor.zero_()
            tables.claim.zero_()
            tables.winner.zero_()
            sync()
            kernel("hash_" + method, lambda: gd.launch(tables, params, stages=gd.STAGE_HASH))
            kernel("claim_" + method, lambda: gd.launch(tables, params, stages=gd.STAGE_CLAIM))
        kernel("mark", lambda: gd.launch(tables, params, stages=gd.STAGE_MARK))
        sync()
        t, _ = timed(lambda: gd.decide_on_host(tables, data, offs, policy))
        keep("host_decide", t)
        kernel("scan", lambda: gx.scan(tables.select))
        sync()
        t, (kept, kept_bytes) = timed(lambda: gx.totals(tables.select))
        keep("totals", t)
        out = None

        def gather():
            nonlocal out
            out = gx.gather(tables.select, kept, kept_bytes)
        kernel("gather", gather)
        sync()
        for name, (e0, e1) in pairs.items():
            keep(name, e0.elapsed_time(e1) * 1e-3)
        t, (out_bytes, indices, hashes) = timed(
            lambda: gd.collect(tables, out, kept, data if host_frames else None, offs))
        keep("d2h", t)
        assert out_bytes == want.data and indices == want.indices and len(hashes) == kept
        del tables, buf, offs_dev, out
        for method in gd.METHODS:
            t, (again, _) = timed(lambda: gd.dedupe(data, policy, dev, method=method))
            keep("dedupe_gpu_wall_" + method, t)
            assert again == want

    stages = HOST_STAGES + KERNELS
    chain = [s for s in stages if not s.endswith("_bytes" if gd.DEFAULT_METHOD == "wide" else "_wide")]
    total = sum(best[s] for s in chain)
    wall = best["dedupe_gpu_wall_" + gd.DEFAULT_METHOD]
    view = memoryview(data)
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "mean_content_bytes": round((len(view) - 4 * events) / events, 1),
        "kept": len(want.indices), "kept_bytes": len(want.data), "duplicates": events - len(want.indices),
        "host_frames": host_frames, "default_method": gd.DEFAULT_METHOD,
        "stages_us": {s: round(best[s] * 1e6, 1) for s in stages},
        "stages_ns_per_event": {s: round(best[s] / events * 1e9, 2) for s in stages},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "dedupe_gpu_wall_ms": {m: round(best["dedupe_gpu_wall_" + m] * 1e3, 3) for m in gd.METHODS},
        "dedupe_gpu_wall_ns_per_event": round(wall / events * 1e9, 2),
        "dedupe_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "dedupe_cpu_ms": round(cpu_s * 1e3, 1),
        "dedupe_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_dedupe_cpu": round(wall / cpu_s, 4),
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,4194304", help="stream sizes, comma-separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_dedupe", "probe.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a", encoding="utf-8") as log:
        for events in (int(x) for x in a.events.split(",")):
            for label, make in streams(events):
                line = json.dumps(probe(make(), Policy(), label, events, a.reps, "cuda:0"))
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
