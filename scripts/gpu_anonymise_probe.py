"""Price ``anonymise`` on the GPU against ``normalise`` on the same capture, stage by stage (MI355X box).

``python -m beholder_amd anonymise --device gpu`` replaces every mediaId and host by a keyed pseudonym
with ops/hip/telemetry_anonymise.hip (beholder_amd/anonymise.py defines the result). Its stages are
the normalise's (ops/gpu_normalise.py) plus one new piece of work, a keyed BLAKE2s per chosen string
in classify, so the yardstick is the normalise on the same upload in the same process: the normalise's
classify is the anonymise's with both strings kept. This script times, for each stream size and stream:

* frame_index and h2d: the host's pass over the length headers and the upload, shared by both;
* classify (both strings replaced) against nm_classify, and classify_media and classify_host (one
  string replaced): the kernels, by HIP events. ``hash_share`` is 1 - nm_classify / classify;
* host: ``decide_on_host``; scan and totals: the extract's, over this module's ``keep_len``;
* emit against nm_emit: the kernels, by HIP events;
* d2h: the output and the indices back to the host, the host's frames spliced in;
* anonymise_gpu_wall and normalise_gpu_wall: the whole calls as the commands run them, allocation
  included; anonymise_cpu: the definition, once.

Every figure is the median of ``--reps`` repeats after one warm-up call that loads the module, with
the least and the most next to it (``*_spread``). The yardstick and the new kernels alternate on one
upload. Every run is checked for equality with ``anonymise_cpu``.

Streams, in the protobufjs dialect: Workload events, half of them progress events, over 200, 10,000
and 200,000 media (ids of 36 bytes, hosts of 8: one compression per string); and ``corpus``, the fold
corpus mix (tests/telemetry_corpus.py ``fold_corpus``, repeated up to the stream size), which has
malformed bodies and non-ASCII ids that go to the host.

Every (size, stream) runs in a fresh child process under its own time limit (``--limit`` seconds);
the first one that fails or runs out of time ends the probe, and nothing more is started.

Usage: ``gpu_anonymise_probe.py [--events 16384,262144,2097152] [--media 200,10000,200000]
[--undecoded drop] [--reps 7] [--limit 240] [--out profiles/box_anonymise/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The anonymise" cites it.
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
sys.path.insert(2, os.path.dirname(os.path.abspath(__file__)))

from gpu_normalise_probe import make_stream, timed  # noqa: E402  the same streams, the same clock

STAGES = ("frame_index", "h2d", "classify", "host", "scan", "totals", "emit", "d2h")
YARDSTICKS = ("nm_classify", "nm_emit", "classify_media", "classify_host")
KEY = bytes(range(32))


def probe(data: bytes, label: str, events: int, reps: int, dev: str, undecoded: str) -> dict:
    import torch

    from beholder_amd import anonymise as an, normalise as nm
    from beholder_amd.ops import gpu_anonymise as ga, gpu_extract as gx, gpu_fold, gpu_normalise as gn
    sync = torch.cuda.synchronize
    dialect = "protobufjs"
    policy = an.Policy(KEY, undecoded)
    one_field = {"classify_media": an.Policy(KEY, undecoded, {"mediaId"}),
                 "classify_host": an.Policy(KEY, undecoded, {"host"})}
    yard = nm.Policy(undecoded)

    def between(fn):
        """Seconds of device time that ``fn``'s launches take, by HIP events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    cpu_s, want = timed(lambda: an.anonymise_cpu(data, policy, dialect))
    # the first call loads the module: no figure
    wall_cold, (got, host_frames) = timed(lambda: ga.anonymise(data, policy, dev, dialect))
    assert got == want, "the GPU anonymise disagrees with anonymise_cpu"
    gn.normalise(data, yard, dev, dialect)
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
        x = gn.allocate(buf, offs_dev, n)
        tb = ga.allocate(buf, offs_dev, n)
        sync()
        keep("nm_classify", between(lambda: gn.classify(x, yard, dialect))[0])
        keep("classify", between(lambda: ga.classify(tb, policy, dialect))[0])
        for name, other in one_field.items():
            extra = ga.allocate(buf, offs_dev, n)
            sync()
            keep(name, between(lambda: ga.classify(extra, other, dialect))[0])
            del extra
        x_host = gn.decide_on_host(x, data, offs, yard, dialect)
        t, host = timed(lambda: ga.decide_on_host(tb, data, offs, policy, dialect))
        keep("host", t)
        gx.scan(x.select)
        x_kept, x_bytes = gx.totals(x.select)
        keep("scan", between(lambda: gx.scan(tb.select))[0])
        t, (kept, kept_bytes) = timed(lambda: gx.totals(tb.select))
        keep("totals", t)
        t, x_out = between(lambda: gn.emit(x, x_kept, x_bytes))
        keep("nm_emit", t)
        t, out = between(lambda: ga.emit(tb, kept, kept_bytes))
        keep("emit", t)
        t, (out_bytes, indices) = timed(lambda: ga.collect(tb, out, kept, host))
        keep("d2h", t)
        assert out_bytes == want.data and indices == want.indices
        del x, tb, buf, offs_dev, out, x_out, x_host
        t, (again, _) = timed(lambda: ga.anonymise(data, policy, dev, dialect))
        assert again == want
        keep("anonymise_gpu_wall", t)
        keep("normalise_gpu_wall", timed(lambda: gn.normalise(data, yard, dev, dialect))[0])

    mid = {name: statistics.median(v) for name, v in seen.items()}
    total = sum(mid[s] for s in STAGES)
    return {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "dialect": dialect, "undecoded": undecoded, "reps": reps,
        "decoded_events": want.events, "host_frames": host_frames,
        "out_frames": len(want.indices), "out_bytes": len(want.data),
        "stages_us": {s: round(mid[s] * 1e6, 1) for s in STAGES + YARDSTICKS},
        "stages_us_spread": {s: [round(f(seen[s]) * 1e6, 1) for f in (min, max)] for s in STAGES + YARDSTICKS},
        "stage_sum_ns_per_event": round(total / events * 1e9, 2),
        "classify_vs_nm_classify": round(mid["classify"] / mid["nm_classify"], 2),
        "hash_share": round(1 - mid["nm_classify"] / mid["classify"], 3),
        "classify_ns_per_event": round(mid["classify"] / events * 1e9, 3),
        "emit_vs_nm_emit": round(mid["emit"] / mid["nm_emit"], 2),
        "anonymise_gpu_wall_ms": round(mid["anonymise_gpu_wall"] * 1e3, 3),
        "anonymise_gpu_wall_ms_spread": [round(f(seen["anonymise_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "anonymise_gpu_wall_ns_per_event": round(mid["anonymise_gpu_wall"] / events * 1e9, 2),
        "anonymise_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "normalise_gpu_wall_ms": round(mid["normalise_gpu_wall"] * 1e3, 3),
        "normalise_gpu_wall_ms_spread": [round(f(seen["normalise_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "wall_vs_normalise_gpu": round(mid["anonymise_gpu_wall"] / mid["normalise_gpu_wall"], 2),
        "anonymise_cpu_ms": round(cpu_s * 1e3, 1),
        "anonymise_cpu_ns_per_event": round(cpu_s / events * 1e9, 1),
        "wall_vs_anonymise_cpu": round(mid["anonymise_gpu_wall"] / cpu_s, 4),
    }


def one(a: argparse.Namespace) -> int:
    """The child: one (size, stream), one JSON line on stdout."""
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    label, events = a.one.rsplit(":", 1)
    result = probe(make_stream(label, int(events)), label, int(events), a.reps, "cuda:0", a.undecoded)
    print(json.dumps(result), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,2097152", help="stream sizes, comma-separated")
    ap.add_argument("--media", default="200,10000,200000", help="media counts of the Workload streams")
    ap.add_argument("--undecoded", choices=["keep", "drop"], default="drop")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds each (size, stream) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_anonymise", "probe.jsonl"))
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
