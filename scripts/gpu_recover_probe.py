"""Price ``recover`` on the GPU stage by stage, against the definition and the host's framing walk (MI355X box).

``python -m beholder_amd recover --device gpu`` finds the frames of a damaged capture with
ops/hip/telemetry_recover.hip (beholder_amd/recover.py defines the result). Its tables are per byte
offset, though only a few percent of the offsets are nodes of the walk, so what it costs next to the
host's serial walk is the question. This script times, for each stream size, an intact stream and
the same stream with four damages:

* h2d: the bytes to HBM, padded, from pageable memory as ``recover_gpu`` does it;
* candidates, next_anchor, reach: the kernels, by HIP events;
* host: ``decide_on_host``, which reads the overflow list's length and decides those offsets;
* collect: mark, the extract's scan, the total read back, resolve and the node lists to the host;
* assemble: the host cuts the gaps out of its own copy;
* recover_gpu_wall: the whole call as the command runs it, allocation included; recover_cpu: the
  definition, once; and for the intact stream frame_index, ``ops.native.frame_index``, the one pass
  over the length headers that every other command starts with.

Every figure is the median of ``--reps`` repeats after one warm-up call that loads the module, with
the least and the most next to it (``*_spread``). Every run is checked for equality with
``recover_cpu``.

Streams: Workload events, half of them progress events, over 10,000 media. The damaged one has the
first header byte of frame ``3k // 4`` XORed with 0x04, 300 random bytes before frame ``k // 2``,
the bytes from 3 into frame ``k // 4`` to 1 into frame ``k // 4 + 2`` deleted, and its last 3 bytes
dropped.

Every (size, stream) runs in a fresh child process under its own time limit (``--limit`` seconds);
the first one that fails or runs out of time ends the probe, and nothing more is started.

Usage: ``gpu_recover_probe.py [--events 16384,262144,2097152] [--dialect protobufjs] [--reps 5]
[--limit 240] [--out profiles/box_recover/probe.jsonl]``.
Output: one JSON object per (size, stream) on stdout and appended to ``--out``.
docs/DESIGN.md "The recover" cites it.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("h2d", "candidates", "host", "next_anchor", "reach", "collect", "assemble")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def make_stream(label: str, events: int) -> bytes:
    from beholder_amd.bench.generator import Workload
    from beholder_amd.capture_io import frame_spans
    w = Workload(n_media=10000, seed=1, progress_fraction=0.5)
    data = bytearray(b"".join(w.framed(min(65536, events - k)) for k in range(0, events, 65536)))
    if label == "intact":
        return bytes(data)
    spans = list(frame_spans(bytes(data)))
    k = len(spans)
    data[spans[3 * k // 4][0]] ^= 0x04
    rng = random.Random(7)
    at = spans[k // 2][0]
    data[at:at] = bytes(rng.randrange(256) for _ in range(300))
    del data[spans[k // 4][0] + 3:spans[k // 4 + 2][0] + 1]
    del data[-3:]
    return bytes(data)


def probe(data: bytes, label: str, events: int, reps: int, dev: str, dialect: str) -> dict:
    import torch

    from beholder_amd import ops
    from beholder_amd.ops import gpu_recover as gr
    from beholder_amd.recover import Policy, recover_cpu
    sync = torch.cuda.synchronize
    policy = Policy()

    def between(fn):
        """Seconds of device time that ``fn``'s launches take, by HIP events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3, out

    cpu_s, want = timed(lambda: recover_cpu(data, policy, dialect))
    wall_cold, (got, host_offsets) = timed(lambda: gr.recover(data, policy, dev, dialect))  # loads the module: no figure
    assert got == want, "the GPU recover disagrees with recover_cpu"
    seen = {}

    def keep(name, seconds):
        seen.setdefault(name, []).append(seconds)

    for _ in range(reps):
        def h2d():
            out = gr.upload(data, dev)
            sync()
            return out
        t, buf = timed(h2d)
        keep("h2d", t)
        tb = gr.allocate(buf, len(data), policy)
        sync()
        keep("candidates", between(lambda: gr.candidates(tb, dialect))[0])
        keep("host", timed(lambda: gr.decide_on_host(tb, data, policy, dialect))[0])
        keep("next_anchor", between(lambda: gr.next_anchor(tb))[0])
        keep("reach", between(lambda: gr.reach(tb))[0])
        t, nodes = timed(lambda: gr.collect(tb))
        keep("collect", t)
        t, out = timed(lambda: gr.assemble(nodes, data, policy, dialect, True, False))
        keep("assemble", t)
        assert out == want
        del tb, buf
        t, (again, _) = timed(lambda: gr.recover(data, policy, dev, dialect))
        assert again == want
        keep("recover_gpu_wall", t)
        if label == "intact":
            keep("frame_index", timed(lambda: ops.native.frame_index(data))[0])

    mid = {name: statistics.median(v) for name, v in seen.items()}
    result = {
        "device": torch.cuda.get_device_name(0), "stream": label, "events": events, "bytes": len(data),
        "dialect": dialect, "reps": reps, "frames": want.frames, "anchors": want.anchors, "gaps": len(want.gaps),
        "host_offsets": host_offsets, "rounds": (len(data) // 5 + 1).bit_length(),
        "stages_us": {s: round(mid[s] * 1e6, 1) for s in STAGES},
        "stages_us_spread": {s: [round(min(seen[s]) * 1e6, 1), round(max(seen[s]) * 1e6, 1)] for s in STAGES},
        "stage_sum_ns_per_byte": round(sum(mid[s] for s in STAGES) / len(data) * 1e9, 3),
        "recover_gpu_wall_ms": round(mid["recover_gpu_wall"] * 1e3, 3),
        "recover_gpu_wall_ms_spread": [round(f(seen["recover_gpu_wall"]) * 1e3, 3) for f in (min, max)],
        "recover_gpu_first_call_ms": round(wall_cold * 1e3, 1),
        "recover_cpu_ms": round(cpu_s * 1e3, 1),
        "wall_vs_recover_cpu": round(mid["recover_gpu_wall"] / cpu_s, 4),
    }
    if label == "intact":
        result["frame_index_ms"] = round(mid["frame_index"] * 1e3, 3)
        result["wall_vs_frame_index"] = round(mid["recover_gpu_wall"] / mid["frame_index"], 1)
    return result


def one(a: argparse.Namespace) -> int:
    """The child: one (size, stream), one JSON line on stdout."""
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return 1
    label, events = a.one.rsplit(":", 1)
    print(json.dumps(probe(make_stream(label, int(events)), label, int(events), a.reps, "cuda:0", a.dialect)), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--events", default="16384,262144,2097152", help="stream sizes, comma-separated")
    ap.add_argument("--dialect", choices=["protobufjs", "upb"], default="protobufjs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each (size, stream) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_recover", "probe.jsonl"))
    ap.add_argument("--one", metavar="STREAM:EVENTS", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    cases = [(label, events) for events in (int(x) for x in a.events.split(",")) for label in ("intact", "damaged")]
    with open(a.out, "a", encoding="utf-8") as log:
        for label, events in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{label}:{events}", "--dialect", a.dialect,
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
