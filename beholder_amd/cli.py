"""Command line: ``python -m beholder_amd <command>`` (reference entry: ``node index.js``, package.json:5).

Commands
--------
run      start the service (``--source amqp|stdin|file``); the reference's only mode.
config   validate and print the effective config (secrets masked).
gen      write synthetic framed telemetry to stdout/a file (+ optional media fixture).
decode   turn a framed stream into NDJSON (debugging).
export   write a framed stream as NDJSON rows, one per frame with its index, read in the service's dialect (``export``).
import   read NDJSON rows back into a framed stream: the inverse of ``export`` (``import_rows``).
summarise  fold a framed stream into its end state: counters, comments, final statuses (``replay``).
transitions  count a framed stream's per-media status moves: the transition matrix, changes, repeats (``transitions``).
hosts    what every worker host did in a framed stream: events, media, stints, handovers, what it held (``hosts``).
stages   join both topics of a framed stream per media: what stage each is in and how far (``stages``).
extract  cut a framed stream down to selected frames, a framed stream again (``extract``).
recover  salvage the frames of a damaged framed stream: cut out the spans that fit no frame, a framed stream again (``recover``).
normalise  rewrite every decodable event of a framed stream in its canonical encoding, a framed stream again (``normalise``).
anonymise  replace every mediaId and host of a framed stream by a keyed pseudonym, a framed stream again (``anonymise``).
dedupe   drop the byte-identical repeat frames of a framed stream, a framed stream again (``dedupe``).
thin     drop the progress events that repeat their media's step, a framed stream again (``thin``).
coalesce  cut a framed stream down to the frames that set its end state, a framed stream again (``coalesce``).
shard    split a framed stream by media into N framed streams, each media's events in order (``shard``).
compare  match two framed streams frame for frame: what is only in one, what is in both, in what order (``compare``).
seed     load a media fixture into a sqlite/postgres store.
bench    run the BASELINE.json measurement configs (see ``beholder_amd.bench.harness``).
publish  publish a framed stream to an AMQP broker.

Exit codes: 0 ok, 1 runtime failure, 2 usage/config error (startup failures are
fatal — the documented fix of quirk Q10); ``compare --exit-code`` adds 3, the captures differ, and
``recover --exit-code`` adds 3, the capture was not intact.
"""
from __future__ import annotations

import argparse
import asyncio
import json
import os
import signal
import sys
from typing import List, Optional

from .config import Config, ConfigError


def _load_fixture(path: str):
    from .store import Media
    with open(path, "r", encoding="utf-8") as f:
        rows = json.load(f)
    return [Media(**r) for r in rows]


WORKER_MODULE_ENV = "BEHOLDER_WORKER_MODULE"


def worker_command() -> List[str]:
    """How ``run --workers N`` starts each worker: ``python -m beholder_amd`` with the run
    arguments. A wrapper entry module that must be in force in every worker (the bench's
    ``beholder_amd.bench.shared_worker``) opts in by naming itself in ``BEHOLDER_WORKER_MODULE``;
    the supervisor never guesses it from ``__main__`` (a launcher or test runner hosting ``run``
    would otherwise be restarted in its place)."""
    name = os.environ.get(WORKER_MODULE_ENV, "").strip() or "beholder_amd"
    return [sys.executable, "-m", name]


def cmd_run(a: argparse.Namespace) -> int:
    if a.workers and a.workers > 1:
        if a.source in ("stdin", "file"):
            print("beholder: --workers needs a shared broker transport (amqp)", file=sys.stderr)
            return 2
        from .parallel.workers import Supervisor, strip_workers_arg
        argv = strip_workers_arg(sys.argv[1:] if a.argv is None else a.argv)
        if a.metrics_port is not None:
            argv = strip_opt(argv, "--metrics-port")
        try:
            scfg = Config.load("events", path=a.config, env=dict(os.environ)).data["service"]
        except ConfigError as e:
            print(f"beholder: config error: {e}", file=sys.stderr)
            return 2
        mcfg, wcfg = scfg["metrics"], scfg.get("workers") or {}
        port = a.metrics_port if a.metrics_port is not None else (
            int(mcfg.get("port", 3000)) if mcfg.get("enabled", True) else -1)
        return Supervisor(argv, a.workers, metrics_port=port, metrics_host=str(mcfg.get("host", "0.0.0.0")),
                          command=worker_command(),
                          max_restarts=int(wcfg.get("max_restarts", 10)),
                          restart_window_s=float(wcfg.get("restart_window_s", 300.0)),
                          healthy_s=float(wcfg.get("healthy_s", 60.0)),
                          log=lambda m: print(f"beholder supervisor: {m}", file=sys.stderr)).run()
    env = dict(os.environ)
    try:
        cfg = Config.load("events", path=a.config, env=env)
    except ConfigError as e:
        print(f"beholder: config error: {e}", file=sys.stderr)
        return 2
    svc_cfg = cfg.data["service"]
    if a.source:
        svc_cfg["transport"]["kind"] = a.source
    if a.path:
        svc_cfg["transport"]["path"] = a.path
    if a.url:
        svc_cfg["transport"]["url"] = a.url
    if a.policy:
        svc_cfg["transport"]["policy"] = a.policy
    if a.dead_letter:
        svc_cfg["transport"]["dead_letter"] = a.dead_letter
    if a.format:
        svc_cfg["transport"]["format"] = a.format
    if a.log_level:
        svc_cfg["log"]["level"] = a.log_level
    if a.metrics_port is not None:
        svc_cfg["metrics"]["port"] = a.metrics_port
        svc_cfg["metrics"]["enabled"] = a.metrics_port >= 0
    if a.store:
        svc_cfg["store"]["backend"] = a.store
    elif a.media_fixture:
        svc_cfg["store"]["backend"] = "memory"  # a fixture preloads the in-memory store
    if a.dsn:
        svc_cfg["store"]["dsn"] = a.dsn
    if a.ordering:
        svc_cfg["ordering"] = a.ordering

    from .service import Service
    store = None
    if a.media_fixture:
        from .store import MemoryStore
        store = MemoryStore(_load_fixture(a.media_fixture)) if svc_cfg["store"]["backend"] == "memory" else None

    async def main() -> int:
        svc = Service(cfg, store=store)
        loop = asyncio.get_running_loop()
        for sig in (signal.SIGINT, signal.SIGTERM):
            try:
                loop.add_signal_handler(sig, svc.request_stop)
            except (NotImplementedError, RuntimeError):
                pass
        try:
            await svc.init()
            stats = await svc.run()
        finally:
            await svc.close()
        if a.stats:
            print(json.dumps(stats, default=str), file=sys.stderr)
        return 1 if svc.source_error else 0

    try:
        return asyncio.run(main())
    except ConfigError as e:
        print(f"beholder: config error: {e}", file=sys.stderr)
        return 2
    except KeyboardInterrupt:
        return 130
    except Exception as e:  # startup failure is fatal (Q10 fix)
        print(f"beholder: fatal: {type(e).__name__}: {e}", file=sys.stderr)
        return 1


_SECRET_KEYS = ("token", "key", "password", "secret", "dsn", "url")


def redact_config(obj, parent: str = ""):
    """Copy of the config with credentials masked (keys.*, tokens, passwords, DSN/URL userinfo)."""
    import re
    if isinstance(obj, dict):
        return {k: redact_config(v, k) for k, v in obj.items()}
    if isinstance(obj, list):
        return [redact_config(v, parent) for v in obj]
    if isinstance(obj, str) and any(s in parent.lower() for s in _SECRET_KEYS):
        if parent.lower() in ("dsn", "url"):
            return re.sub(r"//([^:/@]+):([^@]+)@", r"//\1:***@", obj)
        return "***" if obj else obj
    return obj


def cmd_config(a: argparse.Namespace) -> int:
    """Validate the config and print the effective (merged, env-overridden) result, secrets masked."""
    try:
        cfg = Config.load("events", path=a.config, env=dict(os.environ))
    except ConfigError as e:
        print(f"beholder: config error: {e}", file=sys.stderr)
        return 2
    out = {"source": cfg.source, "no_trello": cfg.no_trello, "config": redact_config(cfg.data)}
    print(json.dumps(out, indent=2, default=str))
    return 0


def cmd_gen(a: argparse.Namespace) -> int:
    import time

    from .bench.generator import Workload
    w = Workload(n_media=a.media, seed=a.seed, progress_fraction=a.progress_fraction,
                 unknown_media_fraction=a.unknown_fraction)
    if a.media_out:
        with open(a.media_out, "w", encoding="utf-8") as f:
            json.dump([m._asdict() for m in w.media], f)
    out = open(a.out, "wb") if a.out else sys.stdout.buffer
    try:
        if a.ndjson:
            import base64
            from .topics import TOPIC_NAMES_BY_ID
            for t, p in w.events(a.events):
                out.write((json.dumps({"topic": TOPIC_NAMES_BY_ID[t], "b64": base64.b64encode(p).decode()})
                           + "\n").encode())
            return 0
        if a.rate <= 0:
            chunk = 65536
            left = a.events
            while left > 0:
                n = min(chunk, left)
                out.write(w.framed(n))
                left -= n
            return 0
        # paced producer: emit in 1 ms slices
        from .ops import frames
        evs = w.events(a.events)
        t0 = time.perf_counter()
        sent = 0
        per_ms = max(1, int(a.rate / 1000))
        while sent < len(evs):
            due = int((time.perf_counter() - t0) * a.rate) + per_ms
            if due > sent:
                out.write(frames(evs[sent:min(due, len(evs))]))
                out.flush()
                sent = min(due, len(evs))
            else:
                time.sleep(0.0005)
        return 0
    except BrokenPipeError:
        return 0
    finally:
        if a.out:
            out.close()
        else:
            try:
                out.flush()
            except BrokenPipeError:
                pass


def cmd_decode(a: argparse.Namespace) -> int:
    from .models import proto
    from .topics import PROGRESS_ID, STATUS_ID, TOPIC_NAMES_BY_ID
    from .transport.framing import iter_frames
    data = open(a.input, "rb").read() if a.input else sys.stdin.buffer.read()
    types = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}
    from google.protobuf import json_format
    for t, p in iter_frames(data):
        rec = {"topic": TOPIC_NAMES_BY_ID[t] if t < len(TOPIC_NAMES_BY_ID) else t}
        try:
            rec["json"] = json_format.MessageToDict(proto.decode(types[t], p), preserving_proto_field_name=True)
        except Exception as e:  # noqa: BLE001
            rec["error"] = str(e)
        print(json.dumps(rec))
    return 0


def _gpu_ready(a: argparse.Namespace, module_name: str) -> bool:
    """Whether the command can go on: true under ``--device cpu``, and under ``--device gpu`` where
    torch, ``ops.<module_name>``, a device and the HIP library are all there. Where one is missing it
    says so on stderr, and the command returns 1."""
    if a.device != "gpu":
        return True
    import importlib
    try:
        import torch
        importlib.import_module(f".ops.{module_name}", __package__)  # its imports fail here, not mid-run
        from .ops import hip_lib
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU is visible")
        hip_lib.lib()
    except (ImportError, RuntimeError, OSError) as e:
        print(f"beholder: --device gpu is not available ({e}); use --device cpu", file=sys.stderr)
        return False
    return True


def cmd_summarise(a: argparse.Namespace) -> int:
    """What the service will have done once this stream has gone through (``beholder_amd.replay``)."""
    import io

    from . import replay
    if not _gpu_ready(a, "gpu_fold"):
        return 1
    try:
        source = a.input if a.input else io.BytesIO(sys.stdin.buffer.read())
        summary = replay.fold_file(source, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes)
    except ValueError as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 1
    out = {"summary": summary.to_json()}
    if a.media_fixture:
        out["prediction"] = summary.apply(_load_fixture(a.media_fixture))
    print(json.dumps(out))
    return 0


def _report(a: argparse.Namespace, module_name: str, report_file) -> int:
    """A report command: ``report_file`` over the input, read whole where it is stdin, and the report
    with its ``host_frames`` to stdout as one JSON object."""
    import io
    if not _gpu_ready(a, module_name):
        return 1
    try:
        source = a.input if a.input else io.BytesIO(sys.stdin.buffer.read())
        result, host_frames = report_file(source, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes)
    except ValueError as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 1
    out = result.to_json(per_media=a.per_media)
    out["host_frames"] = host_frames
    print(json.dumps(out))
    return 0


def cmd_transitions(a: argparse.Namespace) -> int:
    """How the media of this stream got where they end: their status moves (``beholder_amd.transitions``)."""
    from . import transitions
    return _report(a, "gpu_transitions", transitions.transitions_file)


def cmd_hosts(a: argparse.Namespace) -> int:
    """What every worker host did in this stream, and what it held at the end (``beholder_amd.hosts``)."""
    from . import hosts
    return _report(a, "gpu_hosts", hosts.hosts_file)


def cmd_stages(a: argparse.Namespace) -> int:
    """Both topics of this stream joined per media: the stage every media is in and how far (``beholder_amd.stages``)."""
    from . import stages
    return _report(a, "gpu_stages", stages.stages_file)


def _topic_byte(text: str) -> int:
    from .topics import PROGRESS_ID, STATUS_ID
    named = {"status": STATUS_ID, "progress": PROGRESS_ID}
    value = named[text] if text in named else int(text)
    if not 0 <= value <= 255:
        raise ValueError(f"topic {text!r} is no byte (0-255)")
    return value


def _status_number(text: str) -> int:
    from . import replay
    by_name = {name.upper(): number for number, name in replay.status_names().items()}
    if text.upper() in by_name:
        return by_name[text.upper()]
    try:
        return int(text)
    except ValueError:
        raise ValueError(f"unknown status {text!r} ({'|'.join(sorted(by_name))} or a number 0-63)") from None


def cmd_extract(a: argparse.Namespace) -> int:
    """Cut a framed stream down to the selected frames (``beholder_amd.extract``)."""
    from . import extract
    try:
        media = None
        if a.media or a.media_file:
            media = set(a.media or ())
            for name in a.media_file or ():
                with open(name, "r", encoding="utf-8", newline="") as f:
                    media.update(line.rstrip("\r\n") for line in f)
        selector = extract.Selector(
            topics={_topic_byte(t) for t in a.topic} if a.topic else None,
            outcomes=set(a.outcome) if a.outcome else None, media=media,
            statuses={_status_number(s) for s in a.status} if a.status else None,
            unknown_status=a.unknown_status, invert=a.invert)
    except (ValueError, OSError) as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 2
    if not _gpu_ready(a, "gpu_extract"):
        return 1
    source = a.input if a.input else sys.stdin.buffer
    out = sys.stdout.buffer if a.out == "-" else open(a.out, "wb")  # at once, not lazily: a failed run leaves its files
    indices = open(a.indices, "w", encoding="ascii") if a.indices else None
    try:
        counts = extract.extract_file(source, out, selector, device=a.device, dialect=a.dialect,
                                      chunk_bytes=a.chunk_bytes, indices_out=indices)
    except ValueError as e:  # broken framing: what was written so far is whole frames
        print(f"beholder: {e}", file=sys.stderr)
        return 1
    finally:
        if indices is not None:
            indices.close()
        if a.out == "-":
            out.flush()
        else:
            out.close()
    print(json.dumps(counts), file=sys.stderr)
    return 0


class _LazyOutput:
    """The output file of ``coalesce``, opened at the first write or at ``finish``: a run that fails
    before it has anything to write leaves no file behind."""

    def __init__(self, name: str, text: bool = False):
        self.name = name
        self.text = text
        self.file = None

    def write(self, data) -> int:
        if self.file is None:
            if self.text:
                self.file = open(self.name, "w", encoding="ascii")
            else:
                self.file = sys.stdout.buffer if self.name == "-" else open(self.name, "wb")
        return self.file.write(data)

    def finish(self) -> None:
        self.write("" if self.text else b"")
        if self.name == "-" and not self.text:
            self.file.flush()
        else:
            self.file.close()


def _close_outputs(outs, failed: Optional[Exception] = None) -> None:
    """The end of a run for its :class:`_LazyOutput` files (``None`` entries are passed over). After
    a run that went through, each is finished: one that nothing was written to becomes an empty file.
    After one that failed, only what it had opened is closed (stdout: flushed), holding what it wrote;
    the rest leaves no file."""
    for f in outs:
        if f is None:
            continue
        if failed is None:
            f.finish()
        elif f.file is not None:
            if f.name == "-" and not f.text:
                f.file.flush()
            else:
                f.file.close()


def _rewrite(outs, run, warn=None) -> int:
    """A stream-to-stream command from its outputs on: ``run()`` writes them and returns the counts,
    which go to stderr as one JSON line, after what ``warn(counts)`` has to say. A ``ValueError``
    (broken framing, a malformed row, a chunk too large for the device) is reported and gives 1; what
    was written before it is whole frames."""
    try:
        counts = run()
    except ValueError as e:
        _close_outputs(outs, e)
        print(f"beholder: {e}", file=sys.stderr)
        return 1
    _close_outputs(outs)
    if warn is not None:
        warn(counts)
    print(json.dumps(counts), file=sys.stderr)
    return 0


def _lazy_outputs(a: argparse.Namespace, indices: Optional[str]):
    """``(source, out, indices_out)`` of a stream-to-stream command whose ``-o`` is one file."""
    return (a.input if a.input else sys.stdin.buffer, _LazyOutput(a.out),
            _LazyOutput(indices, text=True) if indices else None)


def cmd_coalesce(a: argparse.Namespace) -> int:
    """Cut a framed stream down to the frames that set its end state (``beholder_amd.coalesce``)."""
    from . import coalesce
    policy = coalesce.Policy(status=a.status, progress=a.progress, undecoded=a.undecoded)  # argparse checked the values
    if not _gpu_ready(a, "gpu_coalesce"):
        return 1
    source, out, indices = _lazy_outputs(a, a.indices)
    return _rewrite((out, indices), lambda: coalesce.coalesce_file(  # fails before anything is written
        source, out, policy, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes, indices_out=indices))


def cmd_dedupe(a: argparse.Namespace) -> int:
    """Drop the byte-identical repeat frames of a framed stream (``beholder_amd.dedupe``)."""
    from . import dedupe
    try:
        policy = dedupe.Policy(keep=a.keep, topics={_topic_byte(t) for t in a.topic} if a.topic else None)
    except ValueError as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 2
    if not _gpu_ready(a, "gpu_dedupe"):
        return 1
    source, out, indices = _lazy_outputs(a, a.indices)
    return _rewrite((out, indices), lambda: dedupe.dedupe_file(  # last: fails before anything is written
        source, out, policy, device=a.device, chunk_bytes=a.chunk_bytes, indices_out=indices))


def cmd_compare(a: argparse.Namespace) -> int:
    """Match two framed streams frame for frame (``beholder_amd.compare``)."""
    from . import compare
    try:
        policy = compare.Policy(topics={_topic_byte(t) for t in a.topic} if a.topic else None)
    except ValueError as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 2
    if not _gpu_ready(a, "gpu_compare"):
        return 1
    outs = [_LazyOutput(name, text=text) if name else None
            for name, text in ((a.only_a, False), (a.only_b, False), (a.indices_a, True), (a.indices_b, True))]
    try:
        counts = compare.compare_file(a.a, a.b, outs[0], outs[1], policy, device=a.device,
                                      indices_a_out=outs[2], indices_b_out=outs[3])
    except (ValueError, OSError) as e:  # broken framing, captures beyond the device's limit: nothing was written
        print(f"beholder: {e}", file=sys.stderr)
        return 1
    _close_outputs(outs)
    print(json.dumps(counts))  # to stdout: the counts are this command's result
    return 3 if a.exit_code and not counts["equal"] else 0


def cmd_thin(a: argparse.Namespace) -> int:
    """Drop the progress events that repeat their media's step (``beholder_amd.thin``)."""
    from . import thin
    try:
        policy = thin.Policy(step=a.step, keep=a.keep)
    except ValueError as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 2
    if not _gpu_ready(a, "gpu_thin"):
        return 1
    source, out, indices = _lazy_outputs(a, a.indices)
    return _rewrite((out, indices), lambda: thin.thin_file(  # last: fails before anything is written
        source, out, policy, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes, indices_out=indices))


def cmd_normalise(a: argparse.Namespace) -> int:
    """Rewrite every decodable event of a framed stream in canonical form (``beholder_amd.normalise``)."""
    from . import normalise
    policy = normalise.Policy(undecoded=a.undecoded)  # argparse checked the value
    if not _gpu_ready(a, "gpu_normalise"):
        return 1
    source, out, indices = _lazy_outputs(a, a.indices)
    return _rewrite((out, indices), lambda: normalise.normalise_file(
        source, out, policy, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes, indices_out=indices))


def cmd_recover(a: argparse.Namespace) -> int:
    """Salvage the frames of a damaged framed stream (``beholder_amd.recover``)."""
    from . import recover
    try:
        policy = recover.Policy(max_frame=a.max_frame)
    except ValueError as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 2
    if not _gpu_ready(a, "gpu_recover"):
        return 1
    source, out, offsets = _lazy_outputs(a, a.offsets)
    gaps = _LazyOutput(a.gaps, text=True) if a.gaps else None
    intact = []
    status = _rewrite((out, offsets, gaps), lambda: recover.recover_file(
        source, out, policy, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes, gaps_out=gaps,
        offsets_out=offsets), warn=lambda counts: intact.append(counts["intact"]))
    return 3 if a.exit_code and intact == [False] else status


ANONYMISE_KEY_ENV = "BEHOLDER_ANONYMISE_KEY"


def _anonymise_key(a: argparse.Namespace) -> bytes:
    """The key from exactly one source; ``ValueError`` for none, several or a bad value. There is no
    option that takes the key itself: it would show in ``ps``."""
    env = os.environ.get(ANONYMISE_KEY_ENV)
    sources = [name for name, given in (("--key-file", a.key_file is not None), (f"${ANONYMISE_KEY_ENV}", bool(env)),
                                        ("--random-key", a.random_key)) if given]
    if len(sources) != 1:
        raise ValueError("the key comes from exactly one of --key-file, $%s and --random-key (%s)"
                         % (ANONYMISE_KEY_ENV, "given: " + ", ".join(sources) if sources else "none given"))
    if a.key_file is not None:
        try:
            with open(a.key_file, "rb") as f:
                key = f.read(65)  # as it is: no stripping
        except OSError as e:
            raise ValueError(f"--key-file: {e}") from None
    elif a.random_key:
        key = os.urandom(32)  # never shown, never stored
    else:
        try:
            key = bytes.fromhex(env)
        except ValueError:
            raise ValueError(f"${ANONYMISE_KEY_ENV} is hex") from None
    if not 16 <= len(key) <= 32:
        raise ValueError(f"the key from {sources[0]} has {len(key) if len(key) < 65 else 'more than 64'} bytes: "
                         "16 to 32 are needed")
    return key


def cmd_anonymise(a: argparse.Namespace) -> int:
    """Replace every mediaId and host of a framed stream by a keyed pseudonym (``beholder_amd.anonymise``)."""
    from . import anonymise
    try:
        if a.keep_media and a.keep_host:
            raise ValueError("--keep-media and --keep-host together leave nothing to replace")
        requests = []
        for request in a.pseudonym_of or []:
            field, eq, value = request.partition("=")
            if not eq or field not in anonymise.PERSON:
                raise ValueError(f"--pseudonym-of takes mediaId=VALUE or host=VALUE, not {request!r}")
            requests.append((field, value))
        fields = anonymise.FIELDS - ({"mediaId"} if a.keep_media else set()) - ({"host"} if a.keep_host else set())
        policy = anonymise.Policy(_anonymise_key(a), undecoded=a.undecoded, fields=frozenset(fields))
    except ValueError as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 2
    if requests:  # the key's owner translates a finding back; no capture is read
        for field, value in requests:
            print(f"{field}\t{value}\t{anonymise.pseudonym_of(policy.key, field, value)}")
        return 0
    if not _gpu_ready(a, "gpu_anonymise"):
        return 1

    def warn(counts: dict) -> None:
        if policy.undecoded == "keep" and counts["undecoded"]:
            print(f"beholder: warning: {counts['undecoded']} undecoded frames were kept byte for byte; they may hold "
                  "names in clear", file=sys.stderr)
    source, out, indices = _lazy_outputs(a, a.indices)
    return _rewrite((out, indices), lambda: anonymise.anonymise_file(
        source, out, policy, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes, indices_out=indices), warn)


def cmd_export(a: argparse.Namespace) -> int:
    """Write a framed stream as NDJSON rows, one per frame (``beholder_amd.export``)."""
    from . import export
    policy = export.Policy(undecoded=a.undecoded)  # argparse checked the value
    if not _gpu_ready(a, "gpu_export"):
        return 1
    source, out, indices = _lazy_outputs(a, a.indices)
    return _rewrite((out, indices), lambda: export.export_file(  # what a failed run wrote is whole rows
        source, out, policy, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes, indices_out=indices))


def cmd_import(a: argparse.Namespace) -> int:
    """Read NDJSON rows back into a framed stream (``beholder_amd.import_rows``)."""
    from . import import_rows
    policy = import_rows.Policy(malformed=a.malformed)  # argparse checked the value
    if not _gpu_ready(a, "gpu_import"):
        return 1
    source, out, lines = _lazy_outputs(a, a.lines)
    return _rewrite((out, lines), lambda: import_rows.import_file(
        source, out, policy, device=a.device, chunk_bytes=a.chunk_bytes, lines_out=lines))


def cmd_shard(a: argparse.Namespace) -> int:
    """Split a framed stream by media into N framed streams (``beholder_amd.shard``)."""
    from . import shard
    try:
        policy = shard.Policy(shards=a.shards, undecoded=a.undecoded)
        for pattern in (a.out, a.indices):
            if pattern is not None and "{}" not in pattern:
                raise ValueError(f"the pattern {pattern!r} needs a '{{}}' for the shard number")
    except ValueError as e:
        print(f"beholder: {e}", file=sys.stderr)
        return 2
    if not _gpu_ready(a, "gpu_shard"):
        return 1
    source = a.input if a.input else sys.stdin.buffer
    outs = [_LazyOutput(a.out.replace("{}", str(s))) for s in range(policy.shards)]
    indices = [_LazyOutput(a.indices.replace("{}", str(s)), text=True) for s in range(policy.shards)] \
        if a.indices else None
    # after a run that went through every shard gets a file, an empty one included
    return _rewrite(outs + (indices or []), lambda: shard.shard_file(
        source, outs, policy, device=a.device, dialect=a.dialect, chunk_bytes=a.chunk_bytes, indices_outs=indices))


def cmd_seed(a: argparse.Namespace) -> int:
    from .store import open_store

    async def main():
        st = open_store(a.store, a.dsn)
        await st.connect()
        try:
            await st.upsert_many(_load_fixture(a.fixture))
            print(await st.count())
        finally:
            await st.close()
    asyncio.run(main())
    return 0


def cmd_bench(a: argparse.Namespace) -> int:
    from .bench import harness
    return harness.main(a.rest)


def cmd_broker(a: argparse.Namespace) -> int:
    from .transport.amqp.broker import serve_forever
    try:
        asyncio.run(serve_forever(a.host, a.port))
    except KeyboardInterrupt:
        pass
    return 0


def cmd_publish(a: argparse.Namespace) -> int:
    from .transport.amqp import publish_frames
    data = open(a.input, "rb").read() if a.input else sys.stdin.buffer.read()
    n = asyncio.run(publish_frames(a.url, data))
    print(n)
    return 0


def _device_arg(p: argparse.ArgumentParser, kernels: str) -> None:
    p.add_argument("--device", choices=["cpu", "gpu"], default="cpu",
                   help=f"cpu: the definition, runs anywhere; gpu: the gfx950 {kernels} kernels")


def _capture_args(p: argparse.ArgumentParser, kernels: str, chunk_help: Optional[str], chunk_default: int = 256 << 20,
                  dialect: bool = True) -> None:
    """What the capture commands share, in the order their help lists it: the input, ``--device``
    (``kernels`` names its kernel family), ``--dialect`` and, where ``chunk_help`` is given,
    ``--chunk-bytes``. A command's own options that come before these are added before the call."""
    p.add_argument("input", nargs="?")
    _device_arg(p, kernels)
    if dialect:
        p.add_argument("--dialect", choices=["protobufjs", "upb"], default="protobufjs")
    if chunk_help:
        p.add_argument("--chunk-bytes", type=int, default=chunk_default, help=chunk_help)


def _indices_arg(p: argparse.ArgumentParser, help: str, metavar: str = "FILE") -> None:
    p.add_argument("--indices", metavar=metavar, help=help)


CUT_HELP = "cut the input in pieces of this size"
READ_HELP = "read the input in pieces of this size"
KEPT_INDICES_HELP = "write the kept frames' input indices here, one per line"
OUTPUT_INDICES_HELP = "write the output frames' input indices here, one per line"


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="beholder", description="Beholder telemetry events service")
    sub = ap.add_subparsers(dest="cmd", required=True)

    r = sub.add_parser("run", help="run the service")
    r.add_argument("--config", help="config file (default: search for 'events')")
    r.add_argument("--source", choices=["amqp", "stdin", "file"])
    r.add_argument("--path", help="input file for --source file")
    r.add_argument("--url", help="AMQP URL (default: dyn('rabbitmq'))")
    r.add_argument("--policy", choices=["block", "drop_newest"], help="ingest backpressure policy")
    r.add_argument("--format", choices=["binary", "ndjson"], help="stdin/file framing (default binary)")
    r.add_argument("--dead-letter", help="append never-acked frames to this file")
    r.add_argument("--log-level", choices=["trace", "debug", "info", "warn", "error", "fatal", "silent"])
    r.add_argument("--metrics-port", type=int, help="metrics port (-1 disables the exposer)")
    r.add_argument("--store", choices=["memory", "sqlite", "postgres"])
    r.add_argument("--dsn")
    r.add_argument("--ordering", choices=["none", "per_media"])
    r.add_argument("--media-fixture", help="JSON list of media rows to preload (implies --store memory)")
    r.add_argument("--stats", action="store_true", help="print final stats JSON to stderr")
    r.add_argument("--workers", type=int, default=0,
                   help="N competing-consumer processes on the same queues (amqp); one merged /metrics")
    r.set_defaults(fn=cmd_run)

    c = sub.add_parser("config", help="validate and print the effective config (secrets masked)")
    c.add_argument("--config")
    c.set_defaults(fn=cmd_config)

    g = sub.add_parser("gen", help="generate synthetic framed telemetry")
    g.add_argument("--events", type=int, default=100)
    g.add_argument("--media", type=int, default=1000)
    g.add_argument("--seed", type=int, default=0)
    g.add_argument("--rate", type=float, default=0.0, help="events/s (0 = as fast as possible)")
    g.add_argument("--progress-fraction", type=float, default=0.9)
    g.add_argument("--unknown-fraction", type=float, default=0.0)
    g.add_argument("--ndjson", action="store_true")
    g.add_argument("--media-out", help="write the media fixture JSON here")
    g.add_argument("--out", help="output file (default stdout)")
    g.set_defaults(fn=cmd_gen)

    d = sub.add_parser("decode", help="framed stream -> NDJSON")
    d.add_argument("input", nargs="?")
    d.set_defaults(fn=cmd_decode)

    z = sub.add_parser("summarise", help="framed stream -> what the service will have done with it (JSON)")
    _capture_args(z, "fold", chunk_help=None)  # --chunk-bytes comes after the command's own option
    z.add_argument("--media-fixture", help="JSON list of media rows: also print the prediction for them")
    z.add_argument("--chunk-bytes", type=int, default=256 << 20, help="fold the input in pieces of this size")
    z.set_defaults(fn=cmd_summarise)

    t = sub.add_parser("transitions", help="framed stream -> its per-media status moves (JSON)",
                       description="Count, over every media's status events in stream order, the moves between "
                                   "status classes: the transition matrix, changes, repeats, and the classes "
                                   "the media start and end on. Prints one JSON object.")
    _capture_args(t, "transitions", READ_HELP)
    t.add_argument("--per-media", action="store_true", help="also print one row per mediaId")
    t.set_defaults(fn=cmd_transitions)

    w = sub.add_parser("hosts", help="framed stream -> what every worker host did in it (JSON)",
                       description="Count, per worker host of the progress events, its events, media, stints, "
                                   "the media it took over and lost, its rewinds, and the media it held when the "
                                   "stream ended, by status. Prints one JSON object.")
    _capture_args(w, "hosts", READ_HELP)
    w.add_argument("--per-media", action="store_true", help="also print one row per mediaId")
    w.set_defaults(fn=cmd_hosts)

    g = sub.add_parser("stages", help="framed stream -> what stage each media is in and how far (JSON)",
                       description="Join the status and the progress events per media: the status events per "
                                   "class, the progress events by standing and reported status, the closed and the "
                                   "open stages by status and progress bucket, and the progress events that come "
                                   "before their media's first status event. Prints one JSON object.")
    _capture_args(g, "stages", READ_HELP)
    g.add_argument("--per-media", action="store_true", help="also print one row per mediaId")
    g.set_defaults(fn=cmd_stages)

    x = sub.add_parser("extract", help="framed stream -> the selected frames, a framed stream again",
                       description="Keep the frames that meet every given condition (none: all frames); "
                                   "the counts go to stderr as one JSON line.")
    x.add_argument("-o", "--out", required=True, help="output file ('-' for stdout)")
    x.add_argument("--topic", action="append", metavar="status|progress|N", help="topic byte; repeatable")
    x.add_argument("--outcome", action="append", choices=["decoded", "error", "other"],
                   help="decoded, error (the topic's codec raises) or other (neither topic); repeatable")
    x.add_argument("--media", action="append", metavar="ID", help="mediaId of a decoded frame; repeatable")
    x.add_argument("--media-file", action="append", metavar="FILE", help="mediaIds, one per line (an empty line is the empty id); repeatable")
    x.add_argument("--status", action="append", metavar="NAME|N",
                   help="status of a decoded frame, a TelemetryStatusEntry name or a number 0-63; repeatable")
    x.add_argument("--unknown-status", action="store_true",
                   help="a decoded frame whose status is no TelemetryStatusEntry number (quirk Q6)")
    x.add_argument("--invert", action="store_true", help="keep exactly the frames the rest rejects")
    _capture_args(x, "select", CUT_HELP)
    _indices_arg(x, KEPT_INDICES_HELP)
    x.set_defaults(fn=cmd_extract)

    u = sub.add_parser("dedupe", help="framed stream -> the same without byte-identical repeat frames",
                       description="Keep one frame of every distinct content (topic byte and body), by default "
                                   "the last, which is the one that is safe to replay; nothing is decoded. "
                                   "The counts go to stderr as one JSON line.")
    u.add_argument("-o", "--out", required=True, help="output file ('-' for stdout)")
    u.add_argument("--keep", choices=["last", "first"], default="last",
                   help="which occurrence of a content survives; 'first' can end a replay on a stale status")
    u.add_argument("--topic", action="append", metavar="status|progress|N",
                   help="only frames of this topic byte take part, the others are kept as they are; repeatable")
    _capture_args(u, "dedupe", CUT_HELP, dialect=False)  # nothing is decoded
    _indices_arg(u, KEPT_INDICES_HELP)
    u.set_defaults(fn=cmd_dedupe)

    h = sub.add_parser("thin", help="framed stream -> the same without the progress events that repeat their step",
                       description="Keep a media's progress history only where it moves: of neighbouring progress "
                                   "events of one mediaId with the same status and the same progress // STEP, one "
                                   "survives, by default the last. Every other frame is kept as it is. "
                                   "The counts go to stderr as one JSON line.")
    h.add_argument("-o", "--out", required=True, help="output file ('-' for stdout)")
    h.add_argument("--step", type=int, default=10, help="the width of a step in percentage points (1..2^31-1)")
    h.add_argument("--keep", choices=["last", "first"], default="last",
                   help="which event of a stretch of one step survives; 'last' keeps every stage's last event")
    _capture_args(h, "thin", CUT_HELP)
    _indices_arg(h, KEPT_INDICES_HELP)
    h.set_defaults(fn=cmd_thin)

    o = sub.add_parser("coalesce", help="framed stream -> the frames that set its end state, a framed stream again",
                       description="Keep, per key, the last frame only: by default the last status event and the "
                                   "last progress event of every mediaId, and every frame that is neither. "
                                   "The counts go to stderr as one JSON line.")
    o.add_argument("-o", "--out", required=True, help="output file ('-' for stdout)")
    o.add_argument("--status", choices=["last", "all"], default="last",
                   help="decoded status events: the last per mediaId, or all of them")
    o.add_argument("--progress", choices=["last", "per-status", "all", "none"], default="last",
                   help="decoded progress events: the last per mediaId, the last per mediaId and status number, "
                        "all (keeps beholder_progress_updates_total whole) or none")
    o.add_argument("--undecoded", choices=["keep", "drop"], default="keep",
                   help="frames that fail to decode or carry another topic byte")
    _capture_args(o, "coalesce", CUT_HELP)
    _indices_arg(o, KEPT_INDICES_HELP)
    o.set_defaults(fn=cmd_coalesce)

    z = sub.add_parser("normalise", help="framed stream -> the same with every event in its canonical encoding",
                       description="Decode every status and progress frame in the dialect it was captured under "
                                   "and write it as the service's own encoder would: fields in order, defaults "
                                   "omitted, unknown fields gone. Run it first, before dedupe. "
                                   "The counts go to stderr as one JSON line.")
    z.add_argument("-o", "--out", default="-", help="output file (default '-': stdout)")
    z.add_argument("--undecoded", choices=["keep", "drop"], default="keep",
                   help="frames that fail to decode or carry another topic byte: as they are, or nowhere")
    _capture_args(z, "normalise", CUT_HELP)
    _indices_arg(z, OUTPUT_INDICES_HELP)
    z.set_defaults(fn=cmd_normalise)

    y = sub.add_parser("anonymise", help="framed stream -> the same with every mediaId and host a keyed pseudonym",
                       description="Write every decoded status and progress event in its canonical encoding with "
                                   "mediaId and host replaced by keyed pseudonyms (BLAKE2s, 32 hex characters): "
                                   "the same key gives the same pseudonym in every run and capture, so the "
                                   "reports of the output are the input's up to renaming. The key comes from "
                                   "--key-file, $BEHOLDER_ANONYMISE_KEY (hex) or --random-key, exactly one. "
                                   "The counts go to stderr as one JSON line.")
    y.add_argument("-o", "--out", default="-", help="output file (default '-': stdout)")
    y.add_argument("--key-file", metavar="PATH", help="the key: this file's bytes as they are, 16 to 32")
    y.add_argument("--random-key", action="store_true",
                   help="a fresh key that is never shown or stored: consistent output, linkable to nothing else")
    y.add_argument("--undecoded", choices=["drop", "keep"], default="drop",
                   help="frames that fail to decode or carry another topic byte: nowhere, or as they are, with "
                        "whatever names they hold")
    y.add_argument("--keep-media", action="store_true", help="leave mediaId in clear")
    y.add_argument("--keep-host", action="store_true", help="leave host in clear")
    y.add_argument("--pseudonym-of", action="append", metavar="mediaId=VALUE|host=VALUE",
                   help="print field, value and pseudonym, tab-separated, and read no capture; repeatable")
    _capture_args(y, "anonymise", CUT_HELP)
    _indices_arg(y, OUTPUT_INDICES_HELP)
    y.set_defaults(fn=cmd_anonymise)

    x = sub.add_parser("export", help="framed stream -> NDJSON rows, one per frame, for jq, DuckDB, pandas and grep",
                       description="Decode every status and progress frame in the dialect it was captured under "
                                   "and write one JSON row per frame: its index in the input, its topic, and "
                                   "its fields with the status name, or the body as base64 where it does not "
                                   "decode. The rows are NDJSON input to the service again. "
                                   "The counts go to stderr as one JSON line.")
    x.add_argument("-o", "--out", default="-", help="output file (default '-': stdout)")
    x.add_argument("--undecoded", choices=["keep", "drop"], default="keep",
                   help="frames that fail to decode or carry another topic byte: a base64 row, or none")
    _capture_args(x, "export", CUT_HELP + " (the rows take several times the input's bytes)", chunk_default=64 << 20)
    _indices_arg(x, "write the rows' frame indices here, one per line")
    x.set_defaults(fn=cmd_export)

    im = sub.add_parser("import", help="NDJSON rows -> framed stream: the inverse of export",
                        description="Read one JSON row per line (topic with b64, or topic with json, as export "
                                    "writes them) and write one frame per row: the base64 body verbatim, or the "
                                    "fields in the canonical encoding. import of an export is the capture's "
                                    "normalise. Blank lines are passed over. "
                                    "The counts go to stderr as one JSON line.")
    im.add_argument("-o", "--out", default="-", help="output file (default '-': stdout)")
    im.add_argument("--malformed", choices=["fail", "skip"], default="fail",
                   help="a line that is no row: stop there with its line number and exit 1, or leave it out and count it")
    _capture_args(im, "import", "cut the input after the last newline within this size", dialect=False)
    im.add_argument("--lines", metavar="FILE", help="write the line numbers of the rows that became frames here, one per line")
    im.set_defaults(fn=cmd_import)

    h = sub.add_parser("shard", help="framed stream -> N framed streams, split by media, for parallel replay in order",
                       description="Every mediaId's events go to one shard, in their original order; the shard "
                                   "is a function of the decoded mediaId and N alone. "
                                   "The counts go to stderr as one JSON line.")
    h.add_argument("--shards", type=int, required=True, metavar="N", help="how many streams, 1-256")
    h.add_argument("-o", "--out", required=True, metavar="PATTERN",
                   help="output files; '{}' becomes the shard number ('dlq-{}.bin')")
    h.add_argument("--undecoded", choices=["first", "drop"], default="first",
                   help="frames that fail to decode or carry another topic byte: to shard 0, or nowhere")
    _capture_args(h, "shard", CUT_HELP)
    _indices_arg(h, "write each shard's input indices to these files, one per line; '{}' as in -o", metavar="PATTERN")
    h.set_defaults(fn=cmd_shard)

    v = sub.add_parser("recover", help="damaged framed stream -> its frames, with the spans that fit no frame cut out",
                       description="Walk the framing; where a header does not fit, skip to the next offset "
                                   "where a status or progress frame with a mediaId starts and is followed by "
                                   "another frame or the end, and go on from there. The frame just before a "
                                   "gap is the one to distrust. The counts go to stderr as one JSON line.")
    v.add_argument("-o", "--out", required=True, help="output file ('-': stdout)")
    v.add_argument("--gaps", metavar="FILE",
                   help="write one NDJSON row per gap here: offset, length, and after_frame, the output index of "
                        "the frame before it or -1")
    v.add_argument("--offsets", metavar="FILE", help="write the recovered frames' input offsets here, one per line")
    v.add_argument("--max-frame", type=int, default=1 << 20, metavar="N",
                   help="the longest frame length a header may hold, 1 to 16777216; --chunk-bytes is at least "
                        "four times this and 16")
    v.add_argument("--exit-code", action="store_true", help="exit with status 3 where the capture was not intact")
    _capture_args(v, "recover", READ_HELP)
    v.set_defaults(fn=cmd_recover)

    m = sub.add_parser("compare", help="two framed streams -> what is only in one, what is in both, in what order",
                       description="Match A and B as multisets of frames: the k-th occurrence of a content (topic "
                                   "byte and body) in A is paired with the k-th in B, every other frame is only "
                                   "in its capture. Nothing is decoded; run normalise on both first if two "
                                   "encodings of one event should count as equal. The counts go to stdout as "
                                   "one JSON object.")
    m.add_argument("a", metavar="A")
    m.add_argument("b", metavar="B")
    m.add_argument("--topic", action="append", metavar="status|progress|N",
                   help="only frames of this topic byte take part, the others are skipped; repeatable")
    m.add_argument("--only-a", metavar="PATH", help="write the frames only in A here, a framed stream")
    m.add_argument("--only-b", metavar="PATH", help="write the frames only in B here, a framed stream")
    m.add_argument("--indices-a", metavar="PATH", help="write the indices in A of the frames only in A, one per line")
    m.add_argument("--indices-b", metavar="PATH", help="write the indices in B of the frames only in B, one per line")
    _device_arg(m, "compare")
    m.add_argument("--exit-code", action="store_true", help="exit with status 3 where the captures differ")
    m.set_defaults(fn=cmd_compare)

    s = sub.add_parser("seed", help="load a media fixture into a store")
    s.add_argument("fixture")
    s.add_argument("--store", default="sqlite")
    s.add_argument("--dsn", required=True)
    s.set_defaults(fn=cmd_seed)

    b = sub.add_parser("bench", help="BASELINE.json measurement configs")
    b.add_argument("rest", nargs=argparse.REMAINDER)
    b.set_defaults(fn=cmd_bench)

    k = sub.add_parser("broker", help="run the built-in AMQP test broker (local development)")
    k.add_argument("--host", default="127.0.0.1")
    k.add_argument("--port", type=int, default=5672)
    k.set_defaults(fn=cmd_broker)

    p = sub.add_parser("publish", help="publish a framed stream to AMQP")
    p.add_argument("--url", required=True)
    p.add_argument("input", nargs="?")
    p.set_defaults(fn=cmd_publish)
    return ap


def strip_opt(argv: List[str], name: str) -> List[str]:
    out, skip = [], False
    for x in argv:
        if skip:
            skip = False
            continue
        if x == name:
            skip = True
            continue
        if x.startswith(name + "="):
            continue
        out.append(x)
    return out


def main(argv: Optional[List[str]] = None) -> int:
    a = build_parser().parse_args(argv)
    a.argv = argv
    return a.fn(a)
