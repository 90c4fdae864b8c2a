"""``anonymise`` on the CPU (beholder_amd/anonymise.py): the pseudonym against ``hashlib`` and two pinned
values; the output against a rebuild from ``normalise``; the joins that survive, the names that do
not; keys, chunks, merge; the command line."""
from __future__ import annotations

import functools
import hashlib
import io
import json
import subprocess
import sys

import pytest

from beholder_amd import anonymise as an, hosts, ops, replay, stages, transitions
from beholder_amd.anonymise import Anonymised, Policy, anon_of, anonymise_cpu, anonymise_file, pseudonym_of
from beholder_amd.bench.generator import Workload
from beholder_amd.coalesce import DROP, KEEP
from beholder_amd.models import proto
from beholder_amd.normalise import Policy as NormalisePolicy, frame_of, normalise_cpu
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS_ID, STATUS_ID
from beholder_amd.transport.framing import iter_frames

import wire_edges  # noqa: E402
from telemetry_corpus import fold_corpus  # noqa: E402

KEY = bytes(range(32))
OTHER_KEY = bytes(range(1, 33))
CORPORA = {"fold_corpus": fold_corpus, "wire_edges": lambda: wire_edges.stream(6000),
           "workload": lambda: Workload(n_media=16, seed=3).framed(2000)}
TYPES = {STATUS_ID: proto.load("api.TelemetryStatus"), PROGRESS_ID: proto.load("api.TelemetryProgress")}
ONLY_MEDIA, ONLY_HOST = frozenset({"mediaId"}), frozenset({"host"})

both = pytest.mark.parametrize("dialect", ops.DIALECTS)
policies = pytest.mark.parametrize("undecoded", ["keep", "drop"])


@functools.lru_cache(maxsize=None)
def _stream(name: str) -> bytes:
    return CORPORA[name]()


@functools.lru_cache(maxsize=None)
def _anonymised(name: str, undecoded: str, dialect: str, fields: frozenset = an.FIELDS) -> Anonymised:
    return anonymise_cpu(_stream(name), Policy(KEY, undecoded, fields), dialect)


# ---- the pseudonym ---------------------------------------------------------------------------------------

def test_the_pinned_pseudonyms():
    """A compatibility surface: whoever holds this key finds these names in every capture."""
    assert pseudonym_of(KEY, "mediaId", "abc") == "b43e852137b0f85cd672ee1eeece559a"
    assert pseudonym_of(KEY, "host", "abc") == "1b6723a26a3859aff3dd67995e6eac73"
    assert an.PERSON == {"mediaId": b"bh.media", "host": b"bh.host"}


@pytest.mark.parametrize("text", ["a", "x" * 63, "x" * 64, "x" * 65, "y" * 128, "y" * 129, "média-é", "�m", "主机"])
def test_pseudonym_of_is_keyed_blake2s(text):
    for key in (KEY, KEY[:16], KEY[:17]):
        for field, person in an.PERSON.items():
            want = hashlib.blake2s(text.encode("utf-8"), key=key, digest_size=16, person=person).hexdigest()
            got = pseudonym_of(key, field, text)
            assert got == want and len(got) == 32 and got == got.lower()


def test_the_empty_string_and_the_arguments():
    assert pseudonym_of(KEY, "mediaId", "") == "" == pseudonym_of(KEY, "host", "")
    for n in (0, 15, 33):
        with pytest.raises(ValueError):
            pseudonym_of(bytes(n), "host", "h")
        with pytest.raises(ValueError):
            Policy(bytes(n))
    with pytest.raises(ValueError):
        pseudonym_of(KEY, "status", "h")
    with pytest.raises(TypeError):
        pseudonym_of("0" * 32, "host", "h")


def test_policy_validation():
    p = Policy(KEY)
    assert (p.undecoded, p.fields) == ("drop", frozenset({"mediaId", "host"}))
    assert p.key_id == hashlib.blake2s(KEY, digest_size=16, person=b"bh.keyid").hexdigest()[:8] and len(p.key_id) == 8
    assert Policy(OTHER_KEY).key_id != p.key_id
    assert KEY.hex() not in repr(p) and repr(KEY) not in repr(p)  # a policy in a log line gives no key away
    assert Policy(KEY, fields={"host"}).fields == ONLY_HOST
    with pytest.raises(ValueError):
        Policy(KEY, fields=frozenset())
    with pytest.raises(ValueError):
        Policy(KEY, fields={"status"})
    with pytest.raises(TypeError):
        Policy(KEY, fields="host")
    with pytest.raises(ValueError):
        Policy(KEY, "first")
    with pytest.raises(TypeError):
        Policy(KEY, 1)
    for call in (lambda: anon_of("keep"), lambda: anonymise_cpu(b"", NormalisePolicy()),
                 lambda: anonymise_file(io.BytesIO(b""), io.BytesIO(), "drop")):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        anonymise_cpu(b"", p, "proto2")
    with pytest.raises(ValueError):
        anonymise_file(io.BytesIO(b""), io.BytesIO(), p, dialect="proto2")
    empty = anonymise_cpu(b"", p, "upb")
    assert empty == Anonymised(b"", [], 0, 0, "upb", "drop", an.FIELDS, p.key_id)
    assert KEY not in repr(empty).encode() + empty.data and KEY.hex() not in repr(empty)


# ---- against a rebuild from normalise ------------------------------------------------------------------------

def _rebuild(data: bytes, policy: Policy, dialect: str) -> bytes:
    """Every frame of the normalised stream decoded, its strings mapped, and encoded again."""
    normalised = normalise_cpu(data, NormalisePolicy(policy.undecoded), dialect)
    parts = []
    for topic, body in iter_frames(normalised.data):
        codec = ops.codec_for(TYPES[topic], dialect) if topic in TYPES else None
        try:
            m = codec.decode(body) if codec else None
        except proto.DecodeError:
            m = None
        if m is not None:
            fields = {name: getattr(m, name) for name in ("mediaId", "status", "progress", "host") if hasattr(m, name)}
            for name in policy.fields & set(fields):
                fields[name] = pseudonym_of(policy.key, name, fields[name])
            body = bytes(codec.encode(fields))
        parts.append(frame_of(topic, body))
    return b"".join(parts)


@pytest.mark.parametrize("name", ["fold_corpus", "wire_edges"])
@both
@policies
def test_anonymise_is_normalise_with_the_strings_mapped(name, dialect, undecoded):
    data = _stream(name)
    got = _anonymised(name, undecoded, dialect)
    normalised = normalise_cpu(data, NormalisePolicy(undecoded), dialect)
    assert got.data == _rebuild(data, Policy(KEY, undecoded), dialect)
    assert (got.indices, got.frames, got.events) == (normalised.indices, normalised.frames, normalised.events)
    assert got.events > 400 and got.frames > 5000
    assert (got.dialect, got.undecoded, got.fields, got.key_id) == (dialect, undecoded, an.FIELDS, Policy(KEY).key_id)
    for fields in (ONLY_MEDIA, ONLY_HOST):
        want = _rebuild(data, Policy(KEY, undecoded, fields), dialect)
        assert _anonymised(name, undecoded, dialect, fields).data == want


@pytest.mark.parametrize("name", ["fold_corpus", "wire_edges"])
@both
@policies
def test_anonymise_after_normalise_is_anonymise(name, dialect, undecoded):
    normalised = normalise_cpu(_stream(name), NormalisePolicy(undecoded), dialect)
    again = anonymise_cpu(normalised.data, Policy(KEY, undecoded), dialect)
    assert again.data == _anonymised(name, undecoded, dialect).data


# ---- joins survive, names do not -----------------------------------------------------------------------------

def _reports(data: bytes, dialect: str) -> dict:
    return {"summarise": replay.fold_cpu(data, dialect).to_json(),
            "transitions": transitions.transitions_cpu(data, dialect).to_json(per_media=True),
            "hosts": hosts.hosts_cpu(data, dialect).to_json(per_media=True),
            "stages": stages.stages_cpu(data, dialect).to_json(per_media=True)}


def _renamed(node, key: bytes, under: str = ""):
    """A report with every name mapped: the keys of every ``media`` and ``hosts`` mapping, and the
    host in the ``[index, host, status, progress]`` rows of the hosts report. Mappings stay mappings,
    so the order of their rows does not count."""
    if isinstance(node, dict):
        field = {"media": "mediaId", "hosts": "host"}.get(under)
        out = {(pseudonym_of(key, field, k) if field else k): _renamed(v, key, k) for k, v in node.items()}
        assert len(out) == len(node)  # no two names share a pseudonym
        return out
    if under in ("first", "last") and isinstance(node, list) and len(node) == 4 and isinstance(node[1], str):
        return [node[0], pseudonym_of(key, "host", node[1])] + node[2:]
    return node


@pytest.mark.parametrize("name", ["workload", "fold_corpus"])
@both
def test_the_reports_are_the_same_up_to_renaming(name, dialect):
    clear = normalise_cpu(_stream(name), NormalisePolicy("drop"), dialect).data
    before, after = _reports(clear, dialect), _reports(_anonymised(name, "drop", dialect).data, dialect)
    assert len(before["summarise"]["media"]) >= 16 and len(before["hosts"]["hosts"]) >= 3
    for command in before:
        assert after[command] == _renamed(before[command], KEY), command
        assert after[command] != before[command], command
    assert set(after["hosts"]["hosts"]) == {pseudonym_of(KEY, "host", h) for h in before["hosts"]["hosts"]}


def _names(data: bytes) -> tuple:
    ids, hosts_ = set(), set()
    for topic, body in iter_frames(data):
        m = ops.codec_for(TYPES[topic], "protobufjs").decode(body)
        ids.add(m.mediaId.encode())
        if topic == PROGRESS_ID:
            hosts_.add(m.host.encode())
    return ids - {b""}, hosts_ - {b""}


def test_no_name_leaks():
    data = _stream("workload")
    ids, hosts_ = _names(data)
    assert len(ids) >= 16 and len(hosts_) >= 3
    assert all(len(i) == 36 for i in ids) and all(len(h) >= 8 for h in hosts_)  # long enough that no hit is chance
    out = _anonymised("workload", "drop", "protobufjs").data
    assert not [name for name in ids | hosts_ if name in out]
    kept = _anonymised("workload", "drop", "protobufjs", ONLY_MEDIA).data  # --keep-host
    assert not [name for name in ids if name in kept] and all(name in kept for name in hosts_)
    assert _names(kept)[1] == hosts_
    kept = _anonymised("workload", "drop", "protobufjs", ONLY_HOST).data  # --keep-media
    assert not [name for name in hosts_ if name in kept] and _names(kept)[0] == ids


def test_two_keys_share_no_pseudonym():
    data = _stream("workload")
    one, two = (_names(anonymise_cpu(data, Policy(key)).data) for key in (KEY, OTHER_KEY))
    assert len(one[0]) == len(two[0]) >= 16 and len(one[1]) == len(two[1]) >= 3
    assert not (one[0] | one[1]) & (two[0] | two[1])
    assert not one[0] & one[1]  # nor do a media and a host


def test_undecoded_frames_are_dropped_by_default_and_kept_as_they_are():
    events = [(STATUS_ID, b"\x0a\x01m\x10\x03"), (9, b"media-in-clear"), (PROGRESS_ID, b"\x2e"),
              (PROGRESS_ID, b"\x22\x01h\x18\x07\x10\x02\x0a\x01m\x38\x01"), (STATUS_ID, b"")]
    m, h = pseudonym_of(KEY, "mediaId", "m").encode(), pseudonym_of(KEY, "host", "h").encode()
    want = [b"\x0a\x20" + m + b"\x10\x03", KEEP, KEEP, b"\x0a\x20" + m + b"\x10\x02\x18\x07\x22\x20" + h, b""]
    for dialect in ops.DIALECTS:
        for undecoded in ("drop", "keep"):
            anon = anon_of(Policy(KEY, undecoded), dialect)
            got = [anon(topic, body) for topic, body in events]
            assert got == [DROP if w is KEEP and undecoded == "drop" else w for w in want]
        dropped = anonymise_cpu(frames(events), Policy(KEY), dialect)
        assert dropped.indices == [0, 3, 4] and dropped.frames == 5 and dropped.events == 3
        assert dropped.data == b"".join(frame_of(events[i][0], want[i]) for i in (0, 3, 4))
        kept = anonymise_cpu(frames(events), Policy(KEY, "keep"), dialect)
        assert kept.indices == list(range(5)) and b"media-in-clear" in kept.data and kept.events == 3
    assert anon_of(Policy(KEY, fields=ONLY_HOST))(*events[3]) == b"\x0a\x01m\x10\x02\x18\x07\x22\x20" + h
    assert anon_of(Policy(KEY, fields=ONLY_MEDIA))(*events[3]) == b"\x0a\x20" + m + b"\x10\x02\x18\x07\x22\x01h"


def test_two_spellings_of_one_string_get_one_pseudonym():
    """Under protobufjs the hash runs after U+FFFD substitution."""
    anon = anon_of(Policy(KEY), "protobufjs")
    want = b"\x0a\x20" + pseudonym_of(KEY, "mediaId", "�m").encode()
    assert anon(STATUS_ID, b"\x0a\x02\xffm") == anon(STATUS_ID, b"\x0a\x02\xfem") == want
    assert anon(STATUS_ID, b"\x0a\x04\xef\xbf\xbdm") == want
    assert anon_of(Policy(KEY), "upb")(STATUS_ID, b"\x0a\x02\xffm") is DROP


# ---- chunks and merge --------------------------------------------------------------------------------------

@both
def test_chunks_do_not_show(dialect):
    data = _stream("fold_corpus")
    assert len(data) > 7 * 30_000
    for undecoded in ("drop", "keep"):
        want = _anonymised("fold_corpus", undecoded, dialect)
        for chunk_bytes in (30_000, 1 << 30):
            out, indices = io.BytesIO(), io.StringIO()
            counts = anonymise_file(io.BytesIO(data), out, Policy(KEY, undecoded), "cpu", dialect, chunk_bytes, indices)
            assert out.getvalue() == want.data
            assert [int(line) for line in indices.getvalue().split()] == want.indices
            assert counts == {"frames": want.frames, "kept": len(want.indices), "kept_bytes": len(want.data),
                              "in_bytes": len(data), "events": want.events, "undecoded": want.frames - want.events,
                              "host_frames": 0}


def test_each_chunk_is_written_before_the_next_is_read():
    data = frames(list(iter_frames(_stream("workload")))[:80])

    class Source(io.BytesIO):
        def read(self, size=-1):
            reads.append(out.tell())
            return super().read(size)
    reads, out = [], io.BytesIO()
    anonymise_file(Source(data), out, Policy(KEY), chunk_bytes=256)
    assert len(reads) > 5 and reads[0] == 0 and reads == sorted(reads) and len(set(reads)) > 5
    assert out.getvalue() == anonymise_cpu(data, Policy(KEY)).data


@both
def test_merge_is_concatenation_and_refuses_another_setting(dialect):
    events = list(iter_frames(_stream("workload")))[:60] + [(9, b"other"), (PROGRESS_ID, b"\x2e")]
    for undecoded in ("drop", "keep"):
        policy = Policy(KEY, undecoded)
        whole = anonymise_cpu(frames(events), policy, dialect)
        for cut in (0, 1, 31, 61, len(events)):
            a, b = (anonymise_cpu(frames(part), policy, dialect) for part in (events[:cut], events[cut:]))
            before = (a.data, list(a.indices), b.data, list(b.indices))
            assert a.merge(b) == whole
            assert (a.data, a.indices, b.data, b.indices) == before
        other = "upb" if dialect == "protobufjs" else "protobufjs"
        for policy2, dialect2 in ((Policy(OTHER_KEY, undecoded), dialect), (Policy(KEY, undecoded, ONLY_HOST), dialect),
                                  (policy, other), (Policy(KEY, "keep" if undecoded == "drop" else "drop"), dialect)):
            with pytest.raises(ValueError):
                whole.merge(anonymise_cpu(b"", policy2, dialect2))


# ---- the command line ----------------------------------------------------------------------------------------

def _cli(*args, stdin=None, env=None):
    import os
    environ = {k: v for k, v in os.environ.items() if k != "BEHOLDER_ANONYMISE_KEY"}
    environ.update(env or {})
    return subprocess.run([sys.executable, "-m", "beholder_amd", "anonymise", *args], input=stdin, capture_output=True,
                          timeout=120, env=environ)


def _counts(r) -> dict:
    return json.loads(r.stderr.decode().strip().splitlines()[-1])


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    path = tmp_path_factory.mktemp("anonymise") / "capture.bin"
    events = list(iter_frames(_stream("workload")))[:200] + [(9, b"other"), (PROGRESS_ID, b"\x2e")]
    path.write_bytes(frames(events))
    return path


def test_the_command_line_takes_the_key_from_a_file_or_the_environment(capture, tmp_path):
    data = capture.read_bytes()
    keyfile, out, indices = tmp_path / "key", tmp_path / "out.bin", tmp_path / "indices.txt"
    keyfile.write_bytes(KEY)
    for dialect in ops.DIALECTS:
        want = anonymise_cpu(data, Policy(KEY), dialect)
        r = _cli(str(capture), "-o", str(out), "--indices", str(indices), "--key-file", str(keyfile),
                 "--dialect", dialect, "--chunk-bytes", "500")
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == want.data and r.stdout == b""
        assert [int(line) for line in indices.read_text().split()] == want.indices
        assert _counts(r) == {"frames": 202, "kept": 200, "kept_bytes": len(want.data), "in_bytes": len(data),
                              "events": 200, "undecoded": 2, "host_frames": 0}
        assert b"warning" not in r.stderr
    r = _cli(env={"BEHOLDER_ANONYMISE_KEY": KEY.hex()}, stdin=data)  # stdin to stdout, the defaults
    assert r.returncode == 0 and r.stdout == anonymise_cpu(data, Policy(KEY)).data
    whitespace = tmp_path / "key-with-newline"
    whitespace.write_bytes(KEY[:16] + b"\n")  # the file's bytes as they are: the newline is key material
    r = _cli("--key-file", str(whitespace), stdin=data)
    assert r.returncode == 0 and r.stdout == anonymise_cpu(data, Policy(KEY[:16] + b"\n")).data
    r = _cli("--key-file", str(keyfile), "--keep-host", stdin=data)
    assert r.returncode == 0 and r.stdout == anonymise_cpu(data, Policy(KEY, fields=ONLY_MEDIA)).data
    r = _cli("--key-file", str(keyfile), "--keep-media", stdin=data)
    assert r.returncode == 0 and r.stdout == anonymise_cpu(data, Policy(KEY, fields=ONLY_HOST)).data
    r = _cli("--key-file", str(keyfile), "-o", str(out), stdin=data[:-2])  # whole frames only, and exit code 1
    assert r.returncode == 1 and b"truncated" in r.stderr


def test_the_command_line_wants_exactly_one_good_key(capture, tmp_path):
    data = capture.read_bytes()
    keyfile, short, long = tmp_path / "key", tmp_path / "short", tmp_path / "long"
    keyfile.write_bytes(KEY)
    short.write_bytes(KEY[:15])
    long.write_bytes(KEY + b"!")
    hexkey = {"BEHOLDER_ANONYMISE_KEY": KEY.hex()}
    for args, env in (((), None), (("--key-file", str(keyfile), "--random-key"), None), (("--random-key",), hexkey),
                      (("--key-file", str(keyfile)), hexkey), (("--key-file", str(short)), None),
                      (("--key-file", str(long)), None), (("--key-file", str(tmp_path / "none")), None),
                      ((), {"BEHOLDER_ANONYMISE_KEY": "zz" * 16}), ((), {"BEHOLDER_ANONYMISE_KEY": "00" * 15}),
                      (("--key", KEY.hex()), None), (("--key-file", str(keyfile), "--keep-media", "--keep-host"), None),
                      (("--key-file", str(keyfile), "--undecoded", "first"), None),
                      (("--key-file", str(keyfile), "--pseudonym-of", "status=3"), None),
                      (("--key-file", str(keyfile), "--pseudonym-of", "mediaId"), None)):
        r = _cli(*args, env=env, stdin=data)
        assert r.returncode == 2 and r.stdout == b"", (args, env, r.stderr)
        assert KEY.hex().encode() not in r.stderr or "--key" in args


def test_two_random_keys_differ_and_each_is_consistent(capture):
    data = capture.read_bytes()
    one, two = (_cli("--random-key", stdin=data) for _ in range(2))
    assert one.returncode == two.returncode == 0 and one.stdout != two.stdout
    clear = normalise_cpu(data, NormalisePolicy("drop")).data
    want = transitions.transitions_cpu(clear).to_json()
    for r in (one, two):
        assert _counts(r) == {"frames": 202, "kept": 200, "kept_bytes": len(r.stdout), "in_bytes": len(data),
                              "events": 200, "undecoded": 2, "host_frames": 0}
        assert len(list(iter_frames(r.stdout))) == 200
        assert transitions.transitions_cpu(r.stdout).to_json() == want  # the totals, media not named
        ids, hosts_ = _names(r.stdout)
        assert (len(ids), len(hosts_)) == tuple(map(len, _names(clear)))
    assert not _names(one.stdout)[0] & _names(two.stdout)[0]


def test_pseudonym_of_on_the_command_line(tmp_path):
    keyfile = tmp_path / "key"
    keyfile.write_bytes(KEY)
    r = _cli("--key-file", str(keyfile), "--pseudonym-of", "mediaId=abc", "--pseudonym-of", "host=abc",
             "--pseudonym-of", "host=a=b", "--pseudonym-of", "host=", str(tmp_path / "no-such-capture"))
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout.decode().splitlines() == ["mediaId\tabc\tb43e852137b0f85cd672ee1eeece559a",
                                              "host\tabc\t1b6723a26a3859aff3dd67995e6eac73",
                                              "host\ta=b\t" + pseudonym_of(KEY, "host", "a=b"), "host\t\t"]
    r = _cli("--pseudonym-of", "host=abc", env={"BEHOLDER_ANONYMISE_KEY": KEY.hex()})
    assert r.stdout == b"host\tabc\t1b6723a26a3859aff3dd67995e6eac73\n"


def test_keeping_undecoded_frames_warns(capture, tmp_path):
    data = capture.read_bytes()
    keyfile = tmp_path / "key"
    keyfile.write_bytes(KEY)
    r = _cli("--key-file", str(keyfile), "--undecoded", "keep", stdin=data)
    assert r.returncode == 0 and r.stdout == anonymise_cpu(data, Policy(KEY, "keep")).data and b"other" in r.stdout
    warnings = [line for line in r.stderr.decode().splitlines() if "warning" in line]
    assert len(warnings) == 1 and " 2 undecoded frames" in warnings[0]
    assert _counts(r)["kept"] == 202
    decoded = frames(list(iter_frames(data))[:200])
    r = _cli("--key-file", str(keyfile), "--undecoded", "keep", stdin=decoded)
    assert r.returncode == 0 and b"warning" not in r.stderr  # nothing was kept undecoded


def test_cli_gpu_without_a_device_names_the_cpu_path(capture, tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip("torch")  # the gpu path's plumbing; the service never imports it
    from beholder_amd import cli
    from beholder_amd.ops import hip_lib
    monkeypatch.setenv("BEHOLDER_ANONYMISE_KEY", KEY.hex())
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["anonymise", str(capture), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device gpu is not available" in out.err and "--device cpu" in out.err and not out.out
    # and with a device but no library
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "libbeholder_hip.so"))
    monkeypatch.setattr(hip_lib, "_lib", None)
    assert cli.main(["anonymise", str(capture), "--device", "gpu"]) == 1
    out = capsys.readouterr()
    assert "--device cpu" in out.err and "missing" in out.err and not out.out
