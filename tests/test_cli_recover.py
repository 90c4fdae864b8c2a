"""``python -m beholder_amd recover`` (beholder_amd/cli.py cmd_recover): the round trip of a torn file,
what ``--gaps`` and ``--offsets`` hold, the exit status, and a recovered file through ``summarise``."""
from __future__ import annotations

import json
import subprocess
import sys

from beholder_amd import cli
from beholder_amd.recover import Policy, recover_cpu

import recover_cases as cases  # noqa: E402


def _cli(*args, stdin: bytes = b""):
    return subprocess.run([sys.executable, "-m", "beholder_amd", *args], input=stdin, capture_output=True, timeout=120)


def test_round_trip_of_a_torn_file(tmp_path):
    whole = cases.corpus("fold_corpus")
    torn = whole[:-3]
    want = recover_cpu(torn, Policy())
    (tmp_path / "torn.bin").write_bytes(torn)
    out, gaps, offsets = (str(tmp_path / name) for name in ("out.bin", "gaps.ndjson", "offsets.txt"))
    r = _cli("summarise", str(tmp_path / "torn.bin"))
    assert r.returncode == 1 and b"truncated" in r.stderr  # what every other command says
    r = _cli("recover", str(tmp_path / "torn.bin"), "-o", out, "--gaps", gaps, "--offsets", offsets)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    counts = json.loads(r.stderr)
    assert counts == {"in_bytes": len(torn), "kept_bytes": len(want.data), "frames": want.frames, "anchors": 0,
                      "gaps": 1, "gap_bytes": want.gaps[0][1], "largest_gap": want.gaps[0][1], "intact": False,
                      "host_offsets": 0}
    assert (tmp_path / "out.bin").read_bytes() == want.data and whole.startswith(want.data)
    rows = [json.loads(line) for line in (tmp_path / "gaps.ndjson").read_text().splitlines()]
    assert rows == [{"offset": want.gaps[0][0], "length": want.gaps[0][1], "after_frame": want.frames - 1}]
    assert [int(line) for line in (tmp_path / "offsets.txt").read_text().split()] == want.offsets
    # the recovered file goes through the commands again, and says what the intact head says
    r = _cli("summarise", out)
    assert r.returncode == 0, r.stderr
    (tmp_path / "head.bin").write_bytes(want.data)
    assert json.loads(r.stdout) == json.loads(_cli("summarise", str(tmp_path / "head.bin")).stdout)
    r = _cli("recover", out, "-o", str(tmp_path / "again.bin"), "--exit-code")  # the identity, and intact
    assert r.returncode == 0 and json.loads(r.stderr)["intact"] and (tmp_path / "again.bin").read_bytes() == want.data


def test_exit_code_gaps_in_the_middle_and_stdin(tmp_path):
    data = cases.damage_cases()["two_gaps_one_frame_between"]
    want = recover_cpu(data, Policy(64))
    gaps = str(tmp_path / "gaps.ndjson")
    r = _cli("recover", "-o", "-", "--max-frame", "64", "--chunk-bytes", "272", "--gaps", gaps, "--exit-code", stdin=data)
    assert r.returncode == 3 and r.stdout == want.data, r.stderr
    assert json.loads(r.stderr)["gaps"] == 2 and json.loads(r.stderr)["anchors"] == 2
    rows = [json.loads(line) for line in open(gaps).read().splitlines()]
    assert [(row["offset"], row["length"]) for row in rows] == want.gaps and [row["after_frame"] for row in rows] == [0, 2]
    r = _cli("recover", "-o", "-", "--max-frame", "64", stdin=data)  # without --exit-code a damaged capture is 0
    assert r.returncode == 0 and r.stdout == want.data
    r = _cli("recover", "-o", "-", "--dialect", "upb", "--exit-code", stdin=cases.corpus("wire_edges"))
    assert r.returncode == 0 and r.stdout == cases.corpus("wire_edges")
    garbage = _cli("recover", "-o", str(tmp_path / "none.bin"), "--gaps", gaps, "--exit-code", stdin=cases.JUNK)
    assert garbage.returncode == 3 and (tmp_path / "none.bin").read_bytes() == b""
    assert json.loads(open(gaps).read()) == {"offset": 0, "length": 7, "after_frame": -1}


def test_usage_errors(tmp_path):
    r = _cli("recover", "-o", str(tmp_path / "x"), "--max-frame", "0", stdin=b"")
    assert r.returncode == 2 and b"max_frame" in r.stderr
    r = _cli("recover", "-o", str(tmp_path / "y"), "--max-frame", "1024", "--chunk-bytes", "4000", stdin=b"")
    assert r.returncode == 1 and b"--chunk-bytes" in r.stderr and b"--max-frame" in r.stderr
    assert not (tmp_path / "y").exists()  # nothing was written
    assert _cli("recover").returncode == 2  # -o is required
    assert "recover " in cli.__doc__
