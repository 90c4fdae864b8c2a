"""Selectors and ids shared by the tests of ``extract``: the definition (test_extract.py), the
predicate compiled for the host (test_hip_select_host.py) and the device path (test_gpu_extract.py).
They are written against ``telemetry_corpus.fold_corpus()``."""
from __future__ import annotations

from beholder_amd.bench.generator import Workload
from beholder_amd.extract import Selector
from beholder_amd.topics import PROGRESS_ID, STATUS_ID

FFFD = "�"
FFFD3 = FFFD * 3  # how protobufjs reads the fold corpus's id b"\xff\xfe\xfd"; the corpus has no lone U+FFFD id
M3, M7 = (Workload(n_media=64, seed=5).media[k].id for k in (3, 7))  # two media of the fold corpus

# one selector of every kind, and one with everything at once
KINDS = {
    "all": Selector(),
    "topics": Selector(topics={STATUS_ID, 3}),
    "outcome-error": Selector(outcomes={"error"}),
    "outcome-decoded-other": Selector(outcomes={"decoded", "other"}),
    "media": Selector(media={"", FFFD3, M3, "no-such-media"}),
    "statuses": Selector(statuses={0, 3, 63}),
    "unknown-status": Selector(unknown_status=True),
    "statuses-or-unknown": Selector(statuses={1}, unknown_status=True),
    "combined": Selector(topics={PROGRESS_ID}, outcomes={"decoded"}, media={M3, M7, "", "é"},
                         statuses={2, 4}, unknown_status=True),
    "combined-inverted": Selector(topics={PROGRESS_ID, STATUS_ID, 0}, outcomes={"decoded", "other"},
                                  media={M3, M7, FFFD3}, statuses={0, 1, 2, 3}, unknown_status=True, invert=True),
}


def collision_pairs() -> list:
    """60 pairs of ids of one length that differ only in the last byte: (x, y) byte strings."""
    return [(b"pair-%03d-x" % k, b"pair-%03d-y" % k) for k in range(60)]
