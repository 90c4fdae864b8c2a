"""Rows for the ``import`` tests (tests/test_import.py, tests/test_hip_import_host.py,
tests/test_gpu_import.py): hand-written NDJSON lines as bytes, valid and malformed, and the escape,
backslash-run and base64 cases at the edges of the emit's pieces of 64 text bytes."""
from __future__ import annotations

import base64
import functools
import json
from typing import List, Optional

from beholder_amd import export as ex
from beholder_amd.ops import frames
from beholder_amd.topics import PROGRESS, PROGRESS_ID, STATUS, STATUS_ID

import wire_edges
from telemetry_corpus import fold_corpus, varint

CORPORA = ("fold_corpus", "wire_edges")
SIZES = (1, 63, 64, 65, 127, 128, 129, 200)
B64_SIZES = (0, 1, 2, 3, 4, 62, 63, 64, 65)
INT32_EDGES = (0, 1, -1, 127, 128, 2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1, 5, 16384)


@functools.lru_cache(maxsize=None)
def corpus(name: str) -> bytes:
    return fold_corpus() if name == "fold_corpus" else wire_edges.stream(6000)


@functools.lru_cache(maxsize=None)
def exported(name: str, dialect: str, undecoded: str = "keep") -> ex.Exported:
    return ex.export_cpu(corpus(name), ex.Policy(undecoded), dialect)


def event_row(topic=PROGRESS, media: Optional[str] = None, status=None, progress=None, host: Optional[str] = None,
              i: Optional[int] = 0, name: Optional[str] = "null") -> bytes:
    """A row in export's shape. ``media`` and ``host`` are JSON string text as it stands between the
    quotes, escapes written out; ``topic`` is a queue name or a number; ``None`` leaves a key out."""
    fields = []
    if media is not None:
        fields.append(f'"mediaId":"{media}"')
    if status is not None:
        fields.append(f'"status":{status}')
    if progress is not None:
        fields.append(f'"progress":{progress}')
    if host is not None:
        fields.append(f'"host":"{host}"')
    members = [] if i is None else [f'"i":{i}']
    members.append(f'"topic":{json.dumps(topic)}')
    members.append('"json":{' + ",".join(fields) + "}")
    if name is not None:
        members.append(f'"name":{name}')
    return ("{" + ",".join(members) + "}").encode("ascii")


def b64_row(topic, body: bytes, i: Optional[int] = 0) -> bytes:
    head = "" if i is None else f'"i":{i},'
    return ("{" + head + f'"topic":{json.dumps(topic)},"b64":"{base64.b64encode(body).decode()}"' + "}").encode("ascii")


def valid_rows() -> List[bytes]:
    """Rows that ``frame_of_row`` accepts, one property each."""
    rows = [b64_row(t, b"\x00\xffbody") for t in (0, 9, 255, 1, 2, STATUS, PROGRESS)]
    rows += [event_row(1, "m", 3), event_row(2, "m", 3, 40, "h")]  # 1 and 2 as ints
    rows += [  # key order reversed, in the row and in the object
        b'{"name":"CONVERTING","json":{"host":"h","progress":40,"status":2,"mediaId":"m-1"},"topic":"v1.telemetry.progress","i":7}',
        b'{"b64":"AAEC","topic":9,"i":1}',
        b'{"json":{"status":4,"mediaId":"m"},"topic":"v1.telemetry.status"}',
        # whitespace between tokens
        b' \t{ "i" : 3 , "topic" :\t"v1.telemetry.progress" , "json" : { "mediaId" : "m" , "status" : 2 , "progress" : 7 , "host" : "h" } , "name" : null }\t ',
        b'{ "topic" : 9 , "b64" : "QUJD" }',
        b'{"topic":2,"json":{ }}',
        # i and name absent, and of odd types
        event_row(PROGRESS, "m", 1, 2, "h", i=None, name=None),
        event_row(PROGRESS, "m", 1, 2, "h", i=-5, name='"anything \\" at all"'),
        event_row(PROGRESS, "m", 1, 2, "h", i=12345678901234567890, name="7"),
        b'{"i":null,"topic":"v1.telemetry.status","json":{"mediaId":"m","status":1},"name":"DEPLOYED"}',
        b'{"i":[1,{"a":2.5}],"topic":"v1.telemetry.status","json":{"mediaId":"m","status":1},"name":{"x":true}}',
        b'{"i":1.5e3,"topic":"v1.telemetry.status","json":{"mediaId":"m","status":1},"name":false,"extra":[],"more":"x"}',
        # status by name, in mixed case
        b'{"topic":"v1.telemetry.progress","json":{"mediaId":"m1","status":"CONVERTING","progress":40}}',
        b'{"topic":"v1.telemetry.status","json":{"mediaId":"m1","status":"dePLoyed"}}',
        b'{"topic":"v1.telemetry.status","json":{"mediaId":"m1","status":"queued"}}',
        # absent fields, and all default
        event_row(PROGRESS, None, None, 5, None), event_row(PROGRESS, None, 2, None, None),
        event_row(PROGRESS, "", 0, 0, ""), event_row(STATUS, None, None, None, None), event_row(STATUS, "only"),
        event_row(PROGRESS, None, None, None, "host-only"),
        # escapes: every one JSON allows, A, a surrogate pair, raw U+2028
        event_row(PROGRESS, '\\"\\\\\\/\\b\\f\\n\\r\\t', 1, 2, '\\u0041\\u000a\\u007f\\u0000x'),
        event_row(STATUS, "\\ud83d\\ude00 pair", 2),
        event_row(PROGRESS, "\\u00e9\\u20ac", 2, 3, "\\u00E9"),
        '{"i":0,"topic":"v1.telemetry.progress","json":{"mediaId":"a b","status":1,"progress":2,"host":"h é"},"name":null}'.encode(),
        # b64 next to json: b64 wins, whatever json holds
        b'{"topic":"v1.telemetry.status","b64":"CgFt","json":{"mediaId":"other","status":3}}',
        b'{"topic":9,"json":{"mediaId":"other"},"b64":"CgFt"}',
        b'{"topic":9,"json":"not even an object","b64":""}',
        # base64 with non-zero trailing bits
        b'{"topic":9,"b64":"QR=="}', b'{"topic":9,"b64":"QUH="}',
        # a duplicate key: the last one wins, as json.loads has it
        b'{"topic":9,"topic":1,"json":{"status":1,"status":2}}',
    ]
    rows += [event_row(PROGRESS, "m", s, p, "h") for s in INT32_EDGES for p in (0, -1, 2 ** 31 - 1, -2 ** 31)]
    rows += [event_row(STATUS, "m", s) for s in INT32_EDGES]
    rows += [event_row(PROGRESS, "m", "-0", "-0", "h")]
    return rows


def malformed_rows() -> List[bytes]:
    """Lines that are no row, one reason each."""
    return [
        b'not json', b'{"topic":9,"b64":""', b'{"topic":9,"b64":""} trailing', b"{'topic':9,'b64':''}",
        b'[1,2]', b'"a string"', b'17', b'null',                                    # not an object
        b'{"topic":"v1.telemetry.other","b64":""}', b'{"topic":256,"b64":""}', b'{"topic":-1,"b64":""}',
        b'{"topic":true,"b64":""}', b'{"topic":1.0,"b64":""}', b'{"topic":null,"b64":""}', b'{"b64":""}',
        b'{"topic":9}', b'{"topic":"v1.telemetry.status","i":3,"name":null}',       # neither b64 nor json
        b'{"topic":9,"json":{"mediaId":"m"}}', b'{"topic":0,"json":{}}',             # json on another topic
        b'{"topic":"v1.telemetry.status","json":{"mediaId":"m","progress":1}}',
        b'{"topic":1,"json":{"host":"h"}}',
        b'{"topic":"v1.telemetry.progress","json":{"mediaId":"m","extra":1}}',
        b'{"topic":"v1.telemetry.progress","json":["mediaId"]}', b'{"topic":"v1.telemetry.progress","json":null}',
        b'{"topic":"v1.telemetry.progress","json":{"status":1.0}}', b'{"topic":"v1.telemetry.progress","json":{"progress":1.0}}',
        b'{"topic":"v1.telemetry.progress","json":{"status":2147483648}}',
        b'{"topic":"v1.telemetry.progress","json":{"progress":-2147483649}}',
        b'{"topic":"v1.telemetry.progress","json":{"status":true}}', b'{"topic":"v1.telemetry.progress","json":{"progress":false}}',
        b'{"topic":"v1.telemetry.progress","json":{"status":"FLYING"}}', b'{"topic":"v1.telemetry.progress","json":{"status":null}}',
        b'{"topic":"v1.telemetry.progress","json":{"progress":"40"}}',
        b'{"topic":"v1.telemetry.progress","json":{"mediaId":7}}', b'{"topic":"v1.telemetry.progress","json":{"host":null}}',
        b'{"topic":"v1.telemetry.progress","json":{"mediaId":"\\ud800"}}',           # a lone surrogate
        b'{"topic":"v1.telemetry.progress","json":{"host":"x\\udfffy"}}',
        b'{"topic":9,"b64":"QU JD"}', b'{"topic":9,"b64":"QUJ"}', b'{"topic":9,"b64":"QQ="}', b'{"topic":9,"b64":"Q==="}',
        b'{"topic":9,"b64":"=QUJ"}', b'{"topic":9,"b64":"QU-D"}', b'{"topic":9,"b64":17}', b'{"topic":9,"b64":null}',
        b'{"topic":9,"b64":"Q\xc3\xa9=="}',
        b'{"topic":9,"b64":"\xff\xfe"}', b'{"topic":"v1.telemetry.status","json":{"mediaId":"\xc3"}}', b'\x80',  # invalid UTF-8
        b'{"topic":"v1.telemetry.status","json":{"mediaId":"a\tb"}}',                # a raw control byte in a string
        b'{"topic":"v1.telemetry.status","json":{"mediaId":"\\x41"}}', b'{"topic":"v1.telemetry.status","json":{"mediaId":"\\u00"}}',
        b'{"topic":01,"b64":""}', b'{"topic":9,"b64":"",}', b'{,"topic":9,"b64":""}', b'{"topic":9 "b64":""}',
    ]


def relaxed_rows() -> List[bytes]:
    """ASCII rows in the grammar the device decides itself: none of them goes to the host."""
    blank = [" ", "\t", "  \t "]
    rows = []
    for k, ws in enumerate(blank):
        rows.append(f'{ws}{{{ws}"topic"{ws}:{ws}"v1.telemetry.progress"{ws},{ws}"json"{ws}:{ws}{{{ws}"host"{ws}:{ws}"h{k}"{ws},'
                    f'{ws}"progress"{ws}:{ws}-{k}{ws},{ws}"status"{ws}:{ws}{k}{ws},{ws}"mediaId"{ws}:{ws}"m\\n{k}"{ws}}}{ws},'
                    f'{ws}"i"{ws}:{ws}null{ws},{ws}"name"{ws}:{ws}"a \\"name\\""{ws}}}{ws}'.encode())
        rows.append(f'{{{ws}"b64"{ws}:{ws}"QUJDRA=="{ws},{ws}"topic"{ws}:{ws}{k + 7}{ws},{ws}"i"{ws}:{ws}-12{ws}}}'.encode())
    rows += [
        b'{"json":{},"topic":"v1.telemetry.status"}', b'{"json":{ },"topic":2}', b'{"topic":1,"json":{"status":-0}}',
        b'{"name":null,"i":"a string","topic":255,"b64":""}', b'{"i":99999999999999999999999,"topic":0,"b64":"/+/+"}',
        b'{"topic":"v1.telemetry.status","b64":"CgFt","json":{"mediaId":"other","status":3}}',
        b'{"topic":9,"json":{"mediaId":"other"},"b64":"CgFt"}', b'{"topic":9,"b64":"QR=="}',
        b'{"topic":"v1.telemetry.progress","json":{"mediaId":"\\u0041\\u006a\\u007F\\/","host":"\\b\\f\\r\\t\\\\"}}',
        event_row(PROGRESS, "m", 2 ** 31 - 1, -2 ** 31, "h"), event_row(1, "m", 3), event_row(2, "", 0, 0, ""),
    ]
    return rows


def _escape_strings() -> List[str]:
    """JSON string text, ASCII only: two- and six-byte escapes at text positions 62, 63, 64 and last;
    strings of every size in SIZES, all-escape and with single escapes; runs of one to five
    backslashes that end at text position 63 and at 64."""
    texts = []
    for n in SIZES:
        texts += ["\\n" * n, "\\u0001" * n, "\\\\" * n, "\\\"\\u007f\\/a" * (n // 4) + "z" * (n % 4)]
        for at in sorted({0, 62, 63, 64, n - 1} & set(range(n))):
            for esc in ('\\"', "\\u001f", "\\t", "\\u0041"):
                texts.append("a" * at + esc + "b" * (n - at - 1))
    for last in (63, 64):  # the run's last backslash is at this text position
        for run in (1, 2, 3, 4, 5):
            for tail in ("n", '"', "u0041", "\\"):
                closing = tail if run % 2 else ""   # an odd run's last backslash escapes what follows
                if tail == "\\" and run % 2:
                    continue                        # that would be a run one longer
                texts.append("a" * (last - run + 1) + "\\" * run + closing + "zz")
                texts.append("a" * (last - run + 1) + "\\" * run + closing)
    return list(dict.fromkeys(texts))


def escape_rows() -> List[bytes]:
    rows = []
    for text in _escape_strings():
        rows += [event_row(STATUS, text, 4), event_row(PROGRESS, "plain", 1, 2, text), event_row(PROGRESS, text, 1, 2, text),
                 event_row(PROGRESS, text, None, None, "plain")]
    return rows


def _str(field: int, value: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(value)) + value


def ascii_byte_rows(dialect: str) -> bytes:
    """Every ASCII byte as an id and as a host, through export: the rows' text."""
    events = [(PROGRESS_ID, _str(1, bytes([c]))) for c in range(0x80)]
    events += [(PROGRESS_ID, _str(1, b"m") + _str(4, bytes([c]))) for c in range(0x80)]
    events += [(STATUS_ID, _str(1, bytes([c]) * 3)) for c in range(0x80)]
    return ex.export_cpu(frames(events), ex.Policy(), dialect).data


def base64_rows() -> List[bytes]:
    rows = []
    for size in B64_SIZES:
        rows += [b64_row(9, bytes(range(size))), b64_row(0, b"\xff" * size), b64_row(255, b"\xfb\xef\xbe" * size),
                 b64_row(STATUS, b"\x2e" + b"\xc8" * size, i=None)]
    return rows


def frame_length_rows(length: int) -> List[bytes]:
    """Rows whose frame has exactly ``length`` bytes, as events and as base64 rows."""
    rows = [b64_row(9, b"\xfb" * (length - 5)), b64_row(PROGRESS, bytes(range(length - 5)))]
    assert length < 5 + 2 + 128  # the id's length varint is one byte
    rows.append(event_row(STATUS, "i" * (length - 7)))                    # 5 | 0a len id
    rows.append(event_row(PROGRESS, "i" * (length - 12), 1, None, "h"))   # 5 | 0a len id | 10 01 | 22 01 h
    rows.append(event_row(STATUS, "\\n" + "i" * (length - 8)))
    return rows


def edge_line(at: int) -> bytes:
    """A line of exactly ``at`` bytes, so that its newline is byte ``at`` of a text it begins: a base64
    row behind blanks, or blanks alone below the 20 bytes of the shortest row."""
    row = b64_row(9, b"\xfb" * (0 if at < 4000 else 3000), i=None)
    line = b" " * (at - len(row)) + row if at >= len(row) else b" " * at
    assert len(line) == at
    return line


def text_of(rows: List[bytes], newline: bytes = b"\n", final: bool = True) -> bytes:
    return newline.join(rows) + (newline if final and rows else b"")
