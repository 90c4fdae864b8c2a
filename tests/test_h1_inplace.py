"""H1Parser's in-place path: a whole reply fed in one chunk into an empty parser is parsed where
it lies (``inplace`` counts those). The buffered path is the specification: every input here is
also fed with its first byte alone, which always buffers, and both must end the same way."""
import pytest

from beholder_amd.ops import H1Parser
from beholder_amd.sinks.http import HttpResponse

STUB = b"HTTP/1.1 200 OK\r\nContent-Type: application/json; charset=utf-8\r\nContent-Length: 2\r\n\r\n{}"
STUB_HEADERS = b"Content-Type: application/json; charset=utf-8\r\nContent-Length: 2\r\n"

BASES = [
    STUB,
    b"HTTP/1.1 204 No Content\r\nX-A: b\r\n\r\n",
    b"HTTP/1.0 200 OK\r\nContent-Length: 3\r\n\r\nabc",
    b"HTTP/1.1 200 OK\r\nConnection: close\r\nContent-Length: 1\r\n\r\nx",
    b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n2\r\n{}\r\n0\r\n\r\n",
    b"HTTP/1.1 100 Continue\r\n\r\nHTTP/1.1 200 OK\r\nContent-Length: 0\r\n\r\n",
    b"HTTP/1.1 200\r\nContent-Length: 0\r\n\r\n",
    b"HTTP/1.1 200 OK\nContent-Length: 2\n\n{}",
    b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\nContent-Length: 2\r\n\r\n{}",
    b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n\r\n{}EXTRA",
]
SUBS = [b"\r", b"\n", b" ", b":", b"\x80", b"0", b"\t", b"A"]


def outcome(chunks, head):
    """How a fresh parser ends after `chunks`: the result (feed's, else eof's) or the error
    text, with `buffered` and `responses`."""
    p = H1Parser()
    p.start(head=head)
    try:
        r = None
        for c in chunks:
            r = p.feed(c)
        if r is None:
            r = p.eof()
    except ValueError as e:
        r = ("ValueError", str(e))
    return r, p.buffered, p.responses


def variants(base):
    yield base
    for i in range(len(base)):
        for s in SUBS:
            yield base[:i] + s + base[i + 1:]
    for i in range(len(base)):
        yield base[:i]


def test_case_count():
    assert sum(1 for b in BASES for _ in variants(b)) * 2 == 9362


@pytest.mark.parametrize("base", BASES, ids=range(len(BASES)))
def test_one_chunk_equals_buffered(base):
    bad = []
    for c in variants(base):
        for head in (False, True):
            whole = outcome([c], head)
            split = outcome([c[:1], c[1:]], head)
            if whole != split:
                bad.append((c, head, whole, split))
    assert not bad, (len(bad), bad[:3])


def fed(p, data, head=False):
    p.start(head=head)
    return p.feed(data)


def test_stub_reply_is_parsed_in_place():
    p = H1Parser()
    assert p.inplace == 0
    assert fed(p, STUB) == (200, "OK", STUB_HEADERS, b"{}", True)
    assert p.inplace == 1 and p.responses == 1 and p.buffered == 0 and p.idle


def test_repeated_reply_reuses_its_objects():
    p = H1Parser()
    a = fed(p, STUB)
    b = fed(p, bytes(bytearray(STUB)))  # other memory, equal bytes
    assert p.inplace == 2
    assert b[1] is a[1] and b[2] is a[2] and b[3] is a[3]
    c = fed(p, STUB.replace(b"{}", b"[]"))
    assert p.inplace == 3
    assert c[1] is a[1] and c[2] is a[2]
    assert c[3] == b"[]" and c[3] is not a[3]
    # the buffered path shares the same cache
    p.start()
    assert p.feed(STUB[:20]) is None
    d = p.feed(STUB[20:].replace(b"{}", b"[]"))
    assert p.inplace == 3
    assert d[1] is a[1] and d[2] is a[2] and d[3] is c[3]


def test_split_reply_is_buffered():
    p = H1Parser()
    p.start()
    assert p.feed(STUB[:40]) is None
    assert p.feed(STUB[40:]) == (200, "OK", STUB_HEADERS, b"{}", True)
    assert p.inplace == 0 and p.responses == 1


def test_trailing_bytes_are_buffered():
    p = H1Parser()
    extra = b"HTTP/1.1 2"
    assert fed(p, STUB + extra) == (200, "OK", STUB_HEADERS, b"{}", True)
    assert p.inplace == 0 and p.buffered == len(extra)


def test_interim_reply_then_whole_reply():
    p = H1Parser()
    p.start()
    assert p.feed(b"HTTP/1.1 100 Continue\r\n\r\n") is None
    assert p.inplace == 0 and p.buffered == 0
    assert p.feed(STUB) == (200, "OK", STUB_HEADERS, b"{}", True)
    assert p.inplace == 1 and p.responses == 1


@pytest.mark.parametrize("reply, head, want", [
    (b"HTTP/1.0 200 OK\r\nContent-Length: 3\r\n\r\nabc", False, (200, "OK", b"Content-Length: 3\r\n", b"abc", False)),
    (b"HTTP/1.0 200 OK\r\nConnection: Keep-Alive\r\nContent-Length: 0\r\n\r\n", False,
     (200, "OK", b"Connection: Keep-Alive\r\nContent-Length: 0\r\n", b"", True)),
    (b"HTTP/1.1 200 OK\r\nConnection: foo, Close\r\nContent-Length: 1\r\n\r\nx", False,
     (200, "OK", b"Connection: foo, Close\r\nContent-Length: 1\r\n", b"x", False)),
    (b"HTTP/1.1 204 No Content\r\nContent-Length: 5\r\n\r\n", False, (204, "No Content", b"Content-Length: 5\r\n", b"", True)),
    (b"HTTP/1.1 304 Not Modified\r\n\r\n", False, (304, "Not Modified", b"", b"", True)),
    (b"HTTP/1.1 200 OK\r\nContent-Length: 7\r\n\r\n", True, (200, "OK", b"Content-Length: 7\r\n", b"", True)),
    (b"HTTP/1.1 200\r\nContent-Length: 0\r\n\r\n", False, (200, "", b"Content-Length: 0\r\n", b"", True)),
    (b"HTTP/1.1 200 \r\ncontent-length:  2 \r\n\r\nhi", False, (200, "", b"content-length:  2 \r\n", b"hi", True)),
    (b"HTTP/1.1 404 Not Found\r\nContent-Length: 0\r\n\r\n", False, (404, "Not Found", b"Content-Length: 0\r\n", b"", True)),
])
def test_framings_handled_in_place(reply, head, want):
    p = H1Parser()
    assert fed(p, reply, head) == want
    assert p.inplace == 1
    assert outcome([reply[:1], reply[1:]], head) == (want, 0, 1)


@pytest.mark.parametrize("reply", [
    b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n0\r\n\r\n",
    b"HTTP/1.1 200 OK\r\nContent-Length: 1\r\nContent-Length: 1\r\n\r\nx",
    b"HTTP/1.1 200 OK\r\n\r\nrest",  # close-delimited
    b"HTTP/1.1 200 OK\nContent-Length: 1\n\nx",
    b"HTTP/1.1 200 OK\r\nA: b\r\n c\r\nContent-Length: 1\r\n\r\nx",
    b"HTTP/1.1 200 OK\r\nContent-Length: 3\r\n\r\nx",  # short
    b"HTTP/2.0 200 OK\r\nContent-Length: 0\r\n\r\n",
    b"HTTP/1.1 200 OK\r\nBad Name: x\r\nContent-Length: 0\r\n\r\n",
])
def test_other_framings_stay_on_the_buffered_path(reply):
    p = H1Parser()
    p.start()
    try:
        p.feed(reply)
    except ValueError:
        pass
    assert p.inplace == 0


def test_limits_are_the_buffered_path_s():
    big = b"HTTP/1.1 200 OK\r\nContent-Length: 9\r\n\r\n123456789"
    p = H1Parser(max_body=8)
    p.start()
    with pytest.raises(ValueError, match="exceeds max_body"):
        p.feed(big)
    assert p.inplace == 0
    long_head = b"HTTP/1.1 200 OK\r\nX: " + b"a" * 80 + b"\r\nContent-Length: 0\r\n\r\n"
    for chunks in ([long_head], [long_head[:1], long_head[1:]]):
        p = H1Parser(max_header=64)
        p.start()
        with pytest.raises(ValueError, match="header block too large"):
            for c in chunks:
                p.feed(c)
        assert p.inplace == 0


def test_latin1_reason_decodes_as_before():
    reply = b"HTTP/1.1 200 \xe9t\xe9\r\nContent-Length: 0\r\n\r\n"
    p = H1Parser()
    r = fed(p, reply)
    assert p.inplace == 1
    assert r[1] == "\xe9t\xe9"
    assert outcome([reply[:1], reply[1:]], False)[0] == r
    utf8 = "HTTP/1.1 200 été\r\nContent-Length: 0\r\n\r\n".encode()
    assert fed(p, utf8)[1] == "été"
    assert fed(p, reply)[1] == "\xe9t\xe9"  # non-ASCII reasons are not cached


def test_memory_of_the_chunk_is_not_kept():
    p = H1Parser()
    buf = bytearray(STUB)
    r = fed(p, buf)
    buf[:] = b"\x00" * len(buf)
    assert r == (200, "OK", STUB_HEADERS, b"{}", True)
    assert fed(p, STUB) == r


def test_response_fields_equal_whole_and_split():
    def response(chunks):
        p = H1Parser()
        p.start()
        r = None
        for c in chunks:
            r = p.feed(c)
        status, _reason, raw, body, _keep = r
        return p.inplace, HttpResponse(status, body, None, "http://sink/x", raw)
    n1, a = response([STUB])
    n2, b = response([STUB[:1], STUB[1:]])
    assert (n1, n2) == (1, 0)
    for f in ("status", "body", "headers", "url", "ok"):
        assert getattr(a, f) == getattr(b, f), f
    assert a.headers == {"content-type": "application/json; charset=utf-8", "content-length": "2"}
    assert a.json() == {} and b.json() == {}
