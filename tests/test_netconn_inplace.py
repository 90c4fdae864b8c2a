"""A reply that reaches the NetConn in one recv is parsed in place by its H1Parser; one that
arrives in two pieces is buffered. Either way the request completes with the same response."""
import asyncio
import os
import socket

from beholder_amd.ops import H1Parser, IOFuture
from beholder_amd.sinks.http import HttpResponse
from beholder_amd.utils import netconn

REPLY = b"HTTP/1.1 200 OK\r\nContent-Type: application/json; charset=utf-8\r\nContent-Length: 2\r\n\r\n{}"
REQUEST = b"GET /x HTTP/1.1\r\nHost: sink\r\n\r\n"


def exchange(pieces):
    """One request over a socketpair whose peer answers with `pieces`, one send each, the next
    only after the connection has taken the one before: (inplace before, after, HttpResponse)."""
    async def go():
        loop = asyncio.get_running_loop()
        a, b = socket.socketpair()
        fd = os.dup(a.fileno())
        a.close()
        os.set_blocking(fd, False)
        lost = []

        class Owner:
            def _net_lost(self, exc):
                lost.append(exc)

            def _net_error(self, exc):
                lost.append(exc)

        parser = H1Parser()
        nc = netconn.NetConn(fd, loop, "h1", Owner(), parser)
        before = parser.inplace
        w = IOFuture(loop)
        nc.request(REQUEST, w, False)
        assert b.recv(100) == REQUEST
        fed = 0
        for piece in pieces:
            b.send(piece)
            fed += len(piece)
            for _ in range(1000):  # until the connection has read this piece
                if w.done() or parser.buffered == fed:
                    break
                await asyncio.sleep(0)
        status, _reason, raw, body, keep = await asyncio.wait_for(w, 5)
        after = parser.inplace
        nc.close()
        b.close()
        assert lost == [] and keep is True
        return before, after, HttpResponse(status, body, None, "http://sink/x", raw)
    return asyncio.run(go())


def test_one_send_is_parsed_in_place_two_sends_are_buffered():
    b1, a1, whole = exchange([REPLY])
    assert (b1, a1) == (0, 1)
    b2, a2, split = exchange([REPLY[:30], REPLY[30:]])
    assert (b2, a2) == (0, 0)
    for f in ("status", "body", "headers", "url", "ok"):
        assert getattr(whole, f) == getattr(split, f), f
    assert whole.status == 200 and whole.body == b"{}"
    assert whole.headers == {"content-type": "application/json; charset=utf-8", "content-length": "2"}
