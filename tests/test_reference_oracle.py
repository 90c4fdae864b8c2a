"""The reference's own business logic (``/root/reference/index.js:50-155``, run on Node) against
both handler implementations, event by event (``tests/reference_oracle.py`` has the details).

Compared per event: ack count, the status listener's rejection text (Q1), whether decode threw,
every sink request (method + full URL), every log line (level + message). At the end: counter
values and the media table's statuses. Modes: plain, ``NO_TRELLO`` (Q2), sink and store faults
(Q1, Q4, Q7: every awaited call of index.js fails on every seed,
``test_faults_mode_forces_every_failure``), pino@5's ``positional_args: drop`` (Q11), ``reread``
(Q3) and ``concurrent`` (Q9); at the handler level, through the whole consumer, and over real
sockets, where the forced failures are dropped connections and Postgres error replies. Without
``node`` or the reference checkout the reference's side comes from the recordings under
``tests/golden/reference_oracle/``.
"""
import pytest

import reference_oracle as ro
from beholder_amd.utils import netconn

pytestmark = pytest.mark.skipif(not ro.available(), reason="needs node and /root/reference/index.js")

SEEDS = range(5)
EVENTS = 520


@pytest.mark.parametrize("io", ["sync", "suspend"])
@pytest.mark.parametrize("mode", ro.MODES)
def test_reference_parity(mode, io):
    """``suspend``: the store and the sink client yield at every call, as production's socket
    clients do, so the compiled handlers finish every event in their resume states. The
    ``concurrent`` mode always suspends (at its gates) and is run once."""
    if mode == "concurrent" and io == "suspend":
        pytest.skip("the concurrent mode suspends at every call already")
    failures = {}
    for seed in SEEDS:
        sc = ro.make_scenario(seed, EVENTS, mode)
        ref = ro.run_node(sc)
        assert len(ref["events"]) == EVENTS
        for impl in ("python", "native"):
            d = ro.diff(ref, ro.run_python(sc, impl, suspend=io == "suspend"))
            if d:
                failures[(seed, impl)] = d
    assert not failures, "\n".join(f"{k}: " + "\n  ".join(v) for k, v in failures.items())


@pytest.mark.parametrize("io", ["sync", "suspend"])
def test_reference_parity_through_the_consumer(io):
    """Every sequential mode through the whole consumer (``run_service``): each event published to
    an in-process AMQP broker, delivered by ``AmqpSource``, dispatched by the service (the direct
    hand-over from the read callback when it waits), handled and acked over AMQP. Identical to
    ``index.js`` per event, as the handler-level gate, and most deliveries took the hand-over. The
    ``concurrent`` mode runs once (its gates suspend every call): the scripted interleavings of up
    to 4 deliveries in flight, step for step, through the service's dispatch and the compiled
    handlers' resumes."""
    failures = {}
    for mode in ro.MODES:
        if mode == "concurrent" and io == "suspend":
            continue
        for seed in range(2):
            sc = ro.make_scenario(seed, EVENTS, mode)
            ref = ro.run_node(sc)
            for impl in ("python", "native"):
                got = ro.run_service(sc, impl, suspend=io == "suspend")
                d = ro.diff(ref, got)
                if d:
                    failures[(mode, seed, impl)] = d
                assert got["path"]["direct_batches"] >= EVENTS // 2, got["path"]
    assert not failures, "\n".join(f"{k}: " + "\n  ".join(v) for k, v in failures.items())


@pytest.mark.parametrize("transport", ["tcp", "tls"])
def test_reference_parity_over_sockets(transport):
    """As above, with production's clients over TCP as well (``run_service(sockets=True)``): the
    media table in a Postgres wire-protocol server (tests/pg_fake.py) read and written by
    ``PostgresStore``, and every sink request sent by ``H1Client`` to a local HTTP server per
    origin, which records it under the reference's origin. Every store call and sink request waits
    on a socket, through the NetPoller; the compiled handlers finish in their resume states. The
    scenarios are :func:`reference_oracle.for_sockets`'s, on both sides. ``tls``: the sink servers
    speak HTTPS (as Trello and Telegram do), through the H1 client's native TLS connections."""
    failures = {}
    for mode in ro.MODES:
        if mode == "concurrent":
            continue
        for seed in range(2):
            sc = ro.for_sockets(ro.make_scenario(seed, EVENTS, mode))
            ref = ro.run_node(sc)
            for impl in ("python", "native"):
                got = ro.run_service(sc, impl, sockets=True, tls=transport == "tls")
                d = ro.diff(ref, got)
                if d:
                    failures[(mode, seed, impl)] = d
                # BEHOLDER_NATIVE_IO=0: every socket on an asyncio transport, no NetPoller
                assert got["path"]["netpoller"] == netconn.enabled(), got["path"]
                assert got["path"]["direct_batches"] >= EVENTS // 2, got["path"]
                if impl == "native":
                    assert got["path"]["suspended"] > EVENTS // 4, got["path"]
                # an error reply (the faults mode's store faults) leaves its connection in service:
                # the store opened its pool and nothing after it
                assert got["path"]["pg_connections"] <= got["path"]["pg_pool_size"], got["path"]
    assert not failures, "\n".join(f"{k}: " + "\n  ".join(v) for k, v in failures.items())


def test_concurrent_scenarios_interleave():
    """Mode ``concurrent`` (Q9, index.js:43,62,127): the reference's own runs of the scripted
    schedules have two deliveries of one media in flight, resume deliveries out of arrival order,
    and flip the DEPLOYED-hooks decision of some status events against their message (another
    delivery's UPDATE lands between an event's updateStatus and its getByID, index.js:68,76,94)."""
    total: dict = {}
    for seed in SEEDS:
        sc = ro.make_scenario(seed, EVENTS, "concurrent")
        for k, v in ro.concurrent_coverage(sc, ro.run_node(sc)).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total


def test_faults_mode_forces_every_failure():
    """Every ``faults`` scenario, at the suite's size and at the mutation gate's
    (tests/test_oracle_mutations.py), fails each awaited call of index.js in the reference's own
    run, so a handler that gets any of these wrong diverges on every seed:

    * Telegram for some DEPLOYED rows while Emby is on, and no Emby request follows (Q4,
      index.js:92-122); Emby is still asked after a Telegram success;
    * a comment POST on ``card1`` (index.js:53-57: not counted, warned, acked);
    * the card-move PUT of the pinned card (index.js:83-86): thrown, un-acked (Q1);
    * the Emby GET after a Telegram success (index.js:112,120-122): warned, acked;
    * ``updateStatus`` of an existing row (index.js:68): thrown, un-acked;
    * ``getByID`` of an existing row, in the status listener (index.js:76: un-acked) and in the
      progress listener (index.js:140,149-151: warned, acked).

    Seeds 0-4 at the suite's size and seeds 0-1 at 400 events. The socket form of each scenario
    (``for_sockets``) keeps every one of them a failure."""
    for events, seed in [(EVENTS, s) for s in SEEDS] + [(400, s) for s in range(2)]:
        sc = ro.make_scenario(seed, events, "faults")
        for form in (sc, ro.for_sockets(sc)):
            _forced_failures_occur(form, events, seed)


def _forced_failures_occur(form, events, seed):
    """One scenario form: the reference's own run of it holds every forced failure."""
    ref = ro.run_node(form)
    assert len(ref["events"]) == events
    reqs = [(e, m, u) for e in ref["events"] for m, u in e["requests"]]
    failed_tg = [e for e, m, u in reqs if u.startswith(ro.TELEGRAM_FAULT_PREFIX)]
    assert failed_tg and all(not any("/emby/" in u for _, u in e["requests"]) for e in failed_tg), seed
    assert any("/emby/" in u for _, _, u in reqs), seed
    assert any(u.startswith("https://api.trello.com/1/cards/card1/actions/comments") for _, _, u in reqs), seed
    cov = ro.forced_failure_coverage(ref)
    print(f"faults seed {seed} events {events} sockets {bool(form.get('sockets'))}: {cov}")
    assert set(cov) == {"card_move_failed_unacked", "emby_failed_after_telegram", "update_failed_unacked",
                        "get_failed_unacked", "get_failed_progress_warned"}
    assert all(v >= 1 for v in cov.values()), (seed, cov)
    # a failed updateStatus left its row as it was (no other call writes a status)
    m4 = next(m for m in form["media"] if m["id"] == "m4")
    assert ref["media"]["m4"] == m4["status"], seed


def test_streams_reach_every_reference_branch():
    """The gate is only as good as its streams: every branch of index.js:50-155 is reached."""
    total = {}
    for mode in ro.MODES:
        for seed in SEEDS:
            cov = ro.coverage(ro.run_node(ro.make_scenario(seed, EVENTS, mode)))
            for k, v in cov.items():
                total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total


# one-line mutations of the business logic, applied to the handler object both implementations read
MUTATIONS = {
    "deployed_enum": lambda h: setattr(h, "deployed", 3),             # index.js:94 compares DEPLOYED
    "trello_creator": lambda h: setattr(h, "trello_creator", 0),      # index.js:142
    "flow_lists": lambda h: setattr(h, "lists", dict(h.lists, converting="L-other")),  # index.js:80
    "no_trello": lambda h: setattr(h, "no_trello", True),             # index.js:70
}


@pytest.mark.parametrize("impl", ["python", "native"])
@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_gate_catches_mutations(name, impl):
    sc = ro.make_scenario(1, EVENTS, "faults" if name == "deployed_enum" else "base")
    ref = ro.run_node(sc)
    assert not ro.diff(ref, ro.run_python(sc, impl))
    assert ro.diff(ref, ro.run_python(sc, impl, mutate=MUTATIONS[name]))


def test_reference_parity_on_the_bench_workload():
    """The bench's own event stream, config and media table, one event at a time: zero
    differences. (The concurrent Node A/B, scripts/bench_reference_node.py, can differ by a few
    sink requests in hundreds of thousands: concurrent status events for one media re-read its
    status in a different interleaving, quirks Q3/Q9; one at a time there is no interleaving.)"""
    sc = ro.bench_scenario(3000, seed=1)
    ref = ro.run_node(sc)
    for impl in ("native", "python"):
        assert ro.diff(ref, ro.run_python(sc, impl)) == [], impl
    assert sum(len(e["requests"]) for e in ref["events"]) > 1000
