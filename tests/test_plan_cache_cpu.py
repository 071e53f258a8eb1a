"""The plan cache of the reference-signature wrappers (engine.borrowed_plan) from several host threads, and the library's
error text per thread -- no GPU.

The cache is driven with stub plans: an object with close() and a run() that raises a counter of holders, sleeps a
millisecond and lowers it (a stub has no device, so the cache records and waits for no event).  What must hold whatever the
threads do: no stub is ever held by two callers, none is closed while held or run after its close, none is closed twice, and
at most _MAX_PLANS stubs stay idle.  `scenario_same_key` and `scenario_eviction` take the way a caller gets and uses a plan as an
argument (`use(key, factory, body)`), so the same scenarios can be pointed at another cache.

The error text: two threads provoke two different QI_ERR_ARG refusals at once (those of tests/test_resample_cpu.py, which
come before the device) and each must read its own message from qi_last_error() every time."""
import ctypes as C
import random
import threading
import time

import numpy as np
import pytest

from quantum_inferno_amd import _lib, engine

THREADS = 4


class Stub:
    """A plan as the cache sees it: close(), and run() in place of a transform call."""

    def __init__(self, book, key):
        self.key = key
        self._mu = threading.Lock()
        self.holders = self.most_holders = self.runs = self.closes = 0
        self.closed_in_use = self.run_after_close = False
        with book.mu:
            book.made.append(self)

    def run(self):
        with self._mu:
            self.holders += 1
            self.runs += 1
            self.most_holders = max(self.most_holders, self.holders)
            self.run_after_close |= self.closes > 0
        time.sleep(0.001)
        with self._mu:
            self.holders -= 1

    def close(self):
        with self._mu:
            self.closes += 1
            self.closed_in_use |= self.holders > 0


class Book:
    """Every stub a scenario's factories made."""

    def __init__(self):
        self.mu = threading.Lock()
        self.made = []

    def factory(self, key):
        return lambda: Stub(self, key)

    def faults(self):
        """What went wrong, in words; empty when the contract held."""
        out = []
        for k, s in enumerate(self.made):
            if s.most_holders > 1:
                out.append(f"stub {k} (key {s.key}) was held by {s.most_holders} callers at once")
            if s.closed_in_use:
                out.append(f"stub {k} (key {s.key}) was closed while a caller was inside run()")
            if s.run_after_close:
                out.append(f"stub {k} (key {s.key}) was run after its close()")
            if s.closes > 1:
                out.append(f"stub {k} (key {s.key}) was closed {s.closes} times")
        return out


def in_threads(count, body):
    """body(thread index) in `count` threads released by one barrier; what a thread raised is raised here."""
    barrier = threading.Barrier(count)
    raised = []

    def run(t):
        try:
            barrier.wait()
            body(t)
        except BaseException as e:  # noqa: BLE001 (handed to the main thread)
            raised.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(count)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if raised:
        raise raised[0]


def use_borrowed(key, factory, body):
    with engine.borrowed_plan(key, factory) as plan:
        body(plan)


def scenario_same_key(use, rounds=25):
    """Four threads, one key."""
    book = Book()
    in_threads(THREADS, lambda t: [use("k", book.factory("k"), Stub.run) for _ in range(rounds)])
    assert sum(s.runs for s in book.made) == THREADS * rounds
    return book


def scenario_eviction(use, rounds=40, keys=5):
    """Four threads over five keys: more keys than _MAX_PLANS, so plans are evicted while others are in use."""
    assert keys > engine._MAX_PLANS
    book = Book()

    def body(t):
        rng = random.Random(1000 + t)
        for _ in range(rounds):
            key = rng.randrange(keys)
            use(key, book.factory(key), Stub.run)

    in_threads(THREADS, body)
    assert sum(s.runs for s in book.made) == THREADS * rounds
    return book


@pytest.fixture(autouse=True)
def empty_cache():
    engine.clear_plans()
    assert not engine._PLANS
    yield
    engine.clear_plans()
    assert not engine._PLANS


def idle_stubs():
    with engine._PLANS_LOCK:
        return [e.plan for e in engine._PLANS.values()]


def test_same_key_from_four_threads():
    book = scenario_same_key(use_borrowed)
    assert not book.faults(), book.faults()
    assert 1 <= len(book.made) <= THREADS * 25
    idle = idle_stubs()
    assert len(idle) <= engine._MAX_PLANS and all(s.closes == 0 for s in idle)
    assert sorted(map(id, idle)) == sorted(id(s) for s in book.made if s.closes == 0)  # what is not idle has been closed


def test_eviction_under_four_threads():
    book = scenario_eviction(use_borrowed)
    assert not book.faults(), book.faults()
    idle = idle_stubs()
    assert len(idle) <= engine._MAX_PLANS and all(s.closes == 0 for s in idle)
    assert sorted(map(id, idle)) == sorted(id(s) for s in book.made if s.closes == 0)
    assert len(book.made) > engine._MAX_PLANS  # (five keys were used: something was evicted)


def test_one_thread_reuses_and_evicts_least_recently_used():
    book = Book()
    for key in ("a", "b", "c", "a", "d"):  # "a" is used again, so "b" is the least recently used when "d" comes back
        use_borrowed(key, book.factory(key), Stub.run)
    assert [s.key for s in book.made] == ["a", "b", "c", "d"]
    assert [s.key for s in book.made if s.closes] == ["b"] and book.made[0].runs == 2
    assert [s.key for s in idle_stubs()] == ["c", "a", "d"]
    assert not book.faults()


def test_a_busy_key_gets_a_plan_of_its_own_without_waiting():
    book = Book()
    with engine.borrowed_plan("k", book.factory("k")) as first:
        with engine.borrowed_plan("k", book.factory("k")) as second:  # (one thread: waiting here would never end)
            assert second is not first
    assert len(book.made) == 2 and len(idle_stubs()) == 2 and not book.faults()


def test_a_plan_comes_back_when_its_borrower_raises():
    book = Book()
    with pytest.raises(ZeroDivisionError):
        with engine.borrowed_plan("k", book.factory("k")):
            1 / 0
    assert idle_stubs() == book.made and book.made[0].closes == 0


def test_clear_closes_every_plan_once_and_a_borrowed_one_on_its_return():
    book = Book()
    held, release = threading.Event(), threading.Event()

    def borrower():
        with engine.borrowed_plan("held", book.factory("held")) as plan:
            plan.run()
            held.set()
            assert release.wait(30)

    th = threading.Thread(target=borrower)
    th.start()
    assert held.wait(30)
    for key in ("a", "b"):
        use_borrowed(key, book.factory(key), Stub.run)
    assert len(idle_stubs()) == 2
    engine.clear_plans()  # while "held" is borrowed
    assert not engine._PLANS
    assert [(s.key, s.closes) for s in book.made] == [("held", 0), ("a", 1), ("b", 1)]
    release.set()
    th.join()
    assert not engine._PLANS  # it was closed, not kept
    assert [s.closes for s in book.made] == [1, 1, 1] and not book.faults()
    engine.clear_plans()
    assert [s.closes for s in book.made] == [1, 1, 1]


def test_last_error_is_per_thread():
    """Two threads, fifty refusals each, a different one per thread: each reads its own message after every call."""
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    calls = {
        0: (lambda: lib.qi_interp_grid(_lib.QI_F64, 0, p, p, 0, 1, 8, 0.0, 0.0, 4, p, None), b"delta"),
        1: (lambda: lib.qi_resample_fft(_lib.QI_F64, 0, p, 1, 8, 4, p, p, 16, None), b"needed"),
    }
    for call, word in calls.values():  # alone first: the messages are what this test takes them for
        assert call() == -1 and word in lib.qi_last_error()
        assert all(other not in lib.qi_last_error() for _, other in calls.values() if other != word)  # and tell the two apart
    seen = {0: [], 1: []}

    def body(t):
        call, _ = calls[t]
        for _ in range(50):
            rc = call()
            seen[t].append((rc, lib.qi_last_error()))

    in_threads(2, body)
    for t, (_, word) in calls.items():
        other = calls[1 - t][1]
        assert len(seen[t]) == 50
        assert all(rc == -1 and word in msg and other not in msg for rc, msg in seen[t]), [m for _, m in seen[t] if word not in m][:3]
