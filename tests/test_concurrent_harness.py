"""tests/concurrent_harness.py on the CPU, with stand-in jobs: time.sleep releases the GIL as a ctypes call into the library does."""
import threading
import time

import pytest

import concurrent_harness as CH


def sleeper(ms, out=None):
    def f():
        time.sleep(ms / 1000.0)
        return out
    return f


def test_overlap_on_a_hand_made_timeline():
    C = CH.Call
    calls = [C("a", 0, "j", 0.0, 1.0, None), C("a", 0, "j", 1.0, 2.0, None), C("a", 1, "j", 5.0, 6.0, None), C("a", 1, "j", 8.0, 9.0, None),
             C("b", 0, "j", 1.5, 1.6, None), C("b", 0, "j", 6.0, 7.0, None),            # 6.0: touches a's [5, 6]
             C("c", 0, "j", 20.0, 21.0, None)]
    s = CH.overlap_shares(calls)
    assert s == {"a": 0.5, "b": 1.0, "c": 0.0}                   # a: [1, 2] and [5, 6] of four; a's own calls do not count for a
    assert CH.overlap_shares([C("a", 0, "j", 0.0, 1.0, None)]) == {"a": 0.0}
    r = CH.Result(["a", "b", "c", "d"], calls, [], [], 1.0)
    assert r.shares["d"] == 0.0                                  # a worker that made no call
    with pytest.raises(AssertionError, match="made no call"):
        r.check()
    with pytest.raises(AssertionError, match="tested nothing"):
        CH.Result(["a", "b", "c"], calls, [], [], 1.0).check()
    CH.Result(["a", "b"], calls[:6], [], [], 1.0).check()


def test_four_workers_overlap_and_every_call_is_recorded():
    workers = [(str(i), lambda: [("x", sleeper(2)), ("y", sleeper(3))]) for i in range(4)]
    r = CH.run(workers, rounds=5, limit_s=20)
    assert len(r.calls) == 4 * 5 * 2 and not r.hung and not r.setup_errors and not r.failures
    assert all(c.t1 >= c.t0 for c in r.calls)
    assert sorted((c.round, c.job) for c in r.calls if c.worker == "2") == sorted((k, j) for k in range(5) for j in "xy")
    r.check()
    assert all(s >= 0.9 for s in r.shares.values()), r.report()


def test_a_wrong_result_and_an_exception_are_reported_with_worker_round_and_job():
    n = {"boom": 0, "wrong": 0}

    def boom():
        n["boom"] += 1
        time.sleep(0.001)
        if n["boom"] == 3:
            raise ValueError("status 2")

    def wrong():
        n["wrong"] += 1
        time.sleep(0.001)
        return "match_idx differs at 17" if n["wrong"] == 2 else None
    r = CH.run([("good", lambda: [("g", sleeper(1))]), ("bad", lambda: [("boom", boom), ("wrong", wrong)])], rounds=4, limit_s=20)
    got = sorted((c.worker, c.round, c.job, c.outcome) for c in r.failures)
    assert got == [("bad", 1, "wrong", "match_idx differs at 17"), ("bad", 2, "boom", "raised ValueError('status 2')")]
    assert len(r.calls) == 4 + 8                                 # the list went on after the exception
    with pytest.raises(AssertionError, match="2 of 12 calls"):
        r.check()


def test_a_failed_setup_starts_nobody():
    started = []

    def bad():
        raise RuntimeError("no device")
    r = CH.run([("a", lambda: [("x", lambda: started.append(1))]), ("b", bad)], rounds=3, limit_s=20)
    assert not started and not r.calls and [w for w, _ in r.setup_errors] == ["b"] and "no device" in r.setup_errors[0][1]
    with pytest.raises(AssertionError, match="setup failed"):
        r.check()


def test_a_worker_past_its_limit_is_reported_as_hung():
    gate = threading.Event()
    t0 = time.perf_counter()
    r = CH.run([("fast", lambda: [("x", sleeper(1))]), ("stuck", lambda: [("wait", lambda: gate.wait(30) and None)])], rounds=1, limit_s=0.3)
    assert time.perf_counter() - t0 < 5
    gate.set()
    assert r.hung == ["stuck"]
    with pytest.raises(AssertionError, match="did not finish"):
        r.check()


def test_rounds_of_its_own_and_a_background_worker_that_stops_with_the_others():
    r = CH.run([("fg", lambda: [("x", sleeper(2))]), ("twice", lambda: [("y", sleeper(2))], 2), ("bg", lambda: [("z", sleeper(1))], CH.BACKGROUND)], rounds=10, limit_s=20)
    n = {w: sum(1 for c in r.calls if c.worker == w) for w in r.workers}
    assert n["fg"] == 10 and n["twice"] == 2 and n["bg"] >= 5, n
    last_fg = max(c.t1 for c in r.calls if c.worker == "fg")
    assert sum(1 for c in r.calls if c.worker == "bg" and c.t0 > last_fg) <= 1       # it stops at the first look after the others are done
    assert not r.hung and r.shares["bg"] >= 0.5


def test_keep_going_lets_the_short_lists_run_as_long_as_the_longest():
    workers = [("long", lambda: [("x", sleeper(20))]), ("short", lambda: [("y", sleeper(1))])]
    plain = CH.run(workers, rounds=5, limit_s=20)
    assert plain.shares["long"] < 0.5                             # the short list is over within the long one's first call
    with pytest.raises(AssertionError, match="tested nothing"):
        plain.check()
    r = CH.run(workers, rounds=5, limit_s=20, keep_going=True)
    n = {w: sum(1 for c in r.calls if c.worker == w) for w in r.workers}
    assert n["long"] == 5 and n["short"] > 20, n
    r.check()
