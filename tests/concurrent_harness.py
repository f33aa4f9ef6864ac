"""Worker threads with handles of their own, released together: the harness of tests/test_gpu_concurrent_handles.py.  Nothing here
touches the GPU; tests/test_concurrent_harness.py holds it on the CPU with stand-in jobs.  (Not named concurrent.py: a module of that name on sys.path
would stand in front of the standard library's `concurrent` package.)

A worker is (name, setup): setup() runs ON the worker's thread, creates whatever the worker owns (handles, device buffers) and returns its job list,
[(job name, f)], where f() makes one call and returns None when the result is the expected one, or a short text naming the first field that differs.
All workers finish their setup, meet at a barrier, and then run their lists `rounds` times.  A worker given as (name, setup, k) runs its list k times
instead; (name, setup, BACKGROUND) keeps the device busy: it repeats its list, at least once, until every other worker has finished.  With keep_going every
worker goes on with further rounds until the slowest has done its own: lists of unequal length then overlap to their ends (the remedy for a run
below the overlap condition is more rounds, and this gives them to the workers that would otherwise stand idle).  Per call the harness keeps (t_start, t_end) on the host
clock and the outcome; an exception is an outcome ("raised ..."), never swallowed and never the end of the thread's list.  A setup that raises breaks
the barrier: nobody starts.  A worker that has not finished `limit_s` seconds after the start is reported as hung; its thread is a daemon and is
left behind, and Result.hung tells the caller to start nothing more."""
import threading
import time
import traceback

BACKGROUND = "background"
MIN_SHARE = 0.5          # the overlap condition: at least this share of EVERY worker's calls overlapped a call of another worker, or the run tested nothing


class Call:
    __slots__ = ("worker", "round", "job", "t0", "t1", "outcome")

    def __init__(self, worker, rnd, job, t0, t1, outcome):
        self.worker, self.round, self.job, self.t0, self.t1, self.outcome = worker, rnd, job, t0, t1, outcome

    def __repr__(self):
        return "worker %s round %d job %s: %s" % (self.worker, self.round, self.job, self.outcome or "ok")


def overlap_shares(calls):
    """{worker: share of its calls whose [t0, t1] intersects the [t0, t1] of some call of ANOTHER worker}; a worker without calls has share 0"""
    by = {}
    for c in calls:
        by.setdefault(c.worker, []).append(c)
    out = {}
    for w, mine in by.items():
        others = sorted(((c.t0, c.t1) for c in calls if c.worker != w))
        hit = sum(1 for c in mine if any(a <= c.t1 and c.t0 <= b for a, b in others))
        out[w] = hit / len(mine) if mine else 0.0
    return out


class Result:
    def __init__(self, workers, calls, setup_errors, hung, seconds, setup_seconds=0.0):
        self.workers, self.calls, self.setup_errors, self.hung, self.seconds, self.setup_seconds = workers, calls, setup_errors, hung, seconds, setup_seconds
        self.shares = overlap_shares(calls)
        for w in workers:
            self.shares.setdefault(w, 0.0)

    @property
    def failures(self):
        return [c for c in self.calls if c.outcome is not None]

    def report(self):
        n = {w: sum(1 for c in self.calls if c.worker == w) for w in self.workers}
        return "%d workers, %.2f s of which %.2f s setup: " % (len(self.workers), self.seconds, self.setup_seconds) + ", ".join("%s %d calls, %.0f %% overlapped" % (w, n[w], 100 * self.shares[w]) for w in self.workers)

    def check(self, min_share=MIN_SHARE):
        """the assertions of one run: nobody hung, every setup worked, every call gave the expected result, and the overlap condition holds"""
        assert not self.hung, "workers that did not finish within their limit (nothing more is to be started): %s" % self.hung
        assert not self.setup_errors, "setup failed: %s" % self.setup_errors
        assert not self.failures, "%d of %d calls: %s" % (len(self.failures), len(self.calls), self.failures[:5])
        assert all(any(c.worker == w for c in self.calls) for w in self.workers), "a worker made no call"
        low = {w: s for w, s in self.shares.items() if s < min_share}
        assert not low, "this run tested nothing: fewer than %.0f %% of the calls of %s overlapped another worker's (more rounds are the remedy)" % (100 * min_share, low)


def run(workers, rounds, limit_s=60.0, clock=time.perf_counter, keep_going=False):
    """workers: [(name, setup) or (name, setup, rounds of its own or BACKGROUND)] -> Result"""
    workers = [(w[0], w[1], w[2] if len(w) > 2 else rounds) for w in workers]
    names = [w[0] for w in workers]
    assert len(set(names)) == len(names) and any(w[2] != BACKGROUND for w in workers)
    barrier = threading.Barrier(len(workers))
    calls, setup_errors, lock = [], [], threading.Lock()
    left, done, released = [sum(1 for w in workers if w[2] != BACKGROUND)], threading.Event(), [None]

    def finished(own):
        if own != BACKGROUND:
            with lock:
                left[0] -= 1
                if left[0] == 0:
                    done.set()

    def body(name, setup, own):
        try:
            jobs = setup()
        except BaseException as e:                                  # nobody starts
            with lock:
                setup_errors.append((name, "%r\n%s" % (e, traceback.format_exc(limit=4))))
            barrier.abort()
            done.set()
            return
        try:
            barrier.wait(timeout=limit_s)
        except threading.BrokenBarrierError:
            return
        released[0] = time.perf_counter()
        mine, r = [], -1
        while (not done.is_set() or r < 0) if own == BACKGROUND else (r + 1 < own or (keep_going and not done.is_set())):
            r += 1
            for job, f in jobs:
                t0 = clock()
                try:
                    out = f()
                except BaseException as e:
                    out = "raised %r" % (e,)
                mine.append(Call(name, r, job, t0, clock(), None if out is None else str(out)[:300]))
            if r + 1 == own:                                        # that was the last round it owes
                finished(own)
        with lock:
            calls.extend(mine)

    threads = [threading.Thread(target=body, args=w, name="worker-%s" % w[0], daemon=True) for w in workers]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    deadline = t0 + limit_s
    for t in threads:
        t.join(max(0.0, deadline - time.perf_counter()))
    hung = [w for w, t in zip(names, threads) if t.is_alive()]
    with lock:
        return Result(names, list(calls), list(setup_errors), hung, time.perf_counter() - t0, (released[0] or time.perf_counter()) - t0)
