"""The late-inputs / early-snapshot harness of tests/test_gpu_stream_order.py: does a `*_device` entry point do ALL of its work in the
order of the stream it is given?

The usual -m gpu test uploads with a blocking hipMemcpy, calls, and reads behind hipDeviceSynchronize(): the inputs are complete before the call and the
device is idle before the read, so a launch on the wrong stream, a fork behind the wrong event or a missing join give the right bytes all the same.  Here
the caller's stream s is held back by a delay, the real inputs reach their buffers only behind it (device-to-device copies on s), the outputs are copied
to snapshots on s right behind the call and then overwritten on s, and the host waits for s alone:

  before anything is enqueued   inputs <- the DECOY (a second valid case of the same sizes), staging <- the real inputs, outputs <- 0x55,
                                snapshots <- 0xAA; one device-wide wait
  on s, no host wait between    delay | staging -> inputs | the call(stream = s) | outputs -> snapshots | outputs <- 0xEE     ... the next step the same
  right after a step's last     the event recorded behind the step's delay must be NOT READY: the inputs had not arrived when the host finished
  enqueue                       enqueueing the step.  If it is ready the run proves nothing: drain, double the delay, run the whole scene again
                                (three times at the most)
  read                          hipStreamSynchronize(s) and nothing wider; plain hipMemcpy of the snapshots and the outputs

A kernel that ran anywhere but behind the copies on s read the decoy (its result, or the 0x55 fill, is in the snapshot); one that ran behind the
snapshot copy left 0x55 there and its result over the 0xEE.  The decoy is a valid case, so nothing reads an index out of range whatever the order.

A scene is a list of Steps on one stream, each with buffers of its own (a step's decoy is valid for ITS sizes only).  A step may take an input from an
earlier step's output buffer (`link`): that buffer starts from the decoy's valid intermediate result (`prefill`), not from 0x55, and is not overwritten
behind the call that produced it."""
import time

import numpy as np

import hipmem

FILL_OUT, FILL_SNAP, FILL_AFTER = 0x55, 0xAA, 0xEE
DELAY_BYTES = 256 << 20          # one delay copy: 256 MiB read + 256 MiB written, ~0.1 ms at the copy roof of DESIGN.md 6
DELAY_REPS = 32                  # the first attempt: 16 GiB moved, ~3 ms; doubled while the host is still enqueueing when the delay ends
MAX_ATTEMPTS = 3


class Step:
    """one entry-point call.
    inputs   {key: (real, decoy)}: numpy arrays of equal shape and dtype
    outputs  {key: bytes}
    work     {key: bytes}: caller-owned work areas (0x55-filled, not compared)
    call     f(p, stream): enqueues the entry point; p[key] is the device address of every input, output and work area, `stream` the raw handle
    expect   {key: [(byte offset, real array, decoy array), ...]}: the DEFINED bytes of an output and what the reference gives for both cases;
             compared exactly.  An output that is compared within a tolerance goes to `check` instead
    check    f(got, which) or None: got[key] the output's bytes (uint8); asserts as the module's own GPU test does (which = "real")
    link     {input key: (step index, output key)}: this input IS that earlier output's buffer (no staging, no copy)
    prefill  {output key: array}: what a linked-to output holds before anything runs (the decoy's valid result)
    waits    None, or WHY this call may wait on the host (a regrow that drains the stream, an upload): such a wait lets the step's delay run out, so
             the not-ready condition is not asked of it; its bytes and its place in the stream are checked all the same"""

    def __init__(self, name, inputs, outputs, call, expect, work=None, check=None, link=None, prefill=None, waits=None):
        self.name, self.inputs, self.outputs, self.call, self.expect = name, inputs, outputs, call, expect
        self.work, self.check, self.link, self.prefill, self.waits = work or {}, check, link or {}, prefill or {}, waits
        names = list(inputs) + list(outputs) + list(self.work) + list(self.link)
        assert len(names) == len(set(names)), (name, "two buffers of one name")
        for k, (a, b) in inputs.items():
            assert a.shape == b.shape and a.dtype == b.dtype, (name, k, a.shape, b.shape)


def _raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class _Delay:
    _bufs = None

    @classmethod
    def bufs(cls):
        if cls._bufs is None:                                     # two scratch buffers, allocated once per process
            cls._bufs = hipmem.DevBuf(DELAY_BYTES), hipmem.DevBuf(DELAY_BYTES)
        return cls._bufs


def _enqueue_delay(ex, reps, s):
    a, b = _Delay.bufs()
    for _ in range(reps):
        ex.debug_stream_copy(b.ptr, a.ptr, DELAY_BYTES, 16, s.ptr)


def _attempt(delay_ex, steps, s, call_stream, reps):
    """-> (conclusive, snapshots, outputs_after) of one run of the scene"""
    D = hipmem.DevBuf
    bufs, staging, snaps, keep = [], [], [], set(link for st in steps for link in st.link.values())
    for i, st in enumerate(steps):                                # ---- before anything is enqueued
        b, g = {}, {}
        for k, (j, ok) in st.link.items():
            b[k] = bufs[j][ok]
        for k, (real, decoy) in st.inputs.items():
            assert k not in st.link, (st.name, k)
            b[k], g[k] = D.from_numpy(_raw(decoy)), D.from_numpy(_raw(real))
        for k, nbytes in list(st.outputs.items()) + list(st.work.items()):
            b[k] = D(nbytes, zero=False)
            b[k].fill(FILL_OUT)
            if k in st.prefill:
                a = _raw(st.prefill[k])
                assert a.nbytes <= nbytes
                hipmem._ok(hipmem.hip().hipMemcpy(b[k].ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
        sn = {k: D(nbytes, zero=False) for k, nbytes in st.outputs.items()}
        for v in sn.values():
            v.fill(FILL_SNAP)
        bufs.append(b); staging.append(g); snaps.append(sn)
    hipmem.sync()
    events, held = [hipmem.Event() for _ in steps], []
    for i, st in enumerate(steps):                                # ---- on s, no host wait from here ...
        _enqueue_delay(delay_ex, reps, s)
        events[i].record(s)
        for k, g in staging[i].items():
            hipmem.copy_async(bufs[i][k].ptr, g.ptr, _raw(st.inputs[k][0]).nbytes, s)
        st.call({k: v.ptr for k, v in bufs[i].items()}, (call_stream or s).ptr)
        for k, nbytes in st.outputs.items():
            hipmem.copy_async(snaps[i][k].ptr, bufs[i][k].ptr, nbytes, s)
            if (i, k) not in keep:
                hipmem.memset_async(bufs[i][k].ptr, FILL_AFTER, nbytes, s)
        held.append(not events[i].ready())                        # the step's delay was still running when its last enqueue returned
    #                                                               ... to here
    for st, h in zip(steps, held):
        if st.waits:
            print("  %s may wait on the host (%s): its delay had %s when the call returned" % (st.name, st.waits, "not ended" if h else "ended"))
    conclusive = all(h or st.waits for st, h in zip(steps, held))
    s.synchronize()                                               # ---- hipStreamSynchronize(s) and nothing wider; then plain hipMemcpy
    got = [{k: v.read_after(s, count=st.outputs[k]) for k, v in snaps[i].items()} for i, st in enumerate(steps)]
    after = [{k: bufs[i][k].read_after(s, count=nbytes) for k, nbytes in st.outputs.items() if (i, k) not in keep} for i, st in enumerate(steps)]
    if call_stream is not None:
        call_stream.synchronize()
    hipmem.sync()                                                 # everything read: drain whatever else there is before the buffers are freed
    return conclusive, got, after


CALLER_STREAMS = 2               # every scene runs on this many caller streams, created together (see run)


def run(delay_ex, scene, call_stream=None, tag=""):
    """runs scene() -> [Step] (built anew for every attempt: fresh handles stay fresh) until an attempt is conclusive, once on each of CALLER_STREAMS
    caller streams.  -> [(steps, snapshots, outputs afterwards)] per caller stream.  Why more than one stream: the runtime maps streams onto a few
    hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and two streams on ONE queue execute in the order the host submitted them — a launch that
    went to a library stream sharing the caller's queue runs behind the delay and the late inputs and goes unnoticed.  Streams that are alive together
    are dealt onto different queues, so a given library stream can share a queue with at most one of the caller streams.
    `call_stream`: the negative control only — the entry points get THIS stream while everything else goes to the caller stream"""
    streams = [hipmem.Stream(non_blocking=True) for _ in range(CALLER_STREAMS)]     # not ordered with the NULL stream: a launch that lands there is out of order too
    return [_run_on(delay_ex, scene, s, call_stream, "%s [caller stream %d]" % (tag, i)) for i, s in enumerate(streams)]


def _run_on(delay_ex, scene, s, call_stream, tag):
    reps = DELAY_REPS
    for attempt in range(MAX_ATTEMPTS):
        steps = scene()
        t0 = time.time()
        conclusive, got, after = _attempt(delay_ex, steps, s, call_stream, reps)
        if conclusive:
            print("stream order %s: conclusive with a delay of %d x %d MiB copies (%.1f GiB moved), attempt %d, %.2f s"
                  % (tag, reps, DELAY_BYTES >> 20, 2.0 * reps * DELAY_BYTES / 2 ** 30, attempt + 1, time.time() - t0))
            return steps, got, after
        reps *= 2
    raise AssertionError("%s: could not hold the stream back (the delay had ended before the last enqueue returned, up to %d copies)" % (tag, reps // 2))


def mismatches(step, got):
    """the expect entries of `step` whose snapshot bytes differ from the real case's reference -> [(key, offset, what the bytes are)]"""
    bad = []
    for k, segs in step.expect.items():
        for off, real, decoy in segs:
            r, d = _raw(real), _raw(decoy)
            g = got[k][off:off + r.nbytes]
            if g.tobytes() != r.tobytes():
                gd = got[k][off:off + d.nbytes]                     # (the decoy's count may differ: its defined extent is its own)
                what = "the decoy's result" if gd.tobytes() == d.tobytes() else "0x55" if (g == FILL_OUT).all() else "0xAA" if (g == FILL_SNAP).all() else "other bytes"
                bad.append((k, off, what))
    return bad


def check(steps, got, after, tag=""):
    """the assertions of one conclusive run"""
    for i, st in enumerate(steps):
        bad = mismatches(st, got[i])
        assert not bad, (tag, st.name, "snapshot differs from the reference of the real inputs", bad)
        for k, segs in st.expect.items():                         # every defined byte: neither the fill nor the decoy's result where those differ from the reference
            for off, real, decoy in segs:
                r, d = _raw(real), _raw(decoy)
                g = got[i][k][off:off + r.nbytes]
                assert not ((g == FILL_OUT) & (r != FILL_OUT)).any(), (tag, st.name, k, "0x55 in a defined byte")
                m = min(r.nbytes, d.nbytes)
                assert not ((g[:m] == d[:m]) & (r[:m] != d[:m])).any(), (tag, st.name, k, "the decoy's result in a defined byte")
        if st.check is not None:
            st.check(got[i], "real")
        for k, a in after[i].items():
            assert (a == FILL_AFTER).all(), (tag, st.name, k, "written behind the call's place in the stream: %d bytes" % int((a != FILL_AFTER).sum()))
