"""GPU tests of the stream and thread contract (include/aarmvs.h, "Streams and threads"): a call
is ordered on the caller's stream after what the stream held and before what follows, two sweeps
(or a training step and a sweep) may be in flight on two streams or in two host threads, and one
DepthSweep may change geometry while its last sweep is still queued.  The helpers, the delay /
poison / serial-reference method and the shapes are tests/stream_cases.py; the same scenarios on
the CPU model of the schedule are tests/sweep_schedule_check.cpp (check_two_sweeps).

Everything is compared bit for bit with the same call made alone on the default stream (every
schedule is documented as bit-identical); test_serial_references_are_right ties those serial runs
to the float64 / CPU oracle at the project's tolerances.  Nothing here is captured into a graph
and the profiler stays off.
"""
import ctypes
import os
import threading
import time

import numpy as np
import pytest
import torch

import stream_cases as sc
from stream_cases import DEV, FRAMES

pytestmark = pytest.mark.gpu
FRAME_IDS = ["x".join(map(str, f)) for f in FRAMES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    torch.set_num_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def streams():
    """The callers' side streams, made once (consecutive streams of torch's pool)."""
    sc._sleep_cycles_per_ms()   # (measured here, outside any timed enqueue)
    return {k: torch.cuda.Stream() for k in ("s", "p", "a", "b")}


def on_stream(stream, gen):
    """``gen`` advanced one step at a time with ``stream`` current."""
    it = iter(gen)
    while True:
        with torch.cuda.stream(stream):
            try:
                item = next(it)
            except StopIteration:
                return
        yield item


def _serial(make_gen):
    """(serial results, host seconds of the enqueue), the library warmed first (stream and event
    creation, code object load) so that the time is an enqueue's."""
    sc.timed_serial(make_gen)
    return sc.timed_serial(make_gen)


def _rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


# ---------------------------------------------------------------------------------------
# the serial references against the oracle: "equal to serial" then means "right"
# ---------------------------------------------------------------------------------------
def test_serial_references_are_right():
    """One eval case and one training case of the shapes below, made alone on the default
    stream, against the CPU oracle at the project's tolerances: cost atol = rtol = 1e-4, depth
    relative L1 <= 1e-3 (test_gpu_parity.py), gradients by test_gpu_bptt.bound."""
    from oracle import sweep_oracle as orc
    import test_gpu_bptt as tb
    frame = B, N, H, W, D = FRAMES[0]
    scene = sc.Scene(frame, seed=21, poison_seed=22)
    sw, P = sc.make_sweep(6)
    feats, proj, dv = scene.host["true"]
    scene.fill("true")
    ev, _ = sc.timed_serial(lambda res: sc.eval_steps(sw, scene, res))
    ref = orc.sweep(feats[0], [feats[v] for v in range(1, N)], proj[:, 0], [proj[:, v] for v in range(1, N)], dv, P)
    np.testing.assert_allclose(ev["cost"].cpu().numpy(), ref["cost"].numpy(), atol=1e-4, rtol=1e-4)
    assert _rel_l1(ev["depth"].cpu().numpy(), ref["depth"].numpy()) <= 1e-3
    # the training step: L = sum(R * softmax(cost)), as tests/test_gpu_bptt.py
    rec = sw.record_buffers(B, H, W, D, DEV, nsrc=N - 1)
    tr, _ = sc.timed_serial(lambda res: sc.train_steps(sw, scene, rec, res))
    R = scene.R.cpu()
    tsum = [0.0]
    orc.LOGIT_HOOK = lambda z: z.register_hook(lambda g: tsum.__setitem__(0, tsum[0] + float(g.abs().sum())))
    try:
        g64 = tb._oracle_grads(feats, proj, dv, P, R, torch.float64)
    finally:
        orc.LOGIT_HOOK = None
    _, gf64, gp64, gx64 = g64
    e32 = tb._f32_spread(feats, proj, dv, P, R, g64)
    gfeat = torch.stack([tr["grad_ref"]] + [tr[f"grad_src{v}"] for v in range(N - 1)]).cpu().numpy()
    gx = tr["grad_x"].permute(0, 1, 4, 2, 3).cpu().numpy()
    errs = {"features": (tb.rel_l2(gfeat, gf64.numpy()), e32["features"]),
            "x": (tb.rel_l2(gx, np.stack([g.numpy() for g in gx64])), e32["x"])}
    for k in gp64:
        if k != "cost_regularization.conv_0.bias":   # true gradient 0 (softmax over D)
            errs[k] = (tb.rel_l2(tr["param:" + k].cpu().numpy(), gp64[k].numpy()), e32[k])
    # the omega logits' bias: the common bound or half a unit roundoff of its terms' magnitude
    # sum, as test_gpu_bptt.py::test_backward_matches_float64_autograd
    kb = "omega.reweight_network.2.bias"
    ulp_sum = abs(float(tr["param:" + kb]) - float(gp64[kb])) / (2.0 ** -24 * tsum[0])
    for k, (e, c) in errs.items():
        print(f"  {k:52s} {e:.3e} {c:.3e}")
    bad = {k: e for k, e in errs.items() if not (e[0] <= tb.bound(k, e[1]) or (k == kb and ulp_sum <= 0.5))}
    assert not bad, bad


# ---------------------------------------------------------------------------------------
# 1. a call is ordered after what its stream held and before what follows
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES, ids=FRAME_IDS)
@pytest.mark.parametrize("sched", list(sc.SCHEDULES))
def test_eval_sweep_is_ordered_on_its_stream(monkeypatch, streams, sched, frame):
    """On a side stream: a delay, the producers' copies of the true inputs into the poisoned
    buffers, the sweep in three d_range pieces (workspace last used by the poison scene; depth,
    cost_out, refinement, posterior statistics), clones, the poison written back.  A library or
    aux stream that forks early reads poison (so does a d_begin == 0 initialisation that runs
    early); one still reading after the call's return sees the poison written behind it."""
    overlap = sc.set_schedule(monkeypatch, sched)
    scene = sc.Scene(frame, seed=21, poison_seed=22)
    sw, _ = sc.make_sweep(6, overlap=overlap)
    gen = lambda res: sc.eval_steps(sw, scene, res)   # noqa: E731
    scene.fill("true")
    want, dt = _serial(gen)
    scene.fill("poison")
    want_poison, _ = sc.timed_serial(gen)   # leaves the workspace used and the buffers poisoned
    assert sc.differs(want_poison, want)
    ms = sc.delay_ms(dt)
    s = streams["s"]
    s.wait_stream(torch.cuda.current_stream())
    res = {}
    t0 = time.perf_counter()
    with torch.cuda.stream(s):
        ev = sc.delay(s, ms)
        scene.fill("true")
        sc.run(sc.eval_steps(sw, scene, res))
        scene.fill("poison")
    pending = sc.still_pending(ev)
    host = time.perf_counter() - t0
    sc.note(f"eval_ordered[{sched},{FRAME_IDS[FRAMES.index(frame)]}]", serial_enqueue_ms=dt * 1e3, delay_ms=ms,
            enqueue_behind_delay_ms=host * 1e3, precondition_held=pending, actual_delay_ms=sc.actual_ms(ev))
    sc.require_pending(ev, "eval sweep behind a delay", serial_enqueue_ms=dt * 1e3, delay_ms=ms, host_ms=host * 1e3)
    torch.cuda.synchronize()
    sc.same_bits(sc.tensors(res), want, f"eval sweep on a side stream ({sched})")


@pytest.mark.parametrize("sched,pipe,frame", [("small", None, FRAMES[0]), ("small", "0", FRAMES[0]),
                                              ("large", None, FRAMES[0]), ("large", "0", FRAMES[0]),
                                              ("small", None, FRAMES[1]), ("large", None, FRAMES[1])])
def test_training_step_is_ordered_on_its_stream(monkeypatch, streams, sched, pipe, frame):
    """The same for a training step: the recorded forward into a record that last held the poison
    scene, dL/dcost produced late on the stream, the backward with grad_x (default
    AARMVS_BWD_PIPE and 0), the poison written back behind it.  Every gradient bit-equal."""
    sc.set_schedule(monkeypatch, sched)
    if pipe is None:
        monkeypatch.delenv("AARMVS_BWD_PIPE", raising=False)
    else:
        monkeypatch.setenv("AARMVS_BWD_PIPE", pipe)
    B, N, H, W, D = frame
    scene = sc.Scene(frame, seed=23, poison_seed=24)
    sw, _ = sc.make_sweep(6)
    rec = sw.record_buffers(B, H, W, D, DEV, nsrc=N - 1)
    gen = lambda res: sc.train_steps(sw, scene, rec, res)   # noqa: E731
    scene.fill("true")
    want, dt = _serial(gen)
    scene.fill("poison")
    want_poison, _ = sc.timed_serial(gen)
    assert sc.differs(want_poison, want)
    ms = sc.delay_ms(dt)
    s = streams["s"]
    s.wait_stream(torch.cuda.current_stream())
    res = {}
    t0 = time.perf_counter()
    with torch.cuda.stream(s):
        ev = sc.delay(s, ms)
        scene.fill("true")
        sc.run(sc.train_steps(sw, scene, rec, res))
        scene.fill("poison")
    pending = sc.still_pending(ev)
    host = time.perf_counter() - t0
    sc.note(f"train_ordered[{sched},pipe={pipe},{FRAME_IDS[FRAMES.index(frame)]}]", serial_enqueue_ms=dt * 1e3,
            delay_ms=ms, enqueue_behind_delay_ms=host * 1e3, precondition_held=pending, actual_delay_ms=sc.actual_ms(ev))
    sc.require_pending(ev, "training step behind a delay", serial_enqueue_ms=dt * 1e3, delay_ms=ms,
                       host_ms=host * 1e3)
    torch.cuda.synchronize()
    sc.same_bits(sc.tensors(res), want, f"training step on a side stream ({sched}, pipe {pipe})")


def _stream_not_held_back_by(s, candidates, ms=5.0):
    """The first of ``candidates`` whose pending work does not hold ``s`` back.  A process has a
    fixed number of hardware queues (four here) and streams beyond that share them: work on one
    stream then also waits for what its queue partner holds.  One probe per candidate: a short
    delay on it, an event on ``s``; ``s`` is independent if its event completes first."""
    for name, p in candidates:
        ev = sc.delay(p, ms)
        mark = torch.cuda.Event()
        mark.record(s)
        mark.synchronize()
        free = not ev.query()
        torch.cuda.synchronize()
        if free:
            return name, p
    pytest.fail("every candidate producer stream shares a hardware queue with the sweep's stream: "
                f"{[n for n, _ in candidates]}")


def test_control_a_missing_wait_shows_the_poison(monkeypatch, streams):
    """The set-up can see a missing wait: the producers' copies go behind the delay on another
    stream that the sweep's stream does not wait for, so the sweep runs at once on the poisoned
    inputs.  Its outputs are the poison scene's serial outputs bit for bit, and not the true
    scene's.  On the one-stream schedule, so that the sweep's stream is the only one that has to
    be independent of the producer's: the process has four hardware queues, and a stream that
    shares one with the delayed producer waits for it.  Measured with seven candidate producer
    streams (profiles/stream_reentrancy.txt): under the small- and the large-frame plan two left
    the sweep alone (the poison's bits), one shared the caller's queue (the sweep ran after the
    copies: the true bits) and four shared a library stream's queue, whose units then ran after
    the copies: bits of neither scene.  Which producer is harmless depends on how the library's
    streams map to queues, which cannot be seen from here; on one stream six of seven are, and
    the one used is probed.  The delay has a floor of 100 ms because the whole sweep, not only
    its enqueue, has to end inside it."""
    overlap = sc.set_schedule(monkeypatch, "one-stream")
    scene = sc.Scene(FRAMES[0], seed=21, poison_seed=22)
    sw, _ = sc.make_sweep(6, overlap=overlap)
    gen = lambda res: sc.eval_steps(sw, scene, res)   # noqa: E731
    scene.fill("true")
    want, dt = _serial(gen)
    scene.fill("poison")
    want_poison, _ = sc.timed_serial(gen)
    assert sc.differs(want_poison, want)
    ms = max(sc.delay_ms(dt), 100.0)   # the sweep itself has to end inside it
    s = streams["s"]
    pname, p = _stream_not_held_back_by(s, [(k, streams[k]) for k in ("p", "a", "b")])
    for st in (s, p):
        st.wait_stream(torch.cuda.current_stream())
    res = {}
    with torch.cuda.stream(p):
        ev = sc.delay(p, ms)
        scene.fill("true")
    with torch.cuda.stream(s):
        sc.run(sc.eval_steps(sw, scene, res))
        done = torch.cuda.Event()
        done.record(s)
    done.synchronize()
    pending = sc.still_pending(ev)
    sc.note("control[one-stream]", serial_enqueue_ms=dt * 1e3, delay_ms=ms, producer_stream=pname,
            producer_still_pending_after_sweep=pending)
    sc.require_pending(ev, "control: the sweep has to end while the producer is still delayed",
                       serial_enqueue_ms=dt * 1e3, delay_ms=ms)
    p.synchronize()   # before the buffers are reused
    torch.cuda.synchronize()
    sc.same_bits(sc.tensors(res), want_poison, "control (the poison scene's outputs)")
    assert sc.differs(sc.tensors(res), want)


# ---------------------------------------------------------------------------------------
# 3. two sweeps in flight on two caller streams, one host thread
# ---------------------------------------------------------------------------------------
def _two_callers(streams, gen_a, gen_b, ms, what):
    """Both callers' steps, interleaved on the host, each behind its own delay on its own
    stream; returns the device intervals (start, end) of A and of B in ms after a common event."""
    sa, sb = streams["a"], streams["b"]
    cur = torch.cuda.current_stream()
    t0 = torch.cuda.Event(enable_timing=True)
    t0.record(cur)
    for st in (sa, sb):
        st.wait_stream(cur)
    marks = {k: torch.cuda.Event(enable_timing=True) for k in ("a0", "a1", "b0", "b1")}
    h0 = time.perf_counter()
    ev_a = sc.delay(sa, ms)
    ev_b = sc.delay(sb, ms)
    marks["a0"].record(sa)
    marks["b0"].record(sb)
    order = [who for who, _ in sc.interleave(on_stream(sa, gen_a), on_stream(sb, gen_b))]
    marks["a1"].record(sa)
    marks["b1"].record(sb)
    pend_a, pend_b = sc.still_pending(ev_a), sc.still_pending(ev_b)
    host = time.perf_counter() - h0
    assert order[:4] == [0, 1, 0, 1], order
    for ev, who in ((ev_a, "A"), (ev_b, "B")):
        sc.require_pending(ev, f"{what}: caller {who}", delay_ms=ms, host_ms=host * 1e3)
    torch.cuda.synchronize()
    t = {k: t0.elapsed_time(m) for k, m in marks.items()}
    sc.note(what, delay_ms=ms, enqueue_behind_delay_ms=host * 1e3, precondition_held=pend_a and pend_b,
            actual_delay_ms=min(sc.actual_ms(ev_a), sc.actual_ms(ev_b)), A_start_ms=t["a0"], A_end_ms=t["a1"],
            B_start_ms=t["b0"], B_end_ms=t["b1"])
    return t


@pytest.mark.parametrize("sched", ["small", "large"])
def test_two_sweeps_in_flight_on_two_streams(monkeypatch, streams, sched):
    """Two DepthSweep objects (other weights, other frames; A split precision with refinement and
    posterior statistics, B fp16), their d_range pieces interleaved on the host: one thread's
    single event set and the shared library streams serve both alternately.  Every output equals
    its serial run, and the two sweeps' device intervals overlap."""
    sc.set_schedule(monkeypatch, sched)
    sca, scb = sc.Scene(FRAMES[0], seed=31, poison_seed=32), sc.Scene(FRAMES[1], seed=33, poison_seed=34)
    swa, _ = sc.make_sweep(6)
    swb, _ = sc.make_sweep(7, precision="fp16")
    gen_a = lambda res: sc.eval_steps(swa, sca, res, extras=True)    # noqa: E731
    gen_b = lambda res: sc.eval_steps(swb, scb, res, extras=False)   # noqa: E731
    sca.fill("true")
    scb.fill("true")
    want_a, dt_a = _serial(gen_a)
    want_b, dt_b = _serial(gen_b)
    ms = sc.delay_ms(dt_a + dt_b)
    res_a, res_b = {}, {}
    what = f"two_sweeps[{sched}]"
    sc.note(what + " serial", A_enqueue_ms=dt_a * 1e3, B_enqueue_ms=dt_b * 1e3)
    t = _two_callers(streams, gen_a(res_a), gen_b(res_b), ms, what)
    sc.same_bits(sc.tensors(res_a), want_a, "sweep A beside sweep B")
    sc.same_bits(sc.tensors(res_b), want_b, "sweep B beside sweep A")
    assert t["a0"] < t["b1"] and t["b0"] < t["a1"], f"the sweeps did not overlap on the device: {t}"


@pytest.mark.parametrize("sched", ["small", "large"])
def test_training_step_beside_an_eval_sweep(monkeypatch, streams, sched):
    """A's recorded forward and backward on one stream, B's eval sweep on another, interleaved on
    the host: the sweep's units and the backward share library streams 1 and 2.  A's gradients
    (every parameter, dL/dref, dL/dsrc, grad_x) and B's outputs equal their serial runs."""
    sc.set_schedule(monkeypatch, sched)
    monkeypatch.delenv("AARMVS_BWD_PIPE", raising=False)
    B, N, H, W, D = FRAMES[0]
    sca, scb = sc.Scene(FRAMES[0], seed=35, poison_seed=36), sc.Scene(FRAMES[1], seed=37, poison_seed=38)
    swa, _ = sc.make_sweep(6)
    swb, _ = sc.make_sweep(7)
    rec = swa.record_buffers(B, H, W, D, DEV, nsrc=N - 1)
    gen_a = lambda res: sc.train_steps(swa, sca, rec, res)   # noqa: E731
    gen_b = lambda res: sc.eval_steps(swb, scb, res)         # noqa: E731
    sca.fill("true")
    scb.fill("true")
    want_a, dt_a = _serial(gen_a)
    want_b, dt_b = _serial(gen_b)
    ms = sc.delay_ms(dt_a + dt_b)
    res_a, res_b = {}, {}
    what = f"train_beside_eval[{sched}]"
    sc.note(what + " serial", A_enqueue_ms=dt_a * 1e3, B_enqueue_ms=dt_b * 1e3)
    _two_callers(streams, gen_a(res_a), gen_b(res_b), ms, what)
    sc.same_bits(sc.tensors(res_a), want_a, "training step beside an eval sweep")
    sc.same_bits(sc.tensors(res_b), want_b, "eval sweep beside a training step")


# ---------------------------------------------------------------------------------------
# 4. two host threads
# ---------------------------------------------------------------------------------------
def _rejected_call(**over):
    """A sweep call the argument checks reject before any launch; returns (code, last error)."""
    from aarmvs import _lib, lib
    a = _lib.SweepArgs()
    a.B, a.C, a.H, a.W, a.nsrc, a.D = 1, 32, 8, 8, 1, 4
    a.d_begin, a.d_end = 0, 4
    a.ref_fea = a.rel_proj = a.depth_values = a.packed_params = a.workspace = 0x1000   # never dereferenced
    a.src_fea[0] = 0x1000
    for k, v in over.items():
        setattr(a, k, v)
    rc = lib().aarmvs_sweep(ctypes.byref(a), None)
    return rc, lib().aarmvs_last_error().decode()


@pytest.mark.parametrize("sched", ["small", "large"])
def test_two_host_threads(monkeypatch, streams, sched):
    """Two threads, each with its stream, DepthSweep and inputs, released together: ctypes drops
    the GIL inside each library call, so the two enqueue loops interleave launch by launch, each
    thread with its own event set.  Three whole sweeps each (one call over the three plane
    groups), thread 0 also a training step; thread 1 makes a rejected call in between.  Every
    output equals its serial run and each thread reads only its own error text."""
    from aarmvs import lib
    sc.set_schedule(monkeypatch, sched)
    monkeypatch.delenv("AARMVS_BWD_PIPE", raising=False)
    whole = [(0, FRAMES[0][4])]
    scenes = [sc.Scene(FRAMES[0], seed=41, poison_seed=42), sc.Scene(FRAMES[1], seed=43, poison_seed=44)]
    sweeps = [sc.make_sweep(6)[0], sc.make_sweep(7)[0]]
    B, N, H, W, D = FRAMES[0]
    rec = sweeps[0].record_buffers(B, H, W, D, DEV, nsrc=N - 1)
    for s_ in scenes:
        s_.fill("true")
    t0 = time.perf_counter()
    want = [_serial(lambda res, i=i: sc.eval_steps(sweeps[i], scenes[i], res, pieces=whole))[0] for i in (0, 1)]
    want_train = _serial(lambda res: sc.train_steps(sweeps[0], scenes[0], rec, res))[0]
    serial_s = time.perf_counter() - t0   # (two runs of everything, synchronised)
    cur = torch.cuda.current_stream()
    mine = [streams["a"], streams["b"]]
    for st in mine:
        st.wait_stream(cur)
    barrier = threading.Barrier(2)
    got = [{"sweeps": [], "errors": []}, {"sweeps": [], "errors": []}]

    def work(i):
        out = got[i]
        try:
            if i == 0:   # an error text of this thread's own, set before the other thread's
                out["rc0"], out["err_before"] = _rejected_call(C=16)
            barrier.wait(timeout=60)
            with torch.cuda.stream(mine[i]):
                for it in range(3):
                    res = {}
                    sc.run(sc.eval_steps(sweeps[i], scenes[i], res, pieces=whole))
                    out["sweeps"].append(res)
                    if i == 1 and it == 1:
                        out["rc1"], out["err_mid"] = _rejected_call(H=6)
                if i == 0:
                    out["train"] = {}
                    sc.run(sc.train_steps(sweeps[0], scenes[0], rec, out["train"]))
                mine[i].synchronize()
            out["err_after"] = lib().aarmvs_last_error().decode()
        except BaseException as e:   # reported in the main thread
            out["errors"].append(repr(e))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in (0, 1)]
    limit = max(30.0, 20.0 * serial_s)
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, limit - (time.perf_counter() - t0)))
    if any(t.is_alive() for t in threads):
        pytest.exit(f"test_two_host_threads[{sched}]: a thread is still running after {limit:.0f} s "
                    f"(serial time {serial_s:.2f} s): hung; no further GPU tests", returncode=3)
    torch.cuda.synchronize()
    sc.note(f"two_threads[{sched}]", serial_s=serial_s, threads_s=time.perf_counter() - t0, join_limit_s=limit)
    assert not got[0]["errors"] and not got[1]["errors"], (got[0]["errors"], got[1]["errors"])
    for i in (0, 1):
        assert len(got[i]["sweeps"]) == 3
        for it, res in enumerate(got[i]["sweeps"]):
            sc.same_bits(sc.tensors(res), want[i], f"thread {i}, sweep {it}")
    sc.same_bits(sc.tensors(got[0]["train"]), want_train, "thread 0, training step")
    assert got[0]["rc0"] == 1 and got[0]["err_before"] == "sweep: feature channels C must be 32"
    assert got[0]["err_after"] == got[0]["err_before"]
    assert got[1]["rc1"] == 1 and "multiples of 4" in got[1]["err_mid"]
    assert got[1]["err_after"] == got[1]["err_mid"]


# ---------------------------------------------------------------------------------------
# 5. one DepthSweep across a geometry change while its last sweep is in flight
# ---------------------------------------------------------------------------------------
def test_geometry_change_while_the_last_sweep_is_in_flight(streams):
    """The workspace (and the refine / posterior state) of geometry 1 is allocated under the
    default stream, used by a sweep queued behind a delay on a side stream, and dropped by the
    geometry-2 sweep that follows it through the same object.  A default-stream allocation of the
    same size must not get the block while that sweep is queued: both sweeps equal their serial
    runs, and the new tensors still hold what the default stream wrote (0x5A).  Without
    DepthSweep's record_stream the caching allocator hands the dropped block out at once."""
    from aarmvs import lib
    sc1, sc2 = sc.Scene(FRAMES[0], seed=51, poison_seed=52), sc.Scene(FRAMES[1], seed=53, poison_seed=54)
    sw, _ = sc.make_sweep(6)
    gen1 = lambda res: sc.eval_steps(sw, sc1, res)   # noqa: E731
    gen2 = lambda res: sc.eval_steps(sw, sc2, res)   # noqa: E731
    sc1.fill("true")
    sc2.fill("true")
    want1, dt1 = _serial(gen1)
    want2, dt2 = _serial(gen2)
    s = streams["s"]
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # both sweeps once under the side stream: its allocator pool holds their blocks,
        sc.run(sc.eval_steps(sw, sc1, {}))   # so that the enqueue below does not wait for the driver's allocations
        sc.run(sc.eval_steps(sw, sc2, {}))
    torch.cuda.synchronize()
    sc.timed_serial(gen1)   # the first call at geometry 1: its buffers are allocated here, on the default stream
    B, N, H, W, D = FRAMES[0]
    sizes = [lib().aarmvs_sweep_workspace_bytes(B, H, W, N - 1), 16 * B * H * W, 16 * B * H * W]
    # (the sequence below also allocates: geometry 2's buffers under the side stream and, once the
    # dropped blocks are held back, fresh ones for the default stream -- up to 14 ms of host time
    # where the two serial enqueues take 4 -- so the delay gets a floor of 100 ms instead of 20)
    ms = max(sc.delay_ms(dt1 + dt2), 100.0)
    s.wait_stream(torch.cuda.current_stream())
    res1, res2 = {}, {}
    t0 = time.perf_counter()
    with torch.cuda.stream(s):
        ev = sc.delay(s, ms)
        sc.run(sc.eval_steps(sw, sc1, res1))
        sc.run(sc.eval_steps(sw, sc2, res2))   # drops geometry 1's buffers while sweep 1 is queued
    grabbed = [torch.empty(n, dtype=torch.uint8, device=DEV).fill_(0x5A) for n in sizes]   # default stream
    pending = sc.still_pending(ev)
    host = time.perf_counter() - t0
    sc.note("geometry_change", serial_enqueue_ms=(dt1 + dt2) * 1e3, delay_ms=ms, enqueue_behind_delay_ms=host * 1e3,
            precondition_held=pending, actual_delay_ms=sc.actual_ms(ev))
    sc.require_pending(ev, "geometry change", serial_enqueue_ms=(dt1 + dt2) * 1e3, delay_ms=ms, host_ms=host * 1e3)
    torch.cuda.synchronize()
    sc.same_bits(sc.tensors(res1), want1, "geometry 1's sweep, its buffers dropped while queued")
    sc.same_bits(sc.tensors(res2), want2, "geometry 2's sweep")
    for n, g in zip(sizes, grabbed):
        assert bool((g == 0x5A).all()), f"a {n} B default-stream tensor was written by the queued sweep"


# ---------------------------------------------------------------------------------------
# 2. the standalone entry points launch on the stream they are given
# ---------------------------------------------------------------------------------------
def _rnd(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _rolled(t):
    """The default poison of an input: its own values, one element on (valid wherever the true
    tensor is: the same value set)."""
    return t.flatten().roll(1).view_as(t).contiguous()


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _rels(B, H, W):
    """Relative projections [B,3,4] of source views 1 and 2 of the synthetic cameras."""
    from aarmvs import ops, synthetic as syn
    proj = torch.from_numpy(np.broadcast_to(syn.camera_projections(3, H, W), (B, 3, 4, 4)).copy())
    return [ops.relative_projection(proj[:, v], proj[:, 0]).to(DEV) for v in (1, 2)]


def _depth_list(B, D, descending=False):
    from aarmvs import synthetic as syn
    dv = syn.depth_hypotheses(D, descending=descending)
    return torch.from_numpy(np.broadcast_to(dv, (B, D)).copy()).to(DEV)


class Op:
    """One table row: the true inputs (device tensors), the poison of those that need their own
    (the others get ``_rolled``), the call (inputs -> {name: output tensor}), whether it
    synchronises the host inside, and the outputs compared in relative L2 instead of bit for
    bit (fp32 atomics), with their bound."""

    def __init__(self, inputs, call, poison=None, host_sync=False, loose=None):
        self.inputs, self.call, self.host_sync, self.loose = inputs, call, host_sync, loose or {}
        self.poison = {k: (poison or {}).get(k, None) for k in inputs}
        for k, v in self.poison.items():
            if v is None:
                self.poison[k] = _rolled(inputs[k])


def _op_homo_warp():
    from aarmvs import ops
    B, C, H, W = 2, 32, 16, 24
    r1, r2 = _rels(B, H, W)
    inp = {"src": _rnd(1, B, C, H, W), "rel": r1, "depth": torch.full((B,), 600.0, device=DEV)}
    return Op(inp, lambda i: {"out": ops.homo_warp(i["src"], i["rel"], i["depth"])},
              poison={"rel": r2, "depth": torch.full((B,), 800.0, device=DEV)})


def _op_homo_warp_backward():
    from aarmvs import ops
    B, C, H, W = 2, 32, 16, 24
    r1, r2 = _rels(B, H, W)
    inp = {"g": _rnd(2, B, C, H, W), "rel": r1, "depth": torch.full((B,), 600.0, device=DEV)}
    return Op(inp, lambda i: {"grad_src": ops.homo_warp_backward(i["g"], i["rel"], i["depth"], (B, C, H, W))},
              poison={"rel": r2, "depth": torch.full((B,), 800.0, device=DEV)})


def _op_group_norm():
    from aarmvs import ops
    B, C, H, W = 2, 16, 12, 20
    inp = {"x": _rnd(3, B, C, H, W), "w": _rnd(4, C), "b": _rnd(5, C), "gy": _rnd(6, B, C, H, W)}

    def call(i):
        x, w, b = _leaf(i["x"]), _leaf(i["w"]), _leaf(i["b"])
        y = ops.group_norm(x, 8, w, b)
        dx, dw, db = torch.autograd.grad(y, (x, w, b), i["gy"])
        return {"y": y.detach(), "dx": dx, "dw": dw, "db": db}
    return Op(inp, call)


def _op_lstm_gates():
    from aarmvs import ops
    B, hid, H, W = 2, 8, 12, 20
    inp = {"z": _rnd(7, B, 4 * hid, H, W), "c": _rnd(8, B, hid, H, W), "dh": _rnd(9, B, hid, H, W),
           "dc": _rnd(10, B, hid, H, W)}

    def call(i):
        z, c = _leaf(i["z"]), _leaf(i["c"])
        h, c1 = ops.lstm_gates(z, c)
        dz, dcp = torch.autograd.grad((h, c1), (z, c), (i["dh"], i["dc"]))
        return {"h": h.detach(), "c": c1.detach(), "dz": dz, "dc_prev": dcp}
    return Op(inp, call)


def _op_softmax_depth():
    from aarmvs import ops
    return Op({"cost": _rnd(11, 2, 8, 12, 20)}, lambda i: {"p": ops.softmax_depth(i["cost"])})


def _cls_inputs(B=2, D=8, H=12, W=20):
    dv = _depth_list(B, D)
    gt = 425.0 + 510.0 * torch.rand(B, H, W, generator=torch.Generator().manual_seed(12))
    mask = (torch.rand(B, H, W, generator=torch.Generator().manual_seed(13)) > 0.3).float()
    return {"cost": _rnd(14, B, D, H, W), "gt": gt.to(DEV), "mask": mask.to(DEV), "dv": dv}, _depth_list(B, D, True)


def _op_cls_loss():
    from aarmvs import ops
    inp, dv_p = _cls_inputs()
    inp["gl"] = torch.tensor(0.75, device=DEV)

    def call(i):
        cost = _leaf(i["cost"])
        loss, wta, mp = ops.cls_loss(cost, i["gt"], i["mask"], i["dv"], True)
        (g,) = torch.autograd.grad(loss, cost, i["gl"])
        return {"loss": loss.detach(), "wta": wta, "max_prob": mp, "grad": g}
    return Op(inp, call, poison={"dv": dv_p, "gl": torch.tensor(-1.5, device=DEV)})


def _op_depth_metrics():
    from aarmvs import ops
    inp, _ = _cls_inputs()
    inp = {"est": inp["gt"] + _rnd(15, 2, 12, 20, scale=6.0), "gt": inp["gt"], "mask": inp["mask"]}
    return Op(inp, lambda i: {"m": torch.stack(list(ops.depth_metrics(i["est"], i["gt"], i["mask"]).values()))})


def _op_evidential_epilogue():
    from aarmvs import ops
    D, H, W = 32, 8, 12
    inp = {f"h{k}": _rnd(16 + k, 1, 4, D, H, W) for k in range(3)}
    inp.update(dv=_depth_list(1, D)[0].contiguous(), g_ev=_rnd(20, 4, H, W), g_pc=_rnd(21, 1, D, H, W))

    def call(i):
        hs = [_leaf(i[f"h{k}"]) for k in range(3)]
        ev, pc = ops.evidential_epilogue(*hs, i["dv"])
        gs = torch.autograd.grad((ev, pc), hs, (i["g_ev"], i["g_pc"]))
        return {"ev": ev.detach(), "pc": pc.detach(), "g0": gs[0], "g1": gs[1], "g2": gs[2]}
    return Op(inp, call, poison={"dv": _depth_list(1, D, True)[0].contiguous()})


def _op_deform_sample():
    from aarmvs import ops
    B, H, W, C = 1, 10, 14, 32
    inp = {"x": _rnd(22, B, H, W, C), "off": _rnd(23, B, 18, H, W, scale=1.5),
           "m": torch.sigmoid(_rnd(24, B, 9, H, W)), "g": _rnd(25, B, H * W, 9 * C)}

    def call(i):
        x, off, m = _leaf(i["x"]), _leaf(i["off"]), _leaf(i["m"])
        val = ops.deform_sample(x, off, m, 1, 1)
        gx, goff, gm = torch.autograd.grad(val, (x, off, m), i["g"])
        return {"val": val.detach(), "gx": gx, "goff": goff, "gm": gm}
    # dL/dx is an fp32 atomic scatter: relative L2 2e-5, the bound of tests/test_gpu_deform.py
    return Op(inp, call, loose={"gx": 2e-5})


def _wta_inputs(B=2, D=6, H=12, W=20):
    return {"cost": _rnd(26, B, D, H, W), "dv": _depth_list(B, D)}, {"dv": _depth_list(B, D, True)}


def _op_wta_update():
    from aarmvs import ops
    inp, poison = _wta_inputs()

    def call(i):
        B, D, H, W = i["cost"].shape
        mp, dm, es = (torch.zeros(B, H, W, device=DEV) for _ in range(3))
        for d in range(D):
            ops.wta_update(i["cost"][:, d].contiguous(), i["dv"][:, d], mp, dm, es)
        return {"max_prob": mp, "depth": dm, "exp_sum": es}
    return Op(inp, call, poison=poison)


def _op_wta_refine():
    from aarmvs import ops
    inp, poison = _wta_inputs()

    def call(i):
        B, D, H, W = i["cost"].shape
        mp, dm, es = (torch.zeros(B, H, W, device=DEV) for _ in range(3))
        st = ops.refine_state(B, H * W, DEV)
        for d in range(D):
            ops.wta_refine_update(i["cost"][:, d].contiguous(), d, i["dv"][:, d], mp, dm, es, st)
        out = ops.wta_refine_finalize(mp, dm, es, st, i["dv"], D)
        return {"max_prob": mp, "depth": dm, "exp_sum": es, **out}
    return Op(inp, call, poison=poison)


def _op_refine_from_cost():
    from aarmvs import ops
    inp, poison = _wta_inputs()
    return Op(inp, lambda i: dict(ops.refine_from_cost(i["cost"], i["dv"])), poison=poison)


def _op_wta_posterior():
    from aarmvs import ops
    inp, poison = _wta_inputs()

    def call(i):
        B, D, H, W = i["cost"].shape
        mp, dm, es = (torch.zeros(B, H, W, device=DEV) for _ in range(3))
        st = ops.posterior_state(B, H * W, DEV)
        for d in range(D):
            ops.wta_posterior_update(i["cost"][:, d].contiguous(), d, i["dv"][:, d], mp, dm, es, st)
        out = ops.wta_posterior_finalize(es, st)
        return {"max_prob": mp, "depth": dm, "exp_sum": es, **out}
    return Op(inp, call, poison=poison)


def _op_posterior_from_cost():
    from aarmvs import ops
    inp, poison = _wta_inputs()
    return Op(inp, lambda i: dict(ops.posterior_from_cost(i["cost"], i["dv"])), poison=poison)


def _op_cost_slice():
    from aarmvs import synthetic as syn
    B, N, H, W = 1, 3, 16, 24
    sw, _ = sc.make_sweep(2)
    proj = torch.from_numpy(np.broadcast_to(syn.camera_projections(N, H, W), (B, N, 4, 4)).copy())
    inp = {"f": _rnd(27, N, B, 32, H, W), "depth": torch.full((B,), 600.0, device=DEV)}

    def call(i):
        x, om = sw.cost_slice(i["f"][0], [i["f"][1], i["f"][2]], proj[:, 0], [proj[:, 1], proj[:, 2]], i["depth"],
                              want_omega=True)
        return {"x": x, "omega": om}
    # (cost_slice forms the relative projections on the host and copies them over with a blocking
    # .to(device), DepthSweep.relative: a host wait for the stream inside the call, measured 20 ms
    # behind a 20 ms delay)
    return Op(inp, call, poison={"depth": torch.full((B,), 800.0, device=DEV)}, host_sync=True)


def _op_unet_step():
    sw, _ = sc.make_sweep(2)
    inp = {"x": _rnd(28, 1, 32, 16, 24)}
    return Op(inp, lambda i: {"c0": sw.unet_step(i["x"], 0), "c1": sw.unet_step(i["x"], 1)})


def _fusion_inputs(H=24, W=32, nsrc=2):
    from aarmvs import synthetic as syn
    depths, cams, conf = syn.fusion_views(H, W, nsrc, seed=3)
    pd, _, pconf = syn.fusion_views(H, W, nsrc, seed=4)
    inp = {f"d{v}": torch.from_numpy(d).to(DEV) for v, d in enumerate(depths)}
    inp["conf"] = torch.from_numpy(conf).to(DEV)
    poison = {f"d{v}": torch.from_numpy(d).to(DEV) for v, d in enumerate(pd)}
    poison["conf"] = torch.from_numpy(pconf).to(DEV)
    return inp, poison, cams, nsrc


def _op_fusion_filter():
    from aarmvs import fusion
    inp, poison, cams, nsrc = _fusion_inputs()

    def call(i):
        photo, geo, final, avg = fusion.filter_depth_core(i["d0"], i["conf"], cams[0], [i[f"d{v}"] for v in range(1, nsrc + 1)],
                                                          cams[1:], 0.35)
        return {"photo": photo, "geo": geo, "final": final, "avg": avg}
    return Op(inp, call, poison=poison)


def _op_fusion_filter_dedup():
    from aarmvs import fusion
    inp, poison, cams, nsrc = _fusion_inputs()
    H, W = inp["d0"].shape
    inp["used"] = (torch.rand(H, W, generator=torch.Generator().manual_seed(5)) < 0.3).to(torch.uint8).to(DEV)

    def call(i):
        used_srcs = [torch.zeros(H, W, dtype=torch.uint8, device=DEV) for _ in range(nsrc)]
        photo, geo, final, emit, avg = fusion.filter_depth_dedup(
            i["d0"], i["conf"], cams[0], [i[f"d{v}"] for v in range(1, nsrc + 1)], cams[1:], 0.35, i["used"], used_srcs)
        return {"photo": photo, "geo": geo, "final": final, "emit": emit, "avg": avg,
                **{f"used{v}": u for v, u in enumerate(used_srcs)}}
    return Op(inp, call, poison=poison)


def _op_pyr_down():
    from aarmvs import fusion
    return Op({"img": _rnd(29, 21, 30, 3, scale=60.0)}, lambda i: {"out": fusion.pyr_down(i["img"])})


def _points_inputs(H=24, W=32):
    from aarmvs import synthetic as syn
    depths, cams, _ = syn.fusion_views(H, W, 1, seed=6)
    pd, _, _ = syn.fusion_views(H, W, 1, seed=7)
    mask = (torch.rand(H, W, generator=torch.Generator().manual_seed(8)) < 0.6).to(torch.uint8)
    inp = {"avg": torch.from_numpy(depths[0]).double().to(DEV), "mask": mask.to(DEV), "img": _rnd(30, H, W, 3, scale=80.0)}
    return inp, {"avg": torch.from_numpy(pd[0]).double().to(DEV)}, cams[0]


def _op_fusion_points():
    from aarmvs import fusion
    inp, poison, cam = _points_inputs()
    H, W = inp["avg"].shape

    def call(i):
        xyz = torch.zeros(H * W, 3, device=DEV)
        rgb = torch.zeros(H * W, 3, dtype=torch.uint8, device=DEV)
        count = fusion.fuse_points_into(i["avg"], i["mask"], cam, i["img"], xyz, rgb)
        return {"xyz": xyz, "rgb": rgb, "count": count}
    return Op(inp, call, poison=poison)


def _op_fusion_normals():
    from aarmvs import fusion
    inp, poison, cam = _points_inputs()
    del inp["img"]

    def call(i):
        normal, has = fusion.estimate_normals(i["avg"], i["mask"], cam)
        H, W = i["avg"].shape
        xyz, nrm = torch.zeros(H * W, 3, device=DEV), torch.zeros(H * W, 3, device=DEV)
        count = fusion.fuse_points_into(i["avg"], i["mask"], cam, None, xyz, None, normal_map=normal, nrm=nrm)
        return {"normal": normal, "has": has, "xyz": xyz, "nrm": nrm, "count": count}
    return Op(inp, call, poison=poison)


ORIGIN, CELL = (-2.0, -2.0, -2.0), 0.25


def _cloud(seed, n):
    return (torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 3.0 - 1.5).to(DEV)


def _op_cloud_keys():
    from aarmvs import cloud_eval
    return Op({"xyz": _cloud(31, 700)}, lambda i: {"keys": cloud_eval.cloud_keys(i["xyz"], ORIGIN, CELL)},
              poison={"xyz": _cloud(32, 700)})


def _op_nn_sorted():
    """A key-sorted target and its poison, another key-sorted cloud of the same size: the kernel
    searches the keys, so both must be sorted."""
    from aarmvs import cloud_eval

    def target(seed):
        t, keys, perm = cloud_eval._sorted_by_key(_cloud(seed, 900), ORIGIN, CELL)
        return {"t": t, "keys": keys, "ids": perm.to(torch.int32).contiguous()}
    inp, poison = target(33), target(34)
    inp["q"], poison["q"] = _cloud(35, 500), _cloud(36, 500)

    def call(i):
        dist, index = cloud_eval.nn_sorted(i["q"], i["t"], i["keys"], i["ids"], ORIGIN, CELL, 0.5)
        return {"dist": dist, "index": index}
    return Op(inp, call, poison=poison)


def _op_distance_stats():
    from aarmvs import cloud_eval
    inp = {"dist": torch.rand(3000, generator=torch.Generator().manual_seed(37)).to(DEV)}
    return Op(inp, lambda i: {"stats": torch.tensor(cloud_eval.distance_stats(i["dist"], (0.25, 0.5)), dtype=torch.float64)},
              host_sync=True)


def _op_voxel_downsample():
    from aarmvs import cloud_eval
    return Op({"xyz": _cloud(38, 2000)}, lambda i: {"out": cloud_eval.voxel_downsample(i["xyz"], 0.3)},
              poison={"xyz": _cloud(39, 2000)}, host_sync=True)


OPS = {f.__name__[4:]: f for f in (
    _op_homo_warp, _op_homo_warp_backward, _op_group_norm, _op_lstm_gates, _op_softmax_depth, _op_cls_loss,
    _op_depth_metrics, _op_evidential_epilogue, _op_deform_sample, _op_wta_update, _op_wta_refine,
    _op_refine_from_cost, _op_wta_posterior, _op_posterior_from_cost, _op_cost_slice, _op_unet_step,
    _op_fusion_filter, _op_fusion_filter_dedup, _op_pyr_down, _op_fusion_points, _op_fusion_normals,
    _op_cloud_keys, _op_nn_sorted, _op_distance_stats, _op_voxel_downsample)}


@pytest.mark.parametrize("name", list(OPS))
def test_standalone_op_runs_on_the_stream_it_is_given(streams, name):
    """Every op that launches on torch.cuda.current_stream(), under a side stream: its inputs are
    produced behind a delay from poisoned buffers, its result is consumed on the stream, and the
    poison is written back behind it.  An op that launched on stream 0 (or on any stream that
    does not wait for the caller's) would read the poison.  Bit-equal to its own default-stream
    result; the fp32-atomic outputs within their existing bound.  (Forward and backward of the
    autograd ops: the engine runs a node's backward on its forward's stream.)"""
    op = OPS[name]()
    bufs = {k: v.clone() for k, v in op.inputs.items()}
    torch.cuda.synchronize()
    op.call(bufs)                         # warm (code object load, allocations)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = op.call(bufs)
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in want.items()}
    for k, v in op.poison.items():
        assert v.shape == bufs[k].shape and v.dtype == bufs[k].dtype and not torch.equal(v, op.inputs[k]), k
        bufs[k].copy_(v)
    torch.cuda.synchronize()
    ms = sc.delay_ms(dt)
    s = streams["s"]
    s.wait_stream(torch.cuda.current_stream())
    t0 = time.perf_counter()
    with torch.cuda.stream(s):
        ev = sc.delay(s, ms)
        for k, v in op.inputs.items():
            bufs[k].copy_(v, non_blocking=True)
        if op.host_sync:   # the op waits for the device inside: the precondition holds before it
            sc.require_pending(ev, f"{name} (before the call)", serial_call_ms=dt * 1e3, delay_ms=ms)
        got = {k: v.clone() for k, v in op.call(bufs).items()}
        for k, v in op.poison.items():
            bufs[k].copy_(v, non_blocking=True)
    pending = op.host_sync or sc.still_pending(ev)
    host = time.perf_counter() - t0
    sc.note(f"op[{name}]", serial_call_ms=dt * 1e3, delay_ms=ms, enqueue_behind_delay_ms=host * 1e3,
            precondition_held=pending, host_sync=op.host_sync, actual_delay_ms=sc.actual_ms(ev))
    if not op.host_sync:
        sc.require_pending(ev, name, serial_call_ms=dt * 1e3, delay_ms=ms, host_ms=host * 1e3)
    torch.cuda.synchronize()
    exact = {k: v for k, v in want.items() if k not in op.loose}
    sc.same_bits(got, exact, f"{name} on a side stream")
    for k, tol in op.loose.items():
        err = float((got[k].double() - want[k].double()).norm() / want[k].double().norm().clamp_min(1e-30))
        assert err <= tol, f"{name}: {k} relative L2 {err:.3e} > {tol:.1e}"
