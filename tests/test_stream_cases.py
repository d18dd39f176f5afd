"""The stream and thread contract without a device: aarmvs_last_error is per thread, the
helpers of tests/test_gpu_streams.py size a delay and interleave two callers as documented, and
the CPU model of the sweep's schedule (tests/sweep_schedule_check.cpp, run by
tests/test_sweep_schedule.py) covers two sweeps that share the library streams and one event
set.  Every library call here is rejected by the argument checks, before any launch."""
import ctypes
import threading

import pytest

import stream_cases as sc

FAKE = 0x1000   # never dereferenced: validation fails first
INVALID = 1


def _args(**over):
    from aarmvs import _lib
    a = _lib.SweepArgs()
    a.B, a.C, a.H, a.W, a.nsrc, a.D = 1, 32, 8, 8, 1, 4
    a.d_begin, a.d_end = 0, 4
    a.ref_fea = a.rel_proj = a.depth_values = a.packed_params = a.workspace = FAKE
    a.src_fea[0] = FAKE
    for k, v in over.items():
        setattr(a, k, v)
    return a


# four calls the sweep rejects before touching the device, and what each leaves in last_error
REJECTED = [({"ref_fea": None}, "sweep: null pointer argument"),
            ({"C": 16}, "sweep: feature channels C must be 32"),
            ({"d_end": 5}, "sweep: need 0 <= d_begin < d_end <= D"),
            ({"H": 6}, "multiples of 4")]


def test_last_error_is_per_thread():
    """Four threads, each provoking its own rejection 200 times behind one barrier: a thread only
    ever reads its own message (ctypes drops the GIL inside the call, so the calls interleave)."""
    from aarmvs import lib
    L = lib()
    barrier = threading.Barrier(len(REJECTED))
    seen = [set() for _ in REJECTED]
    errors = []

    def work(i):
        try:
            a = _args(**REJECTED[i][0])
            barrier.wait(timeout=30)
            for _ in range(200):
                assert L.aarmvs_sweep(ctypes.byref(a), None) == INVALID
                seen[i].add(L.aarmvs_last_error().decode())
        except BaseException as e:   # reported in the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(REJECTED))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors
    for i, (_, text) in enumerate(REJECTED):
        assert len(seen[i]) == 1 and text in next(iter(seen[i])), (i, seen[i])
    assert len({next(iter(s)) for s in seen}) == len(REJECTED)


def test_last_error_of_another_thread_is_not_visible():
    """A thread that never failed reads an empty message while the main thread holds one, and the
    main thread's text survives the other thread's failure."""
    from aarmvs import lib
    L = lib()
    a = _args(C=16)
    assert L.aarmvs_sweep(ctypes.byref(a), None) == INVALID
    mine = L.aarmvs_last_error().decode()
    got = {}

    def work():
        got["before"] = L.aarmvs_last_error().decode()
        b = _args(H=6)
        got["rc"] = L.aarmvs_sweep(ctypes.byref(b), None)
        got["after"] = L.aarmvs_last_error().decode()

    t = threading.Thread(target=work, daemon=True)
    t.start()
    t.join(60)
    assert not t.is_alive()
    assert got["before"] == "" and got["rc"] == INVALID and "multiples of 4" in got["after"]
    assert L.aarmvs_last_error().decode() == mine == "sweep: feature channels C must be 32"


@pytest.mark.parametrize("seconds,ms", [(0.0, 20.0), (0.001, 20.0), (0.005, 20.0), (0.00501, 20.04), (0.010, 40.0),
                                        (0.0375, 150.0), (0.075, 300.0), (0.0751, 300.0), (2.0, 300.0)])
def test_delay_is_four_times_the_enqueue_time_within_its_limits(seconds, ms):
    assert sc.delay_ms(seconds) == pytest.approx(ms, rel=1e-12)
    assert sc.DELAY_MIN_MS <= sc.delay_ms(seconds) <= sc.DELAY_MAX_MS


def test_delay_rejects_a_time_that_is_not_one():
    for bad in (-1e-3, float("nan")):
        with pytest.raises(ValueError):
            sc.delay_ms(bad)


def test_interleave_alternates_and_keeps_each_order():
    a, b = sc.PIECES, sc.PIECES
    assert list(sc.interleave(a, b)) == [(0, (0, 16)), (1, (0, 16)), (0, (16, 32)), (1, (16, 32)),
                                         (0, (32, 40)), (1, (32, 40))]
    # unequal lengths: the longer one goes on alone, in order
    assert list(sc.interleave("ab", "wxyz")) == [(0, "a"), (1, "w"), (0, "b"), (1, "x"), (1, "y"), (1, "z")]
    assert list(sc.interleave("abc", "")) == [(0, "a"), (0, "b"), (0, "c")]
    assert list(sc.interleave()) == []
    # generators are advanced one step at a time, never ahead of their turn
    log = []

    def gen(tag, n):
        for i in range(n):
            log.append((tag, i))
            yield i

    for _ in sc.interleave(gen("A", 3), gen("B", 2)):
        pass
    assert log == [("A", 0), ("B", 0), ("A", 1), ("B", 1), ("A", 2)]


def test_pieces_and_frames_are_the_ones_the_schedule_needs():
    """Three plane groups (the two-slot cost stage's 'slices consumed' wait first occurs at the
    third), more planes than the unit event ring, both frames small for plan_sweep."""
    assert [b - a for a, b in sc.PIECES] == [16, 16, 8] and sc.PIECES[0][0] == 0
    assert all(a[1] == b[0] for a, b in zip(sc.PIECES, sc.PIECES[1:]))
    for B, N, H, W, D in sc.FRAMES:
        assert D == sc.PIECES[-1][1] == 40 and D > 8 and B * H * W <= 65536 and H % 4 == 0 and W % 4 == 0
    assert set(sc.SCHEDULES) == {"small", "large", "one-stream"}
