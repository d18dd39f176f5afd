"""Helpers of the stream and thread contract tests (tests/test_gpu_streams.py,
tests/test_stream_cases.py).

The contract under test (include/aarmvs.h, "Streams and threads"): a call is ordered after
everything its stream held and before everything enqueued on that stream afterwards, and calls
from several streams or host threads do not disturb each other as long as each has its own
buffers.  The tests make that visible with three tools:

* ``delay(stream, ms)`` keeps a stream busy, so that a whole call (or several) is enqueued while
  nothing under test has started; the event it returns must still be pending when the last
  enqueue returns (``require_pending``), which makes a test deterministic rather than lucky.
  The delay is sized from the measured host enqueue time of the serial call (``delay_ms``).
* Poison: a second valid scene of the same geometry (other features, the depth list reversed,
  the source views' relative projections rotated).  Input buffers hold it before the producer
  copies (enqueued behind the delay) and again right after the call, so a stream that starts
  early or is still reading after the call's return computes something else.
* Serial references: the same call alone on the default stream, then a synchronize.  Every
  schedule is documented as bit-identical, so concurrency may not change a bit (``same_bits``).

The pure functions (``delay_ms``, ``interleave``) need no device and are checked on the CPU.
"""
from __future__ import annotations

import os
import time

FRAMES = [(1, 3, 32, 48, 40), (2, 4, 24, 40, 40)]   # (B, N, H, W, D): three plane groups 16 + 16 + 8
PIECES = [(0, 16), (16, 32), (32, 40)]
DELAY_FACTOR, DELAY_MIN_MS, DELAY_MAX_MS = 4.0, 20.0, 300.0
# schedule name -> (AARMVS_SMALL_PX or None, overlap)
SCHEDULES = {"small": (None, True), "large": ("0", True), "one-stream": (None, False)}
DEV = "cuda"


def delay_ms(enqueue_seconds: float) -> float:
    """The delay for a call whose un-synchronised serial enqueue took ``enqueue_seconds`` of host
    time: four times that (margin for a second caller's enqueue and for Python), at least 20 ms,
    at most 300 ms."""
    if not enqueue_seconds >= 0.0:
        raise ValueError(f"enqueue time {enqueue_seconds!r}")
    return min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * 1e3 * float(enqueue_seconds)))


def interleave(*seqs):
    """Round robin over the sequences: (0, a0), (1, b0), (0, a1), ...; an exhausted sequence
    drops out and the others go on in order."""
    its = [iter(s) for s in seqs]
    live = list(range(len(its)))
    while live:
        for i in list(live):
            try:
                item = next(its[i])
            except StopIteration:
                live.remove(i)
                continue
            yield i, item


def set_schedule(monkeypatch, name: str) -> bool:
    """Sets the plan override of ``SCHEDULES[name]`` (the library reads it per call); returns the
    ``overlap`` value for the DepthSweep."""
    small_px, overlap = SCHEDULES[name]
    if small_px is None:
        monkeypatch.delenv("AARMVS_SMALL_PX", raising=False)
    else:
        monkeypatch.setenv("AARMVS_SMALL_PX", small_px)
    return overlap


# ---------------------------------------------------------------------------------------
# device helpers (torch imported on use: the CPU checks import this module without a device)
# ---------------------------------------------------------------------------------------
_cycles_per_ms = None


def _sleep_cycles_per_ms() -> float:
    """torch.cuda._sleep's cycles per millisecond on this device, measured once with timing
    events.  The counter follows the shader clock, which an idle device lowers (a first version
    measured a 2 ms spin on an idle device and got delays 2.8 times too short): the spin grows
    until it lasts 8 ms, each spin warming the clocks for the next, and the rate is the largest
    of three such spins, so a delay is at least as long as asked once the clocks are up."""
    global _cycles_per_ms
    import torch
    if _cycles_per_ms is None:
        def spin_ms(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        n, ms = 1_000_000, 0.0
        for _ in range(10):
            ms = spin_ms(n)
            if ms >= 8.0:
                break
            n *= 4
        assert ms >= 1.0, f"torch.cuda._sleep({n}) took {ms} ms: cannot size a delay"
        _cycles_per_ms = max(n / t for t in (ms, spin_ms(n), spin_ms(n)))
    return _cycles_per_ms


def delay(stream, ms: float):
    """Keeps ``stream`` busy for about ``ms`` milliseconds and returns an event recorded behind
    that work (``actual_ms(event)`` is the time it really took, once it has completed)."""
    import torch
    cycles = int(_sleep_cycles_per_ms() * ms)
    with torch.cuda.stream(stream):
        began = torch.cuda.Event(enable_timing=True)
        began.record(stream)
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream)
    ev.began = began
    return ev


def actual_ms(event) -> float:
    event.synchronize()
    return event.began.elapsed_time(event)


def still_pending(event) -> bool:
    """Whether the delay's event was still pending when this was first asked (the answer is
    kept: the caller asks right after its last enqueue, and may wait for the event later)."""
    if not hasattr(event, "held"):
        event.held = not event.query()
    return event.held


def require_pending(event, what: str, **times) -> None:
    """The precondition of a delay-based test: right after the last enqueue returned, the
    delay's event is still pending, i.e. nothing under test has started.  Fails (no skip, no
    retry) with the measured times otherwise."""
    if not still_pending(event):
        shown = ", ".join(f"{k} {v:.3f}" for k, v in times.items())
        raise AssertionError(f"{what}: the delay ran out before the last enqueue returned ({shown}); "
                             "the test would not have been deterministic")


def note(test: str, **values) -> None:
    """One line of measured values per test: printed, and appended to the file named by
    AARMVS_STREAM_PROFILE when that is set (profiles/stream_reentrancy.txt is such a run)."""
    line = test + ": " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in values.items())
    print(line)
    path = os.environ.get("AARMVS_STREAM_PROFILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def same_bits(got: dict, want: dict, what: str) -> None:
    """Every tensor of ``want`` is in ``got`` with the same shape, dtype and bytes (NaN payloads
    included)."""
    bad = []
    for k, w in want.items():
        g = got.get(k)
        if g is None or g.shape != w.shape or g.dtype != w.dtype:
            bad.append(f"{k} (missing or other shape)")
        elif g.cpu().numpy().tobytes() != w.cpu().numpy().tobytes():
            n = int((g.cpu().view(-1) != w.cpu().view(-1)).sum())
            bad.append(f"{k} ({n} of {w.numel()} elements differ)")
    assert not bad, f"{what}: not bit-equal to the serial run: {bad}"


def differs(got: dict, want: dict) -> bool:
    return any(got[k].cpu().numpy().tobytes() != w.cpu().numpy().tobytes() for k, w in want.items())


class Scene:
    """The true scene, the poison scene and one set of input buffers of a frame, on the device."""

    def __init__(self, frame, seed: int, poison_seed: int):
        import torch
        from aarmvs import ops, synthetic as syn
        self.frame = B, N, H, W, D = frame
        self.nsrc = N - 1
        true = syn.scene(B, N, H, W, D, seed=seed)
        pois = syn.scene(B, N, H, W, D, seed=poison_seed, descending=True)
        proj = torch.from_numpy(true["proj_matrices"])
        rel = torch.stack([ops.relative_projection(proj[:, v], proj[:, 0]) for v in range(1, N)])
        rel = rel.reshape(N - 1, B, 12).contiguous()
        self.host = {"true": (torch.from_numpy(true["features"]), proj, torch.from_numpy(true["depth_values"])),
                     "poison": (torch.from_numpy(pois["features"]), proj, torch.from_numpy(pois["depth_values"]))}
        self.data = {"true": (self.host["true"][0].to(DEV), self.host["true"][2].to(DEV), rel.to(DEV)),
                     "poison": (self.host["poison"][0].to(DEV), self.host["poison"][2].to(DEV),
                                rel.roll(1, 0).contiguous().to(DEV))}
        self.f, self.dv, self.rel = (t.clone() for t in self.data["poison"])
        self.R = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
        torch.cuda.synchronize()

    def host_rel(self, which: str):
        """The scene's relative projections as the oracle takes them (per source view, [B,3,4])."""
        return [r.reshape(-1, 3, 4) for r in self.data[which][2].cpu()]

    def fill(self, which: str) -> None:
        """Device-to-device copies of a scene into the input buffers, on the current stream."""
        f, dv, rel = self.data[which]
        self.f.copy_(f, non_blocking=True)
        self.dv.copy_(dv, non_blocking=True)
        self.rel.copy_(rel, non_blocking=True)

    def views(self):
        return self.f[0], [self.f[v] for v in range(1, self.nsrc + 1)]


def make_sweep(wseed: int, overlap: bool = True, precision: str = "split"):
    """(DepthSweep, host parameters) on the current stream; the caller orders other streams
    after it (wait_stream), as the DepthSweep docstring asks."""
    import torch
    from aarmvs import ops, synthetic as syn
    P = {k: torch.from_numpy(v) for k, v in syn.sweep_weights(wseed).items()}
    return ops.DepthSweep({k: v.to(DEV) for k, v in P.items()}, DEV, overlap=overlap, precision=precision), P


REFINE_KEYS = ("depth_refined", "conf_window", "index")
POSTERIOR_KEYS = ("depth_mean", "depth_std", "entropy", "runner_up")


def eval_steps(sw, sc: Scene, res: dict, pieces=PIECES, extras: bool = True):
    """The eval sweep of the scene's input buffers in ``d_range`` pieces, on the current stream
    of each ``next()``: depth, confidence, the cost volume and (``extras``) the refinement and
    the posterior statistics of every piece.  Yields after each piece's enqueue; ``res`` is
    filled with clones (taken on the stream of the last step) when the generator ends."""
    import torch
    B, N, H, W, D = sc.frame
    ref, srcs = sc.views()
    cost = torch.empty(B, D, H, W, device=DEV)
    keep, outs = [], {}
    for d0, d1 in pieces:
        o = sw(ref, srcs, None, [None] * sc.nsrc, sc.dv, want_depth=True, cost_out=cost, d_range=(d0, d1),
               rel=sc.rel, want_refined=extras, want_posterior=extras)
        keep.append(o)
        if extras:
            for k in REFINE_KEYS + POSTERIOR_KEYS:
                outs[f"{k}[{d0},{d1})"] = o[k]
        if d1 == D:
            outs["depth"], outs["conf"], outs["cost"] = o["depth"], o["conf"], cost
            res.update({k: v.clone() for k, v in outs.items()})
            res["_keep"] = keep
        yield (d0, d1)


def train_steps(sw, sc: Scene, rec: dict, res: dict):
    """A training step on the current stream: the recorded forward, dL/dcost of
    sum(R * softmax(cost)) produced on the same stream, the backward with grad_x.  Yields after
    the forward and after the backward; fills ``res`` with the cost volume and every gradient."""
    import torch
    B, N, H, W, D = sc.frame
    ref, srcs = sc.views()
    cost = torch.empty(B, D, H, W, device=DEV)
    o = sw(ref, srcs, None, [None] * sc.nsrc, sc.dv, want_depth=False, cost_out=cost, rel=sc.rel, record=rec)
    yield "forward"
    prob = torch.softmax(cost, dim=1)
    gcost = prob * (sc.R - (sc.R * prob).sum(dim=1, keepdim=True))
    g_ref, g_src, gp, gx = sw.backward(ref, srcs, sc.rel, sc.dv, rec, gcost, want_grad_x=True)
    res["cost"] = cost.clone()
    res["grad_ref"] = g_ref.clone()
    for v, g in enumerate(g_src):
        res[f"grad_src{v}"] = g.clone()
    res["grad_x"] = gx.clone()
    for k, g in gp.items():
        res["param:" + k] = g.clone()
    res["_keep"] = (o, gcost, prob)
    yield "backward"


def run(gen) -> None:
    for _ in gen:
        pass


def tensors(res: dict) -> dict:
    return {k: v for k, v in res.items() if not k.startswith("_")}


def timed_serial(make_gen):
    """Runs ``make_gen(res)`` alone on the default stream: (results, host seconds of the
    un-synchronised enqueue)."""
    import torch
    torch.cuda.synchronize()
    res = {}
    t0 = time.perf_counter()
    run(make_gen(res))
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return tensors(res), dt
