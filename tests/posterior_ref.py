"""numpy restatement of the sweep's depth-posterior statistics (include/aarmvs.h,
aarmvs_posterior_args), in two forms, the error bounds between them, and the sparsification
error (AUSE) that train_ddp --uncertainty_metrics reports:

* ``sequential32``: the online update plane by plane in float32, every operation rounded on its
  own, as the kernels do it (the WTA's arithmetic select included, so NaN and inf land where
  they do there); numpy's float32 exp is not bit-for-bit the device's expf, so this form is
  compared with the GPU only through ``from_volume64`` and ``bounds``;
* ``from_volume64``: the two-pass definition in float64 from the whole volume: the softmax with
  max-subtraction, sum q d, sum q (d - mean)^2, -sum q ln q and the second largest p over sum p;
* ``bounds``: what float32 may lose on the way, by first-order propagation of one rounding
  (u = 2^-24) per operation and 2^-22 per expf / logf.  Nothing in it comes from a GPU result.

Shapes: cost [B,D,HW] (or [B,D,H,W]), depth_values [B,D]; outputs [B,HW] (or [B,H,W]).
"""
import numpy as np

F = np.float32
KEYS = ("depth_mean", "depth_std", "entropy", "runner_up")
U = 2.0 ** -24       # one correctly rounded float32 operation
UE = 2.0 ** -22      # expf / logf of the device: not correctly rounded


def _flat(cost):
    cost = np.asarray(cost)
    B, D = cost.shape[:2]
    return cost.reshape(B, D, -1), cost.shape[2:]


def sequential32(cost, depth_values, n=None, naive=False):
    """The kernels' float32 op sequence over planes 0..n-1 (default: all D).  ``naive`` rescales
    the variance by 1 - k instead of S0 / S1: the textbook form that the definition rules out."""
    c, tail = _flat(np.asarray(cost, F))
    dv = np.asarray(depth_values, F)
    B, D, HW = c.shape
    n = D if n is None else int(n)
    mp, dp, es, mu, V, E, p2 = (np.zeros((B, HW), F) for _ in range(7))
    v_min = np.zeros((B, HW), F)
    with np.errstate(all="ignore"):
        for d in range(n):
            cd = c[:, d]
            p = np.exp(cd).astype(F)
            x = dv[:, d:d + 1]
            win = mp < p
            p2 = np.where(win, mp, np.where(p2 < p, p, p2)).astype(F)
            s1 = (es + p).astype(F)
            k, j = (p / s1).astype(F), (es / s1).astype(F)
            dl = (x - mu).astype(F)
            mu_n = (mu + (dl * k).astype(F)).astype(F)
            scale = (F(1) - k).astype(F) if naive else j
            V_n = (scale * (V + ((dl * dl).astype(F) * k).astype(F)).astype(F)).astype(F)
            E_n = (E + ((cd - E).astype(F) * k).astype(F)).astype(F)
            pos = p > 0
            mu, V, E = np.where(pos, mu_n, mu), np.where(pos, V_n, V), np.where(pos, E_n, E)
            v_min = np.fmin(v_min, V)
            f = win.astype(F)
            mp = (f * p + (F(1) - f) * mp).astype(F)          # drmvsnet.py:324-334
            dp = (f * x + (F(1) - f) * dp).astype(F)
            es = s1
        ok = (es > 0) & np.isfinite(es)
        nan = F(np.nan)
        h = (np.log(es).astype(F) - E).astype(F)
        out = {"depth_mean": np.where(ok, mu, nan), "depth_std": np.where(ok, np.sqrt(V).astype(F), nan),
               "entropy": np.where(ok, np.where(h > 0, h, F(0)), nan),
               "runner_up": np.where(ok, (p2 / es).astype(F), nan),
               "depth": dp, "conf": (mp / es).astype(F), "var": V, "var_min": v_min}
    sh = (B,) + tuple(tail)
    return {k: np.asarray(v, F).reshape(sh) for k, v in out.items()}


def from_volume64(cost, depth_values, n=None):
    """The definition in float64 from the volume (finite costs).  Beside the four outputs it
    returns what ``bounds`` needs, from one float64 pass over the planes in the kernels' order:
    ``_e_mean`` / ``_e_cost``, the first-order error of the running means of depth and cost (see
    ``bounds``), ``_e_std`` likewise for the standard deviation, ``_log_s`` = ln sum p, ``_ecost``
    = sum q c and ``_n``."""
    c, tail = _flat(np.asarray(cost, np.float64))
    dv = np.asarray(depth_values, np.float64)
    B, D, HW = c.shape
    n = D if n is None else int(n)
    c, dv = c[:, :n], dv[:, :n]
    cmax = c.max(1)
    e = np.exp(c - cmax[:, None])
    S = e.sum(1)
    q = e / S[:, None]
    x = dv[:, :, None]
    mean = (q * x).sum(1)
    var = (q * (x - mean[:, None]) ** 2).sum(1)
    lnq = (c - cmax[:, None]) - np.log(S)[:, None]
    entropy = -(np.where(q > 0, q * lnq, 0.0)).sum(1)
    runner = np.sort(e, axis=1)[:, -2] / S if n > 1 else np.zeros((B, HW))
    # the running pass: with rho_k the relative error of k = p / S1 as the kernel has it,
    #   e_d = j_d e_{d-1} + u |mean_d| + rho_k k_d |delta_d|        (the error of the running mean)
    #   g_d = j_d (g_{d-1} + k_d e_{d-1}^2)                          (its weight in the variance)
    rho_k = 2 * UE + (n + 3) * U
    s = np.zeros((B, HW))
    mu, ec = np.zeros((B, HW)), np.zeros((B, HW))
    e_mu, e_c, g = np.zeros((B, HW)), np.zeros((B, HW)), np.zeros((B, HW))
    for d in range(n):
        p = e[:, d]
        s1 = s + p
        k, j = p / s1, s / s1
        dl, dc = dv[:, d:d + 1] - mu, c[:, d] - ec
        g = j * (g + k * e_mu ** 2)
        mu, ec = mu + dl * k, ec + dc * k
        e_mu = j * e_mu + U * np.abs(mu) + rho_k * k * np.abs(dl)
        e_c = j * e_c + U * np.abs(ec) + rho_k * k * np.abs(dc)
        s = s1
    sh = (B,) + tuple(tail)
    out = {"depth_mean": mean, "depth_std": np.sqrt(var), "entropy": entropy, "runner_up": runner,
           "_e_mean": e_mu, "_e_cost": e_c, "_e_std": np.sqrt(g), "_log_s": cmax + np.log(S),
           "_ecost": (q * c).sum(1)}
    out = {k: v.reshape(sh) for k, v in out.items()}
    out["_n"] = n
    return out


def bounds(ref64):
    """One bound per output on |float32 form - ``from_volume64``|: absolute for depth_mean,
    depth_std and entropy, relative for runner_up.  n planes, u = 2^-24, ue = 2^-22.

    Weights.  p = expf(c) carries ue.  exp_sum after d planes carries ue + d u (all terms are
    positive).  So k = p / S1 carries rho_k = 2 ue + (n + 1) u, and with the subtraction and the
    product of delta * k, (n + 3) u.

    depth_mean.  mu_d = mu_{d-1} + delta k: the step's error is u |mu_d| (the add) plus
    rho_k k |delta|, and every later step multiplies it by j = 1 - k.  The sum over the planes is
    ``_e_mean``, evaluated in float64 along the same order.

    depth_std.  V is a sum of non-negative terms k_d delta_d^2 prod_{i >= d} j_i.  (a) The error
    e_{d-1} of the running mean inside delta_d moves V by sum w_d (2 delta_d e + e^2) <=
    2 sqrt(g) sqrt(V) + g with g = sum w_d e_{d-1}^2 (Cauchy-Schwarz), which moves sqrt(V) by at
    most sqrt(g) = ``_e_std``.  (b) Each term's factor carries a relative error: k (2 ue + (n+1) u),
    delta^2 (3 u), the product and the add (2 u), and the product of the later j = S0 / S1, which
    telescopes to S_d / S_n (2 ue + 2 n u) with one division, one add and one product per plane
    (3 n u): 4 ue + (6 n + 6) u on V, half of it on sqrt(V), plus u for the square root.

    entropy = logf(S) - E.  logf: ue |ln S|, and ue + n u from S itself; E is a running mean like
    depth_mean (``_e_cost``); the subtraction: u (|ln S| + |E|) covers it and the clamp at 0 only
    helps.

    runner_up = p2 / S: ue (expf) + ue + n u (the sum) + u (the division), relative."""
    n = ref64["_n"]
    std = ref64["_e_std"] + (0.5 * (4 * UE + (6 * n + 6) * U) + U) * ref64["depth_std"]
    ent = ((UE + U) * np.abs(ref64["_log_s"]) + (UE + n * U) + ref64["_e_cost"] + U * np.abs(ref64["_ecost"]))
    return {"depth_mean": ref64["_e_mean"], "depth_std": std, "entropy": ent,
            "runner_up": np.full_like(ref64["runner_up"], 2 * UE + (n + 1) * U)}


def error_over_bound(got, ref64, bnd=None):
    """{key: max over pixels of |got - ref| / bound} (runner_up: of the relative error); a pixel
    with a zero bound and a zero error counts as 0."""
    bnd = bounds(ref64) if bnd is None else bnd
    out = {}
    for k in KEYS:
        err = np.abs(np.asarray(got[k], np.float64) - ref64[k])
        if k == "runner_up":
            err = np.where(ref64[k] > 0, err / np.where(ref64[k] > 0, ref64[k], 1.0), err)
        with np.errstate(all="ignore"):
            r = np.where(err == 0, 0.0, err / bnd[k])
        out[k] = float(np.max(r))
    return out


def late_dominant(rng, B, D, HW, boost=25.0):
    """A randn cost volume [B,D,HW] with ``boost`` added to one random plane per pixel: the plane
    then holds all but ~1e-8 of the mass, k rounds to within 2^-24 of 1 on it and 1 - k loses the
    variance of everything before it."""
    c = rng.standard_normal((B, D, HW)).astype(F)
    idx = rng.integers(0, D, (B, 1, HW))
    np.put_along_axis(c, idx, np.take_along_axis(c, idx, 1) + F(boost), 1)
    return c


def ause(err, unc, mask, steps=50):
    """Area under the sparsification error curve of ``err`` ranked by ``unc`` over the pixels
    with mask > 0.5: sort by uncertainty, descending and stable (NaN counts as the most
    uncertain); for k = 0..steps-1 drop the first floor(k n / steps) pixels and average the rest;
    do the same ranked by the error itself; the mean difference of the two curves over the mean
    error."""
    valid = np.asarray(mask).reshape(-1) > 0.5
    e = np.asarray(err, np.float64).reshape(-1)[valid]
    u = np.asarray(unc, np.float64).reshape(-1)[valid]
    u = np.where(np.isnan(u), np.inf, u)
    n = e.size

    def curve(rank):
        s = e[np.argsort(-rank, kind="stable")]
        tail = np.concatenate([np.cumsum(s[::-1])[::-1], [0.0]])   # tail[i] = sum s[i:]
        drop = (np.arange(steps) * n) // steps
        return tail[drop] / (n - drop)

    return float(np.mean(curve(u) - curve(e)) / e.mean())
