"""numpy restatement of the sub-plane refinement of the winner-take-all (include/aarmvs.h,
aarmvs_sweep_r), in two forms:

* ``sequential``: the online update plane by plane in float32, every operation rounded on its
  own, as the kernels do it (the WTA's arithmetic select included, so NaN and inf land where
  they do there); numpy's float32 exp is not bit-for-bit the device's expf, so this form is
  compared with the GPU only through ``from_volume64``'s tolerance;
* ``from_volume64``: the definition evaluated in float64 from the whole volume (first arg-max,
  the winner's neighbours, the quotient).  For cost volumes that are finite and do not overflow
  in float32: it has no fallback for a non-finite s or num other than numpy's own isfinite.

Shapes: cost [B,D,HW] (or [B,D,H,W]), depth_values [B,D]; outputs [B,HW] (or [B,H,W]).
"""
import numpy as np

F = np.float32


def _flat(cost):
    cost = np.asarray(cost)
    B, D = cost.shape[:2]
    return cost.reshape(B, D, -1), cost.shape[2:]


def sequential(cost, depth_values, n=None):
    """The kernels' float32 op sequence over planes 0..n-1 (default: all D)."""
    c, tail = _flat(np.asarray(cost, F))
    dv = np.asarray(depth_values, F)
    B, D, HW = c.shape
    n = D if n is None else int(n)
    mp, dp, es = (np.zeros((B, HW), F) for _ in range(3))
    idx = np.full((B, HW), -1, np.int32)
    p_prev, p_left, p_right = (np.zeros((B, HW), F) for _ in range(3))
    with np.errstate(all="ignore"):
        for d in range(n):
            p = np.exp(c[:, d]).astype(F)
            win = mp < p
            nxt = ~win & (idx == d - 1)
            idx = np.where(win, d, idx).astype(np.int32)
            p_left = np.where(win, p_prev, p_left)
            p_right = np.where(win, F(0), np.where(nxt, p, p_right))
            p_prev = p
            f = win.astype(F)
            dvd = dv[:, d:d + 1]
            mp = (f * p + (F(1) - f) * mp).astype(F)          # drmvsnet.py:324-334
            dp = (f * dvd + (F(1) - f) * dp).astype(F)
            es = (es + p).astype(F)
        conf = (mp / es).astype(F)
        w = idx
        left, right = w >= 1, (w >= 0) & (w + 1 < n)
        pl = np.where(left, p_left, F(0)).astype(F)
        pr = np.where(right, p_right, F(0)).astype(F)
        s = ((pl + mp).astype(F) + pr).astype(F)
        conf_window = np.where(w >= 0, (s / es).astype(F), conf)
        wc = np.clip(w, 1, max(D - 2, 1))
        take = lambda k: np.take_along_axis(dv, np.clip(k, 0, D - 1), 1)
        dw, dl, dr = take(wc), take(wc - 1), take(wc + 1)
        num = ((pl * (dl - dw).astype(F)).astype(F) + (pr * (dr - dw).astype(F)).astype(F)).astype(F)
        refined = (dw + (num / s).astype(F)).astype(F)
        ok = left & right & np.isfinite(s) & np.isfinite(num)
        depth_refined = np.where(ok, refined, dp)
    sh = (B,) + tuple(tail)
    return {"depth_refined": depth_refined.reshape(sh), "conf_window": conf_window.reshape(sh),
            "index": idx.reshape(sh), "depth": dp.reshape(sh), "conf": conf.reshape(sh),
            "refined": ok.reshape(sh)}


def from_volume64(cost, depth_values, n=None):
    """The definition in float64 from the volume.  Also ``near_tie`` (the two largest exp(cost)
    of the pixel differ by less than 1e-6 relative: the winner may legitimately differ under
    float32 rounding) and ``spread`` = max |d[w+-1] - d[w]| of refined pixels (0 elsewhere)."""
    c, tail = _flat(np.asarray(cost, np.float64))
    dv = np.asarray(depth_values, np.float64)
    B, D, HW = c.shape
    n = D if n is None else int(n)
    p = np.exp(c[:, :n])
    w = np.argmax(p, axis=1)                                   # the first maximum
    pw = np.take_along_axis(p, w[:, None], 1)[:, 0]
    w = np.where(pw > 0, w, -1)                                # strict < from max_prob = 0
    top = np.sort(p, axis=1)[:, ::-1]
    near_tie = (top[:, 0] - top[:, 1] < 1e-6 * top[:, 0]) if n > 1 else np.zeros((B, HW), bool)
    es = p.sum(1)
    left, right = w >= 1, (w >= 0) & (w + 1 < n)
    gp = lambda k: np.take_along_axis(p, np.clip(k, 0, n - 1)[:, None], 1)[:, 0]
    gd = lambda k: np.take_along_axis(dv, np.clip(k, 0, D - 1), 1)
    pl, pr = np.where(left, gp(w - 1), 0.0), np.where(right, gp(w + 1), 0.0)
    dw, dl, dr = gd(w), gd(w - 1), gd(w + 1)
    s = pl + pw + pr
    num = pl * (dl - dw) + pr * (dr - dw)
    ok = left & right & np.isfinite(s) & np.isfinite(num)
    wta = np.where(w >= 0, dw, 0.0)
    with np.errstate(all="ignore"):
        depth_refined = np.where(ok, dw + num / s, wta)
        conf = pw / es
        conf_window = np.where(w >= 0, s / es, conf)
    spread = np.where(ok, np.maximum(np.abs(dl - dw), np.abs(dr - dw)), 0.0)
    sh = (B,) + tuple(tail)
    return {"depth_refined": depth_refined.reshape(sh), "conf_window": conf_window.reshape(sh),
            "index": w.astype(np.int32).reshape(sh), "depth": wta.reshape(sh), "conf": conf.reshape(sh),
            "refined": ok.reshape(sh), "near_tie": near_tie.reshape(sh), "spread": spread.reshape(sh),
            "d_w": dw.reshape(sh)}


def depth_bound(ref64):
    """The float32 form's allowed distance from ``from_volume64``'s depth_refined, per pixel:
    2^-23 |d_w| (the final add) + 2^-19 max |d[w+-1] - d[w]| (about 2 ulp per expf on each of
    the three probabilities and six roundings in the quotient, each of which moves num / s by at
    most 2^-24 ... 2^-22 of the spread: 16 * 2^-23 in all)."""
    return 2.0 ** -23 * np.abs(ref64["d_w"]) + 2.0 ** -19 * ref64["spread"]
