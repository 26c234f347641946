"""References and error bounds for the per-(sample, channel) sums (ops.changroup, csrc/changroup.hip) and the five metrics the
ActivityMonitor derives from them (ops.changroup_metrics, tracking/monitor.py) -- a helper module, not a test.

* ref_sums: float64 S1 = sum y, S2 = sum y^2, A = sum |y| per (b, c) with an error radius per sum (below).
* ref_metrics: the per-sample quantities and the five metrics straight from the tensor in float64, by the two-pass formulas
  (v_bc = sum_p (y - mu_bg)^2 with mu_bg computed first: no cancellation), in numpy: independent of the code under test.
* metric_bounds: what an error radius on the sums can do to each metric, by interval arithmetic on the kernel-side formulas.

The kernel's accumulation (csrc/changroup.hip), for a tensor of HW pixels per image and nchunk = ops.changroup_chunks chunks of
per = ceil(HW / nchunk) pixels: a lane adds ceil(per / PR) values of its channel in float64, PR = 256 // (channel units of the
channel's 256-channel tile) pixel rows; the workgroup's PR lane sums are added in row order; the final pass adds the nchunk
partials in chunk order.  Every value passes through at most
    D = ceil(per / PR) + PR + nchunk
float64 additions (the first of each chain, onto 0, is exact, which the count ignores), each with relative error at most
u = 2^-53, and the square of an fp32 value is exact in float64.  So |computed - exact| <= gamma_D sum |term| with
gamma_D = D u / (1 - D u) (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4: any order of D additions), the
terms being y, y^2 and |y|.  Without a transform the terms are the stored values and that is the whole error.  Behind a
GroupNorm transform the device evaluates y in fp32; chanhist_refs.ref_transformed gives the float64 value and the radius d an
fp32 evaluation stays within, which adds sum d to S1 and A and sum (2 |y| d + d^2) to S2.

The condition the scheme must meet (not a measured number): at every shape the tests use, the case of a channel with mean
10^3 sigma included, the bound of group_variance_share_per_channel that follows from the accumulation's radii is below 1 % of
the uniform share 1 / cg (assert_share_bound_small).  With fp32 accumulators it would not be: u = 2^-24 and sum y^2 = 10^6 n
against v = n gives a bound above 1.  The fp32 evaluation of y behind a transform is not part of that condition: it is the data
every accumulation scheme is handed (two SiLU values of one group that nearly coincide in a 1 x 1 map make the share of either
uncertain whatever adds them up); the values themselves are still held to the full radius.
"""
import numpy as np
import torch

import chanhist_refs as HR

XF_NONE, XF_AFFINE, XF_AFFINE_SILU = 0, 1, 2
U64 = 2.0 ** -53
SHARE, NRMS, DOM = "group_variance_share_per_channel", "normalized_rms_per_channel", "group_dominance_per_group"
ACTIVE, VARIATION = "active_sample_fraction_per_channel", "sample_variation_per_channel"
FIVE = [SHARE, NRMS, DOM, ACTIVE, VARIATION]


def draw(shape, seed):
    """the moments suite's generator: randn * 1.3 + 0.4"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * 1.3 + 0.4


def chunks(B, HW, Cc):
    """ops.changroup_chunks restated (tests/test_changroup_host.py holds the two together)"""
    units, tile = (Cc // 4, 64) if Cc % 4 == 0 else (Cc, 256)
    pr = max(1, 256 // min(tile, units))
    tiles = (units + tile - 1) // tile
    nch = max(1, min(1024 // max(B * tiles, 1), HW // (16 * pr)))
    per = (HW + nch - 1) // nch
    return (HW + per - 1) // per


def chain_depth(B, HW, Cc, vec=None):
    """D per channel, int64 [C]: the float64 additions a value passes through (module docstring).  vec: whether the kernel takes
    four channels per lane (default: C % 4 == 0, what a contiguous or 16-byte aligned tensor gives)"""
    vec = Cc % 4 == 0 if vec is None else vec
    W = 4 if vec else 1
    nu, UT = Cc // W, 256 // W
    nch = chunks(B, HW, Cc)
    per = (HW + nch - 1) // nch
    D = np.zeros(Cc, dtype=np.int64)
    for c in range(Cc):
        tile = (c // W) // UT
        nut = min(UT, nu - tile * UT)
        PR = 256 // nut
        D[c] = (per + PR - 1) // PR + PR + nch
    return D


def gamma(D):
    D = np.asarray(D, dtype=np.float64)
    return D * U64 / (1.0 - D * U64)


def values(x: torch.Tensor, scale=None, shift=None, xf=XF_NONE):
    """float64 y = XF(x) [B, HW, C] and the radius d [B, HW, C] of the device's fp32 evaluation (0 without a transform)"""
    B, Cc = x.shape[0], x.shape[-1]
    if xf == XF_NONE:
        y = x.detach().cpu().float().double().reshape(B, -1, Cc).numpy()
        return y, np.zeros_like(y)
    y, d = HR.ref_transformed(x, scale, shift, xf)
    return y.reshape(B, -1, Cc), d.reshape(B, -1, Cc)


def ref_sums(x: torch.Tensor, scale=None, shift=None, xf=XF_NONE, vec=None, parts=False):
    """(sums float64 [B, C, 3], radius float64 [B, C, 3]) of y = XF(x); non-finite values propagate as IEEE sums do.  parts: the
    accumulation's share of the radius as a third result (the whole of it without a transform)"""
    y, d = values(x, scale, shift, xf)
    B, HW, Cc = y.shape
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(y)
        sums = np.stack([y.sum(axis=1), (y * y).sum(axis=1), a.sum(axis=1)], axis=2)
        g = gamma(chain_depth(B, HW, Cc, vec))[None, :]
        ahat = a + d  # what the device may have added
        e1 = d.sum(axis=1) + g * ahat.sum(axis=1)
        e2 = (2.0 * a * d + d * d).sum(axis=1) + g * (ahat * ahat).sum(axis=1)
        rad = np.stack([e1, e2, e1], axis=2)
        acc = np.stack([g * ahat.sum(axis=1), g * (ahat * ahat).sum(axis=1), g * ahat.sum(axis=1)], axis=2)
    return (sums, rad, acc) if parts else (sums, rad)


def assert_sums_close(got: np.ndarray, sums: np.ndarray, rad: np.ndarray):
    """the device's sums against ref_sums: finite entries within their radius, non-finite ones the same non-finite value"""
    assert got.dtype == np.float64 and got.shape == sums.shape, (got.dtype, got.shape, sums.shape)
    fin = np.isfinite(sums)
    assert np.array_equal(np.isnan(got), np.isnan(sums)), np.argwhere(np.isnan(got) != np.isnan(sums))[:8]
    inf = np.isinf(sums)
    assert np.array_equal(got[inf], sums[inf])
    err = np.abs(got[fin] - sums[fin])
    assert (err <= rad[fin]).all(), (float((err / np.maximum(rad[fin], 1e-300)).max()), np.argwhere(~(np.abs(got - sums) <= rad) & fin)[:8])
    return float((err / np.maximum(rad[fin], 1e-300)).max()) if err.size else 0.0


def per_sample(y: np.ndarray, groups, eps):
    """from the tensor, two-pass, float64: share, nrms [B, C], dom [B, G], m [B, C] (groups None: the first three are None)"""
    B, HW, Cc = y.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.abs(y).sum(axis=1) / HW
        if groups is None:
            return None, None, None, m
        cg = Cc // groups
        yg = y.reshape(B, HW, groups, cg)
        mu = yg.mean(axis=(1, 3), keepdims=True)
        v = ((yg - mu) ** 2).sum(axis=1)  # [B, G, cg]
        V = v.sum(axis=2, keepdims=True)
        share = np.where(V == 0.0, 0.0, v / np.where(V == 0.0, 1.0, V))
        nrms = np.sqrt((v / HW) / (V / (HW * cg) + eps))
        dom = share.max(axis=2)
        dom = np.where(np.isnan(share).any(axis=2), np.nan, dom)
    return share.reshape(B, Cc), nrms.reshape(B, Cc), dom, m


def summarise(share, nrms, dom, m, tau):
    """the five metrics over the samples given (float64; the monitor rounds them to fp32 at the end)"""
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        if share is not None:
            out[SHARE], out[NRMS], out[DOM] = share.mean(axis=0), nrms.mean(axis=0), dom.mean(axis=0)
        out[ACTIVE] = (m >= tau).mean(axis=0)
        mean = m.mean(axis=0)
        out[VARIATION] = np.where(mean == 0.0, 0.0, m.std(axis=0) / np.where(mean == 0.0, 1.0, mean))
    return out


def ref_metrics(y: np.ndarray, groups, eps, tau):
    return summarise(*per_sample(y, groups, eps), tau)


def _interval_metrics(sums, rad, HW, groups, eps):
    """per-sample [lo, hi] of share and nrms from sums known to within rad, by the kernel-side formulas
    (v = S2 - 2 mu S1 + n mu^2); finite input"""
    B, Cc, _ = sums.shape
    n, cg = float(HW), Cc // groups
    S1, S2 = (sums[:, :, k].reshape(B, groups, cg) for k in (0, 1))
    E1, E2 = (rad[:, :, k].reshape(B, groups, cg) for k in (0, 1))
    mu = S1.sum(axis=2, keepdims=True) / (n * cg)
    dmu = E1.sum(axis=2, keepdims=True) / (n * cg)
    v = np.maximum(S2 - 2.0 * mu * S1 + n * mu * mu, 0.0)
    # d(2 mu S1) <= 2 (|mu| E1 + |S1| dmu + dmu E1); d(n mu^2) <= n (2 |mu| dmu + dmu^2); plus the roundings of the float64
    # evaluation itself, each term to within 2 u of its size
    dv = E2 + 2.0 * (np.abs(mu) * E1 + np.abs(S1) * dmu + dmu * E1) + n * (2.0 * np.abs(mu) * dmu + dmu * dmu) \
        + 4.0 * U64 * (np.abs(S2) + 2.0 * np.abs(mu * S1) + n * mu * mu)
    vlo, vhi = np.maximum(v - dv, 0.0), v + dv
    Vlo, Vhi = vlo.sum(axis=2, keepdims=True), vhi.sum(axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        # share = v / (v + rest): increasing in v, decreasing in the rest of the group
        rest_lo, rest_hi = Vlo - vlo, Vhi - vhi
        s_lo = np.where(vlo + rest_hi > 0.0, vlo / np.where(vlo + rest_hi > 0.0, vlo + rest_hi, 1.0), 0.0)
        s_hi = np.where(vhi + rest_lo > 0.0, vhi / np.where(vhi + rest_lo > 0.0, vhi + rest_lo, 1.0), np.where(vhi > 0.0, 1.0, 0.0))
        s_hi = np.where(Vhi > 0.0, s_hi, 0.0)
        r_lo = np.sqrt((vlo / n) / (Vhi / (n * cg) + eps))
        r_hi = np.sqrt((vhi / n) / (Vlo / (n * cg) + eps))
    rs = lambda t: t.reshape(B, Cc)  # noqa: E731
    alive = np.broadcast_to(v.sum(axis=2, keepdims=True) > 0.0, v.shape)
    return rs(s_lo), rs(s_hi), rs(r_lo), rs(r_hi), rs(alive)


def metric_bounds(sums, rad, HW, groups, eps, tau):
    """{metric: (lo, hi)} float64: every value the five metrics can take when the true sums lie within rad of `sums` (finite
    entries only), widened by the fp32 rounding of the stored result (2^-24 relative)"""
    B, Cc, _ = sums.shape
    n = float(HW)
    out = {}
    if groups is not None:
        s_lo, s_hi, r_lo, r_hi, alive = _interval_metrics(sums, rad, HW, groups, eps)
        share_width = float(np.max(np.where(alive, s_hi - s_lo, 0.0))) / 2.0
        out[SHARE] = (s_lo.mean(axis=0), s_hi.mean(axis=0))
        out[NRMS] = (r_lo.mean(axis=0), r_hi.mean(axis=0))
        cg = Cc // groups
        out[DOM] = (s_lo.reshape(B, groups, cg).max(axis=2).mean(axis=0), s_hi.reshape(B, groups, cg).max(axis=2).mean(axis=0))
    m, em = sums[:, :, 2] / n, rad[:, :, 2] / n + 2.0 * U64 * np.abs(sums[:, :, 2]) / n
    out[ACTIVE] = ((m - em >= tau).mean(axis=0), (m + em >= tau).mean(axis=0))
    mlo, mhi = np.maximum(m - em, 0.0), m + em
    M_lo, M_hi = mlo.mean(axis=0), mhi.mean(axis=0)
    q_lo, q_hi = (mlo * mlo).mean(axis=0), (mhi * mhi).mean(axis=0)
    # the monitor forms var = sum m^2 / S - mean^2 in float64: each term to within a few u of its size on top of the interval
    rnd = 8.0 * U64 * (q_hi + M_hi * M_hi)
    var_lo, var_hi = np.maximum(q_lo - M_hi * M_hi - rnd, 0.0), np.maximum(q_hi - M_lo * M_lo + rnd, 0.0)
    # (the interval of a variance from independent intervals of its terms is loose; the exact variance bounds it from inside)
    with np.errstate(invalid="ignore", divide="ignore"):
        v_lo = np.where(M_hi > 0.0, np.sqrt(var_lo) / np.where(M_hi > 0.0, M_hi, 1.0), 0.0)
        v_hi = np.where(M_lo > 0.0, np.sqrt(var_hi) / np.where(M_lo > 0.0, M_lo, 1.0), np.where(M_hi > 0.0, np.inf, 0.0))
    out[VARIATION] = (v_lo, v_hi)
    f32 = 2.0 ** -24
    res = {k: (lo * (1.0 - f32) - 1e-45, hi * (1.0 + f32) + 1e-45) for k, (lo, hi) in out.items()}
    if groups is not None:
        res["share_width"] = share_width
    return res


def assert_within(got: dict, bounds: dict, ref: dict = None):
    """the monitor's / ops' metrics (arrays) inside their bounds; ref (the two-pass float64 values) must lie inside them too"""
    worst = {}
    for k, (lo, hi) in ((k, v) for k, v in bounds.items() if k != "share_width"):
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == lo.shape, (k, g.shape, lo.shape)
        assert ((lo <= g) & (g <= hi)).all(), (k, np.argwhere(~((lo <= g) & (g <= hi)))[:8], g[~((lo <= g) & (g <= hi))][:4],
                                               lo[~((lo <= g) & (g <= hi))][:4], hi[~((lo <= g) & (g <= hi))][:4])
        if ref is not None:
            r = np.asarray(ref[k], dtype=np.float64)
            assert ((lo <= r) & (r <= hi)).all(), ("reference outside its own bound", k, np.argwhere(~((lo <= r) & (r <= hi)))[:8])
        worst[k] = float(np.max(hi - lo)) if lo.size else 0.0
    return worst


def assert_share_bound_small(bounds: dict, Cc: int, groups: int):
    """the condition on the scheme: the derived bound of the variance share, per (sample, channel), is below 1 % of the uniform
    share 1 / cg wherever the group has any variance (a group with V = 0 has the share 0 by definition: 0 / 0 has no bound to
    meet, and every value in [0, 1] is within reach of a rounding there)"""
    width = bounds["share_width"]
    assert width < 0.01 * groups / Cc, (width, groups / Cc)
    return width


def stats_rows(B, ld, seed):
    return HR.stats_rows(B, ld, seed)


def metrics_from_ops(res, groups):
    """(chan [5, C], grp [G], B) of ops.changroup_metrics -> the five metrics as float64 numpy (the monitor's changroup_summary
    restated; tests/test_changroup_host.py holds the two together)"""
    chan, grp, S = res
    chan, grp, S = chan.detach().cpu().numpy(), grp.detach().cpu().numpy(), float(S)
    mean = chan[2] / S
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.maximum(chan[3] / S - mean * mean, 0.0)
        out = {ACTIVE: chan[4] / S, VARIATION: np.where(mean == 0.0, 0.0, np.sqrt(var) / np.where(mean == 0.0, 1.0, mean))}
    if groups is not None:
        out.update({SHARE: chan[0] / S, NRMS: chan[1] / S, DOM: grp / S})
    return out
