"""Float64 references for the channel covariance (ops.chancov, csrc/chancov.hip; the hook path's formula and
correlation_summary in tracking/monitor.py) -- a helper module, not a test.

* ref: cov, mean and S_c = sum (y_c - K_c)^2 of y = XF(x), with XF evaluated in float64 from the stored x (as chanhist_refs
  does) and K = y at (image 0, pixel 0).
* check: every element of the device covariance within BAR sqrt(S_c S_c') / (N - 1) and the mean within
  1e-6 (|mean| + sqrt(S_c / N)); returns the worst measured ratios on those scales.
* summary_ref: correlation matrix, per-channel redundancy and participation ratio with numpy, for correlation_summary.
"""
import numpy as np
import torch

from chanhist_refs import XF_AFFINE, XF_AFFINE_SILU, XF_NONE, stats_rows  # noqa: F401  (re-exported generators)
from conv_routes import BAR_WGRAD

BAR = BAR_WGRAD        # 3e-5: the project's figure for a split-bf16 pixel contraction; a ceiling, not a target
MEAN_TOL = 1e-6


def y64(x: torch.Tensor, scale=None, shift=None, xf: int = XF_NONE) -> np.ndarray:
    """float64 y = XF(x) [B, HW, C] from the stored values of an NHWC tensor (any device, fp32 or bf16, a prefix view allowed)"""
    B, Cc = x.shape[0], x.shape[-1]
    v = x.detach().cpu().float().double().reshape(B, -1, Cc).numpy()
    if xf == XF_NONE:
        return v
    sc = scale.detach().cpu().double()[:, :Cc].numpy()[:, None, :]
    sh = shift.detach().cpu().double()[:, :Cc].numpy()[:, None, :]
    u = v * sc + sh
    return u / (1.0 + np.exp(-u)) if xf == XF_AFFINE_SILU else u


def ref(x: torch.Tensor, scale=None, shift=None, xf: int = XF_NONE):
    """-> dict(cov [C, C], mean [C], S [C], n)"""
    y = y64(x, scale, shift, xf)
    Cc = y.shape[-1]
    K = y[0, 0].copy()
    y = y.reshape(-1, Cc)
    n = y.shape[0]
    mean = y.mean(axis=0)
    z = y - mean
    cov = z.T @ z / (n - 1)
    return dict(cov=cov, mean=mean, S=((y - K) ** 2).sum(axis=0), n=n)


def errors(cov_dev: np.ndarray, mean_dev: np.ndarray, r: dict):
    """(worst |cov_dev - cov| (N - 1) / sqrt(S_c S_c'), worst |mean_dev - mean| / (|mean| + sqrt(S_c / N))); an element whose
    scale is 0 must be exact and counts as 0, else as inf"""
    n, S = r["n"], r["S"]
    den = np.sqrt(S[:, None] * S[None, :])
    num = np.abs(cov_dev - r["cov"]) * (n - 1)
    e = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))
    dm = np.abs(r["mean"]) + np.sqrt(S / n)
    nm = np.abs(mean_dev - r["mean"])
    m = np.where(dm > 0, nm / np.where(dm > 0, dm, 1.0), np.where(nm == 0, 0.0, np.inf))
    return float(e.max()), float(m.max())


def check(got, x, scale=None, shift=None, xf: int = XF_NONE, bar: float = BAR):
    """got = (cov, mean) device tensors; asserts the criterion, the types and the symmetry; -> (cov ratio, mean ratio)"""
    cov, mean = (t.detach().cpu().numpy() for t in got)
    Cc = x.shape[-1]
    assert cov.dtype == np.float64 and mean.dtype == np.float64 and cov.shape == (Cc, Cc) and mean.shape == (Cc,)
    assert np.array_equal(cov.view(np.uint64), cov.T.copy().view(np.uint64)), "cov must be bitwise symmetric"
    r = ref(x, scale, shift, xf)
    e, m = errors(cov, mean, r)
    print(f"chancov C={Cc} n={r['n']} xf={xf} {str(x.dtype)[6:]}: cov error {e:.3e} of sqrt(S S') (bar {bar:.0e}), "
          f"mean error {m:.3e} of |mean| + rms (bar {MEAN_TOL:.0e})")
    assert e <= bar, (e, bar)
    assert m <= MEAN_TOL, (m, MEAN_TOL)
    return e, m


def summary_ref(cov: np.ndarray, thr: float):
    """numpy's view of correlation_summary on a covariance with strictly positive variances"""
    sd = np.sqrt(np.diag(cov))
    rho = cov / np.outer(sd, sd)
    off = np.abs(rho - np.diag(np.diag(rho)))
    ev = np.linalg.eigvalsh(cov)
    return dict(rho=rho, max_abs=off.max(axis=1) if cov.shape[0] > 1 else np.zeros(1), rank=ev.sum() ** 2 / (ev ** 2).sum(),
                pairs=int((np.triu(off, 1) > thr).sum()))
