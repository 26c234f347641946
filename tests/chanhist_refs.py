"""References for the per-channel magnitude histogram, near-zero count and max |y| (ops.chanhist, csrc/chanhist.hip; the hook
path's formulas in tracking/monitor.py) -- a helper module, not a test.

* ref_exact: the three results of an untransformed NHWC tensor, bins from the bit pattern of the fp32 value (numpy on the host).
* ref_transformed / count_bounds: for y = XF(x) the value in float64 with an error radius per element, and from them the counts
  every correct fp32 evaluation must lie between.
"""
import numpy as np
import torch

BINS = 48
XF_NONE, XF_AFFINE, XF_AFFINE_SILU = 0, 1, 2


def _f32(v):
    return np.float32(v)


def _below(v):
    return np.nextafter(_f32(v), _f32(0))


def _above(v):
    return np.nextafter(_f32(v), _f32(np.inf))


# (value, bin): bin = clamp(floor(log2 |y|) + 31, 0, 47).  The negative of every finite value follows its positive.
_POS = [(_f32(0.0), 0), (_f32(1e-40), 0),                 # zero, a denormal
        (_below(2.0 ** -30), 0), (_f32(2.0 ** -30), 1),   # the first edge
        (_f32(1.0), 31), (_f32(65504.0), 46),             # one; the largest fp16 number
        (_below(2.0 ** 16), 46), (_f32(2.0 ** 16), 47)]   # the last edge: what fp16 cannot hold
EDGES = [(v, b) for v, b in _POS] + [(-v, b) for v, b in _POS] + [(_f32(np.inf), 47), (_f32(-np.inf), 47), (_f32(np.nan), 47)]


def edge_values() -> torch.Tensor:
    return torch.from_numpy(np.array([v for v, _ in EDGES], dtype=np.float32))


def tau_edge_values(tau: float) -> torch.Tensor:
    """just below tau, tau, just above tau (as fp32), and their negatives: near zero are the first and the fourth only"""
    t = _f32(tau)
    vals = [_below(t), t, _above(t)]
    return torch.from_numpy(np.array(vals + [-v for v in vals], dtype=np.float32))


def bits_bin(y32: np.ndarray) -> np.ndarray:
    """bin of every fp32 value from its exponent field"""
    e = ((np.ascontiguousarray(y32, dtype=np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    return np.clip(e - 96, 0, BINS - 1)


def _hist(bins: np.ndarray, keep=None) -> np.ndarray:
    """[N, C] bins -> [C, 48] counts of the elements where keep (default: all)"""
    Cc = bins.shape[1]
    idx = bins + np.arange(Cc, dtype=np.int64)[None, :] * BINS
    if keep is not None:
        idx = idx[keep]
    return np.bincount(idx.reshape(-1), minlength=Cc * BINS).reshape(Cc, BINS).astype(np.int64)


def ref_exact(x: torch.Tensor, tau: float = 1e-3):
    """x: NHWC (any device, fp32 or bf16, a channel-prefix view allowed) -> (hist int64 [C, 48], nzero int64 [C], absmax fp32 [C])"""
    y = x.detach().cpu().float().reshape(-1, x.shape[-1]).contiguous().numpy()
    a = np.abs(y)
    with np.errstate(invalid="ignore"):
        nz = (a < _f32(tau)).sum(axis=0).astype(np.int64)  # NaN compares false
        amax = a.max(axis=0)                                # NaN propagates
    return _hist(bits_bin(y)), nz, amax


def stats_rows(B: int, ld: int, seed: int):
    """the moments suite's GroupNorm rows: scale in [0.25, 1.75], shift ~ 0.5 N(0, 1); CPU tensors [B, ld]"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sc = torch.rand((B, ld), generator=g) * 1.5 + 0.25
    sh = torch.randn((B, ld), generator=g) * 0.5
    return sc, sh


def ref_transformed(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, xf: int):
    """float64 y = XF(x) [N, C] and the radius d [N, C] an fp32 evaluation stays within: for the affine
    du = 2^-21 (|x scale| + |shift|) (one rounding per product and per sum), with SiLU d = 1.1 du + 2^-20 |y| (a few ulp for
    exp and rcp), without d = du"""
    B, Cc = x.shape[0], x.shape[-1]
    x64 = x.detach().cpu().float().double().reshape(B, -1, Cc).numpy()
    sc = scale.detach().cpu().double()[:, :Cc].numpy()[:, None, :]
    sh = shift.detach().cpu().double()[:, :Cc].numpy()[:, None, :]
    u = x64 * sc + sh
    du = 2.0 ** -21 * (np.abs(x64 * sc) + np.abs(sh))
    if xf == XF_AFFINE_SILU:
        y = u / (1.0 + np.exp(-u))
        d = 1.1 * du + 2.0 ** -20 * np.abs(y)
    else:
        assert xf == XF_AFFINE
        y, d = u, du
    return y.reshape(-1, Cc), d.reshape(-1, Cc)


def real_bin(a: np.ndarray) -> np.ndarray:
    """bin of a non-negative real number (float64)"""
    _, e = np.frexp(a)  # a = m 2^e with m in [0.5, 1): floor(log2 a) = e - 1
    b = np.clip(e.astype(np.int64) - 1 + 31, 0, BINS - 1)
    b = np.where(a < 2.0 ** -30, 0, b)
    return np.where(np.isfinite(a), b, BINS - 1)


def count_bounds(y: np.ndarray, d: np.ndarray, tau: float):
    """what is certain about the counts of values known to within d.  An element is uncertain for the histogram when |y - d|
    and |y + d| (0 if the interval holds it) fall in different bins, and for the near-zero count when they fall on different
    sides of tau.  -> dict: hist_lo [C, 48] (elements certain of their bin), hist_unc [C, 48] (uncertain elements, counted in
    every bin their interval reaches), nz_lo [C], nz_unc [C], uncertain (elements uncertain for either count), n"""
    lo, hi = y - d, y + d
    alo = np.where((lo <= 0) & (hi >= 0), 0.0, np.minimum(np.abs(lo), np.abs(hi)))
    ahi = np.maximum(np.abs(lo), np.abs(hi))
    blo, bhi = real_bin(alo), real_bin(ahi)
    unc_b = blo != bhi
    Cc = y.shape[1]
    hist_lo = _hist(blo, ~unc_b)
    hist_unc = np.zeros((Cc, BINS), dtype=np.int64)
    for n, c in zip(*np.nonzero(unc_b)):
        hist_unc[c, blo[n, c]:bhi[n, c] + 1] += 1
    t = float(_f32(tau))
    nz_sure = ahi < t
    nz_unc = (alo < t) & ~nz_sure
    return dict(hist_lo=hist_lo, hist_unc=hist_unc, nz_lo=nz_sure.sum(axis=0).astype(np.int64),
                nz_unc=nz_unc.sum(axis=0).astype(np.int64), uncertain=int((unc_b | nz_unc).sum()), n=int(y.size))


def check_within_bounds(hist, nzero, absmax, y, d, tau, n_rows):
    """the device's (hist, nzero, absmax) as numpy arrays against count_bounds(y, d, tau); -> the bounds (for the shared tally)"""
    bd = count_bounds(y, d, tau)
    assert (hist.sum(axis=1) == n_rows).all(), "histogram rows must sum to B * H * W exactly"
    assert (bd["hist_lo"] <= hist).all() and (hist <= bd["hist_lo"] + bd["hist_unc"]).all(), \
        np.argwhere((bd["hist_lo"] > hist) | (hist > bd["hist_lo"] + bd["hist_unc"]))[:8]
    assert (bd["nz_lo"] <= nzero).all() and (nzero <= bd["nz_lo"] + bd["nz_unc"]).all()
    k = np.abs(y).argmax(axis=0)
    cols = np.arange(y.shape[1])
    err = np.abs(absmax.astype(np.float64) - np.abs(y[k, cols]))
    assert (err <= d[k, cols]).all(), (err.max(), d[k, cols].min())
    return bd


# The edges of the frame the statistics partial passes share (csrc/chanstat_common.h), as (C, B, H, W, layout): a narrow tile of 128
# pixel rows whose four-in-flight loop and tail both run; a second channel tile of one unit of four channels (tiles of 256
# channels: C = 260, chanhist's 128: C = 132 -- 33 units, 7 pixel rows, elsewhere); the scalar path; the view buf[..., :C] of a buffer
# four channels wider; a base one element off, which puts C % 4 == 0 on the scalar path.
FRAME_CASES = [(8, 2, 24, 24, "plain"), (260, 2, 9, 7, "plain"), (132, 2, 9, 7, "plain"), (3, 1, 5, 5, "plain"),
               (8, 2, 24, 24, "prefix"), (8, 2, 24, 24, "offset")]


def frame_params(xfs=(0,)):
    """FRAME_CASES x storage x transform; a base one element off has no transform (the statistics' rows start at the buffer's)"""
    return [c + (dt, xf) for c in FRAME_CASES for dt in (torch.float32, torch.bfloat16) for xf in xfs if not (xf and c[4] == "offset")]


def frame_layout(t: torch.Tensor, layout: str) -> torch.Tensor:
    """the values of t [B, H, W, C] in the layout of a FRAME_CASES entry; what lies around a view is 1e6"""
    Cc = t.shape[3]
    if layout == "prefix":
        buf = torch.full(tuple(t.shape[:3]) + (Cc + 4,), 1e6, device=t.device, dtype=t.dtype)
        buf[..., :Cc] = t
        return buf[..., :Cc]
    if layout == "offset":
        flat = torch.full((t.numel() + 1,), 1e6, device=t.device, dtype=t.dtype)
        flat[1:] = t.reshape(-1)
        return flat[1:].view(t.shape)
    return t
