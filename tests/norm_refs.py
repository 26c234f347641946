"""float64 references, restated host plans and input builders for the GroupNorm / tracker kernels of csrc/norm.hip and the
dead-weight scan of csrc/elementwise.hip (a helper module, not a test).

Every reference is float64 arithmetic on the very fp32 (or bf16-rounded) values the kernel is given.
tests/test_norm_edges_host.py holds each of them, every named shape's property and every builder's stated property to torch
on the CPU, so tests/test_norm_edges_gpu.py rests on references and shapes that were checked without a GPU.

Activations are NHWC ([B, H, W, C], what the kernels read); SHAPES lists them as (B, C, H, W).

Measures, bars and recording are those of tests/streaming_refs.py (rel, bar, check, r16: imported, not copied).  Figures are
recorded under kinds prefixed "norm_edges/"; they pass through streaming_refs.record, which prefixes "streaming_edges/", so
the stored kinds read "streaming_edges/norm_edges/..." (kept as profiles/norm_edges_measured.json).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from streaming_refs import bar, check, r16, rel  # noqa: F401  (the GPU test takes them from here)

G = 32
EPS = 1e-6
KIND = "norm_edges/"

# ---------------------------------------------------------------------------------------------------- host plans, restated
GN_UN = 4                  # norm.hip: quads in flight per thread of gn_bwd_apply_rows_kernel
EW_THREADS = 8192 * 256    # stream_common.h ew_blocks: the capped grid of gn_apply / gn_apply_bf16
GN_GPW = 4                 # norm.hip: groups per workgroup of gn_bwd_final_kernel


def pr_of(C: int) -> int:
    """pixel rows of a workgroup: 256 threads = PR rows x C / 4 channel quads"""
    return 256 // (C // 4)


def stats_plan(B: int, HW: int, C: int):
    """(nchunk, per) of gn_stats / gn_track / gn_bwd_partial: vaehip.ops._gn_nchunk itself, per as the kernels derive it"""
    from vaehip.ops import _gn_nchunk
    n = _gn_nchunk(B, HW, C)
    return n, -(-HW // n)


def row_plan(B: int, HW: int, C: int):
    """(per, nchunk) of vae_gn_bwd_apply: norm.hip row_plan(B, HW, C / 4), restated"""
    PR = pr_of(C)
    per = PR * GN_UN * 4
    while per > PR * GN_UN and B * (-(-HW // per)) < 2048:
        per //= 2
    return per, -(-HW // per)


def final_gy(B: int, nchunk: int, groups: int = G) -> int:
    """grid y of vae_gn_stats_final: 8 workgroups per image for few images with many chunks, else 1"""
    return 8 if (nchunk >= 256 and groups % 8 == 0 and B < 64) else 1


SHAPES = {   # (B, C, H, W)
    "one_pixel": (1, 128, 1, 1),
    "seven_pixels": (3, 128, 1, 7),
    "tail_c256": (2, 256, 3, 3),
    "tail_c512": (1, 512, 5, 7),
    "one_chunk": (2, 128, 8, 16),
    "one_chunk_plus1": (2, 128, 3, 43),
    "ragged_two": (2, 128, 1, 257),
    "last_empty": (2, 512, 33, 33),
    "many_chunks": (2, 512, 91, 91),
    "b65": (65, 128, 2, 2),
    "capped": (40, 128, 64, 64),
    "grid_stride": (2, 128, 257, 257),
}


def _props(B, C, H, W):
    HW, PR = H * W, pr_of(C)
    nchunk, per = stats_plan(B, HW, C)
    rper, rchunk = row_plan(B, HW, C)
    empty = sum(1 for k in range(nchunk) if k * per >= HW)
    last_run = HW - (rchunk - 1) * rper
    return {
        "hw_lt_pr": HW < PR,                                   # most threads hold cnt == 0 and are skipped in the merge
        "one_chunk": nchunk == 1,
        "one_full_chunk": nchunk == 1 and HW == 16 * PR,       # exactly the smallest chunk the plan makes
        "ragged_last": nchunk > 1 and 0 < HW - (nchunk - 1) * per < per,
        "trailing_empty": (nchunk - 1) * per >= HW,
        "several_empty": empty >= 2,
        "gy8": nchunk >= 256 and B < 64 and final_gy(B, nchunk) == 8,
        "b64": B >= 64 and final_gy(B, nchunk) == 1,
        "capped": nchunk == 1024 // B and nchunk < HW // (16 * PR),
        "bwd_tail": HW % (PR * GN_UN) != 0,                    # min(p + u * PR, p1 - 1) clamps inside the last run
        "bwd_short": 0 < last_run < PR * GN_UN,                # ... and that run is shorter than one unrolled pass
        "per_halved": rper < PR * GN_UN * 4,
        "per_halved_once": rper == PR * GN_UN * 2,
        "grid_stride": B * HW * (C // 4) > EW_THREADS and B * HW * (C // 8) > EW_THREADS,
    }


def shape_properties(name: str):
    return _props(*SHAPES[name])


# what each named shape is in the table for (tests/test_norm_edges_host.py asserts every one of them against the plans)
STATED = {
    "one_pixel": ("hw_lt_pr", "one_chunk", "bwd_short"),
    "seven_pixels": ("hw_lt_pr", "one_chunk", "bwd_short"),
    "tail_c256": ("bwd_tail", "bwd_short", "one_chunk", "per_halved"),
    "tail_c512": ("bwd_tail", "bwd_short", "per_halved"),
    "one_chunk": ("one_chunk", "one_full_chunk"),
    "one_chunk_plus1": ("one_chunk", "bwd_tail"),
    "ragged_two": ("ragged_last", "bwd_tail"),
    "last_empty": ("trailing_empty", "bwd_tail"),
    "many_chunks": ("gy8", "trailing_empty", "several_empty", "bwd_tail"),
    "b65": ("b64", "hw_lt_pr"),
    "capped": ("capped", "ragged_last", "per_halved_once"),
    "grid_stride": ("grid_stride",),
}


# ---------------------------------------------------------------------------------------------------- measures
def elem_rel(a, b) -> float:
    """largest per-element relative error (statistics: every (image, group) on its own scale)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b) / b).abs().max())


def scaled_rel(a, b, den, tiny: float = 1e-30) -> float:
    """largest |a - b| / den, entry by entry; `den` broadcasts against the tensors (a channel's own maximum, the absolute sum
    behind a reduction).  Where den is below `tiny` (an activation or derivative that has underflowed to nothing) the entry is
    compared on the scale of the tensor's maximum, not by ratio."""
    a, b, den = a.detach().double().cpu(), b.detach().double().cpu(), den.detach().double().cpu()
    den = torch.where(den >= tiny, den, b.abs().max().clamp_min(tiny))
    return float(((a - b).abs() / den).max())


def chan_max(b) -> torch.Tensor:
    """max |b| per channel of an NHWC tensor, shaped to broadcast against it"""
    return b.detach().double().abs().amax(dim=(0, 1, 2), keepdim=True)


# ---------------------------------------------------------------------------------------------------- GroupNorm references
class GnRef(NamedTuple):
    mean: torch.Tensor    # [B, G]
    rstd: torch.Tensor    # [B, G]
    xhat: torch.Tensor    # [B, H, W, C]
    y: torch.Tensor       # gamma * xhat + beta
    act: torch.Tensor     # silu(y) when silu, else y
    track: torch.Tensor   # [C]: mean |y| over (b, h, w)


class GnBwd(NamedTuple):
    dx: torch.Tensor
    dgamma: torch.Tensor
    dbeta: torch.Tensor
    dgamma_abs: torch.Tensor   # sum |du * xhat| and sum |du| per channel: the scale of what dgamma / dbeta add up
    dbeta_abs: torch.Tensor


def _grouped(x64: torch.Tensor, groups: int):
    B, H, W, C = x64.shape
    return x64.view(B, H * W, groups, C // groups)


def gn_ref64(x, gamma, beta, groups: int = G, eps: float = EPS, silu: bool = False) -> GnRef:
    x64, ga, be = x.detach().cpu().double(), gamma.detach().cpu().double(), beta.detach().cpu().double()
    xg = _grouped(x64, groups)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).view(x64.shape)
    y = xhat * ga + be
    act = y * torch.sigmoid(y) if silu else y
    return GnRef(mean, rstd, xhat, y, act, y.abs().mean(dim=(0, 1, 2)))


def gn_bwd_ref64(x, g, gamma, beta, silu: bool, add=None, groups: int = G, eps: float = EPS, ref: Optional[GnRef] = None) -> GnBwd:
    """the closed form: du = g silu'(y); dbeta = sum du, dgamma = sum du xhat over (b, h, w);
    dx = rstd (gamma du - mean_grp(gamma du) - xhat mean_grp(gamma du xhat)) + add.  ref: gn_ref64 of the same inputs, if at hand"""
    r = ref if ref is not None else gn_ref64(x, gamma, beta, groups, eps, silu)
    ga = gamma.detach().cpu().double()
    du = g.detach().cpu().double()
    if silu:
        s = torch.sigmoid(r.y)
        du = du * (s * (1.0 + r.y * (1.0 - s)))
    t = du * r.xhat
    dy = du * ga
    m1 = _grouped(dy, groups).mean(dim=(1, 3))[:, None, :, None]
    m2 = _grouped(dy * r.xhat, groups).mean(dim=(1, 3))[:, None, :, None]
    dx = ((_grouped(dy, groups) - m1 - _grouped(r.xhat, groups) * m2) * r.rstd[:, None, :, None]).view(du.shape)
    if add is not None:
        dx = dx + add.detach().cpu().double()
    return GnBwd(dx, t.sum(dim=(0, 1, 2)), du.sum(dim=(0, 1, 2)), t.abs().sum(dim=(0, 1, 2)), du.abs().sum(dim=(0, 1, 2)))


def gn_torch(x, gamma, beta, silu: bool, g=None, add=None, dt=torch.float32, groups: int = G, eps: float = EPS):
    """the same by torch itself (F.group_norm, F.silu and autograd) in the precision `dt` on the CPU
    -> y, act, track, dx, dgamma, dbeta (NHWC; the last three None without g).  In fp32 this is the arithmetic whose own distance
    from float64 sets the bars; in float64 it is what the host test holds the references to."""
    xr = x.detach().cpu().to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(g is not None)
    gm = gamma.detach().cpu().to(dt).clone().requires_grad_(g is not None)
    bt = beta.detach().cpu().to(dt).clone().requires_grad_(g is not None)
    y = F.group_norm(xr, groups, gm, bt, eps)
    act = F.silu(y) if silu else y
    track = y.detach().abs().mean(dim=(0, 2, 3))
    dx = dgamma = dbeta = None
    if g is not None:
        act.backward(g.detach().cpu().to(dt).permute(0, 3, 1, 2).contiguous())
        dx = xr.grad.permute(0, 2, 3, 1)
        if add is not None:
            dx = dx + add.detach().cpu().to(dt)
        dgamma, dbeta = gm.grad, bt.grad
    return y.detach().permute(0, 2, 3, 1), act.detach().permute(0, 2, 3, 1), track, dx, dgamma, dbeta


def track_final_ref64(ws, count: int) -> torch.Tensor:
    """column sums of the partials over the exact count (the kernel is handed the fp32 rounding of 1 / count)"""
    return ws.detach().cpu().double().sum(dim=0) / float(count)


# ---------------------------------------------------------------------------------------------------- value builders
class Case(NamedTuple):
    x: torch.Tensor       # [B, H, W, C] fp32
    gamma: torch.Tensor
    beta: torch.Tensor
    g: torch.Tensor       # output gradient
    add: torch.Tensor     # residual-path gradient
    info: dict


def _nhwc(shape):
    B, C, H, W = shape
    return B, H, W, C


def plain_case(name: str, seed: int = 0) -> Case:
    """x ~ N(0.3, 1.7), gamma = 1 + 0.3 N, beta = 0.2 N, g and add ~ N(0, 1)"""
    B, H, W, C = _nhwc(SHAPES[name])
    gen = torch.Generator().manual_seed(1000 * seed + 7 * C + H * W + B)
    x = torch.randn(B, H, W, C, generator=gen) * 1.7 + 0.3
    gamma = 1 + 0.3 * torch.randn(C, generator=gen)
    beta = 0.2 * torch.randn(C, generator=gen)
    g = torch.randn(B, H, W, C, generator=gen)
    add = torch.randn(B, H, W, C, generator=gen)
    return Case(x, gamma, beta, g, add, {})


def large_mean_case(name: str, ratio: float) -> Case:
    """|mean| / std of `ratio` per channel, as test_groupnorm_statistics_with_large_mean builds it: N(0, 1) plus
    ratio (1 + 0.1 N) per channel, gamma = 1, beta = 0"""
    c = plain_case(name, seed=31)
    gen = torch.Generator().manual_seed(31)
    C = c.x.shape[-1]
    x = torch.randn(c.x.shape, generator=gen) + ratio * (1 + 0.1 * torch.randn(C, generator=gen))
    return Case(x, torch.ones(C), torch.zeros(C), c.g, c.add, {"ratio": ratio})


CONST_VALUE = 0.7
CONST_GROUP = 5


def constant_case(name: str) -> Case:
    """plain, but group CONST_GROUP of the last image holds one bit pattern, and (with more than one image) all of image 0
    does: var == 0 there, rstd = 1 / sqrt(eps), xhat == 0, the normalised value is beta, the tracker contribution |beta|"""
    c = plain_case(name, seed=2)
    B, _, _, C = c.x.shape
    cpg = C // G
    x = c.x.clone()
    x[B - 1, :, :, CONST_GROUP * cpg:(CONST_GROUP + 1) * cpg] = CONST_VALUE
    const = [(B - 1, CONST_GROUP)]
    if B > 1:
        x[0] = CONST_VALUE
        const += [(0, grp) for grp in range(G)]
    return Case(x, c.gamma, c.beta, c.g, c.add, {"const": const})


OUTLIER = 1e4


def outlier_case(name: str, where: str) -> Case:
    """N(0, 1) with one value of 1e4 per (image, group).
    first  element 0 of a channel quad at pixel p0 + pr of a chunk (pr < PR): the value thread (pr, quad) reads first and takes
           as the pivot of its shifted sums
    last   element 3 of a quad at the last pixel of a chunk: the last value its thread adds
    info["at"]: the (b, pixel, channel) of every outlier"""
    B, H, W, C = _nhwc(SHAPES[name])
    HW, PR, cpg = H * W, pr_of(C), C // G
    nchunk, per = stats_plan(B, HW, C)
    filled = [k for k in range(nchunk) if k * per < HW]
    gen = torch.Generator().manual_seed(17 + C + HW)
    x = torch.randn(B, H, W, C, generator=gen)
    at = []
    for b in range(B):
        for grp in range(G):
            k = filled[(b + grp) % len(filled)]
            p0, p1 = k * per, min(HW, (k + 1) * per)
            quad = grp % (cpg // 4)
            if where == "first":
                pix, ch = p0 + grp % min(PR, p1 - p0), grp * cpg + 4 * quad
            else:
                pix, ch = p1 - 1, grp * cpg + 4 * quad + 3
            x.view(B, HW, C)[b, pix, ch] = OUTLIER
            at.append((b, pix, ch))
    c = plain_case(name, seed=3)
    return Case(x, c.gamma, c.beta, c.g, c.add, {"at": at})


SILU_PLANTS = (0.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0)   # |u| >= 88: __expf(-u) overflows or flushes to zero
GAMMA_KINDS = ("plain", "negative", "zero")


def silu_case(name: str) -> Case:
    """plain x; of every 32 channels the first 21 carry a planted beta (SILU_PLANTS, once per gamma kind), the rest stay plain.
    gamma kind plain: 1 + 0.3 N, so u = gamma xhat + beta spreads a few units around the plant (and crosses 88);
    negative: -(|1 + 0.3 N|); zero: gamma == 0, u is the plant exactly.
    info["plant"], info["kind"]: per channel, the planted beta (NaN for none) and the index into GAMMA_KINDS (-1 for none)"""
    c = plain_case(name, seed=4)
    C = c.x.shape[-1]
    gamma, beta = c.gamma.clone(), c.beta.clone()
    plant, kind = torch.full((C,), float("nan")), torch.full((C,), -1, dtype=torch.long)
    for ch in range(C):
        slot = ch % 32
        if slot < len(SILU_PLANTS) * len(GAMMA_KINDS):
            plant[ch], kind[ch] = SILU_PLANTS[slot % len(SILU_PLANTS)], slot // len(SILU_PLANTS)
            beta[ch] = plant[ch]
            gamma[ch] = (gamma[ch].abs(), -gamma[ch].abs(), 0.0)[int(kind[ch])]
    return Case(c.x, gamma, beta, c.g, c.add, {"plant": plant, "kind": kind})


def one_hot_case(name: str) -> Case:
    """plain, but g is zero except for one element per image (info["hot"]: its (b, pixel, channel))"""
    c = plain_case(name, seed=5)
    B, H, W, C = c.x.shape
    g = torch.zeros_like(c.g)
    hot = [(b, (7 * b + 3) % (H * W), (37 * b + 5) % C) for b in range(B)]
    for b, pix, ch in hot:
        g.view(B, H * W, C)[b, pix, ch] = 3.0
    return Case(c.x, c.gamma, c.beta, g, c.add, {"hot": hot})


def build_case(name: str, values: str) -> Case:
    if values == "plain":
        return plain_case(name)
    if values.startswith("large_mean_"):
        return large_mean_case(name, float(values.rsplit("_", 1)[1]))
    if values == "constant":
        return constant_case(name)
    if values.startswith("outlier_"):
        return outlier_case(name, values.split("_", 1)[1])
    if values == "silu_range":
        return silu_case(name)
    if values == "one_hot":
        return one_hot_case(name)
    raise KeyError(values)


# ---------------------------------------------------------------------------------------------------- vae_track_final
TRACK_ROWS = (1, 255, 256, 257, 1000)
TRACK_C = (3, 8, 128, 130)


def track_ws(rows: int, C: int) -> torch.Tensor:
    """non-negative partials spanning 1e-6 .. 1e3 (log-uniform)"""
    gen = torch.Generator().manual_seed(rows * 131 + C)
    return torch.exp(torch.rand(rows, C, generator=gen) * math.log(1e9) + math.log(1e-6))


# ---------------------------------------------------------------------------------------------------- dead-weight scan
DEAD_CHUNK = 32768
DEAD_THR = 1e-5
DEAD_LENGTHS = (1, 3, 4, 5, 32767, 32768, 32769, 2 * 32768 + 7)


def f32(v: float) -> float:
    return float(np.float32(v))


def dead_plants(thr: float):
    """values around the strict `<`: exactly thr and -thr (not counted), the fp32 number just below thr (counted), its
    negative, -0.0 and a denormal (counted)"""
    t = np.float32(thr)
    below = np.nextafter(t, np.float32(0.0))
    return [float(t), float(below), float(-t), -0.0, 1e-40, float(-below)]


def dead_layout(gap_fill: float, seed: int = 0, thr: float = DEAD_THR):
    """a flat fp32 buffer holding 16 segments with gaps between them, before the first and after the last: every length of
    DEAD_LENGTHS once with its start on a 16-byte boundary of the buffer (float4 body) and once one element past one
    (scalar path).  Gaps hold `gap_fill` (0.0: counted if a bound is off by one; NaN: poisons a sum that reaches into them).
    Inside: 0.05 N(0, 1), with dead_plants cycling over the first element, the last, and both sides of every chunk boundary;
    +inf at element 2 of the segments listed in info["inf"]; a NaN at element 1 of segment info["nan"] alone.
    -> flat, segments [(begin, end)], info"""
    gen = torch.Generator().manual_seed(100 + seed)
    order = [(L, odd) for odd in (0, 1) for L in DEAD_LENGTHS]
    order = order[::3] + order[1::3] + order[2::3]   # lengths mixed: the bisection does not meet them sorted
    segs, off = [], 4
    for L, odd in order:
        begin = (off + 3) // 4 * 4 + 4 + odd
        segs.append((begin, begin + L))
        off = begin + L
    flat = torch.full((off + 8,), float(gap_fill))
    plants = dead_plants(thr)
    info = {"inf": [], "nan": None, "planted": []}
    for s, (b, e) in enumerate(segs):
        L = e - b
        flat[b:e] = torch.randn(L, generator=gen) * 0.05
        pos = sorted({p for p in (0, L - 1, DEAD_CHUNK - 1, DEAD_CHUNK, 2 * DEAD_CHUNK - 1, 2 * DEAD_CHUNK) if 0 <= p < L})
        for i, p in enumerate(pos):
            flat[b + p] = plants[(i + s) % len(plants)]
            info["planted"].append((s, p, plants[(i + s) % len(plants)]))
        if L >= 5 and s % 3 == 0:
            flat[b + 2] = float("inf")
            info["inf"].append(s)
        if L == DEAD_CHUNK + 1 and (b % 4) == 1:
            flat[b + 1] = float("nan")
            info["nan"] = s
    return flat, segs, info


def dead_chunk0(segs):
    """seg_chunk0 as DeadNeuronTracker._scan_arena lays it out: prefix sum of max(1, ceil(len / DEAD_CHUNK))"""
    return np.concatenate([[0], np.cumsum([max(1, -(-(e - b) // DEAD_CHUNK)) for b, e in segs])]).astype(np.int32)


def dead_counts(flat, segs, thr: float, athr=None, use_fixed: bool = True):
    """per segment: the exact count of |w| < thr (athr None), or of |w| < athr[s] (and < thr when use_fixed), as the fp32
    comparisons they are; and the float64 sum of |w|"""
    t = np.float32(thr)
    counts, sums = [], []
    for s, (b, e) in enumerate(segs):
        a = flat[b:e].detach().cpu().abs().numpy()
        if athr is None:
            m = a < t
        else:
            m = a < np.float32(athr[s])
            if use_fixed:
                m &= a < t
        counts.append(int(m.sum()))
        sums.append(float(a.astype(np.float64).sum()))
    return counts, sums


def dead_ref(flat, segs, thr: float, mean_percentage: float, mode: str):
    """counts and sum |w| per segment, and the percentages by DeadNeuronTracker's formulas (smaller_than_threshold,
    percent_of_mean, both): the mean of |w| is the float64 sum over the count, rounded to fp32 as `.mean().item()` is; below
    1e-9 it is degenerate (percent_of_mean: 100 if every |w| < 1e-9 else 0; both: |w| < thr and |w| < 1e-9)
    -> dict(counts, abssum, pct, athr, margin); margin: the smallest relative distance of a |w| from its adaptive threshold"""
    counts, sums = dead_counts(flat, segs, thr)
    n = [e - b for b, e in segs]
    mean_abs = [f32(s / k) if k else 0.0 for s, k in zip(sums, n)]
    degenerate = [abs(m) < 1e-9 for m in mean_abs]
    athr = [1e-9 if d else mean_percentage * m for d, m in zip(degenerate, mean_abs)]
    margin = math.inf
    for (b, e), t, d in zip(segs, athr, degenerate):
        if e > b and not d:
            a = flat[b:e].detach().cpu().abs().double()
            margin = min(margin, float(((a - f32(t)).abs() / f32(t)).min()))
    if mode == "threshold":
        pct = [c / k * 100.0 if k else 0.0 for c, k in zip(counts, n)]
    elif mode == "percent_of_mean":
        ac, _ = dead_counts(flat, segs, thr, athr, use_fixed=False)
        pct = [0.0 if not k else ((100.0 if c == k else 0.0) if d else c / k * 100.0) for c, k, d in zip(ac, n, degenerate)]
    elif mode == "both":
        ac, _ = dead_counts(flat, segs, thr, athr, use_fixed=True)
        pct = [c / k * 100.0 if k else 0.0 for c, k in zip(ac, n)]
    else:
        raise KeyError(mode)
    return {"counts": counts, "abssum": sums, "pct": pct, "athr": athr, "margin": margin}


# the tracker on the synthetic model's arena: what is planted where (names of the synthetic SDXL VAE)
TRACKER_SEED = 42
TRACKER_THR, TRACKER_MEAN_PCT = 1e-5, 0.1
PLANT_ZERO_BIAS = "decoder.mid_block.attentions.0.to_q.bias"        # all zero: degenerate, reports 100 %
PLANT_TINY_BIAS = "encoder.mid_block.attentions.0.to_v.bias"        # all 5e-10: degenerate
PLANT_ONE_VALUE = "encoder.conv_out.bias"                           # one non-zero value: mean |w| >= 1e-9, not degenerate
PLANT_LARGE_CONV = "decoder.up_blocks.0.resnets.0.conv1.weight"     # zeros in its first and last 100 elements in memory
PLANT_BETWEEN = "decoder.up_blocks.0.resnets.0.conv1.bias"          # small, between two large conv weights in the arena


def plant_tracker_params(params) -> None:
    """`params`: name -> tensor of logical shape (CPU tensors of a state dict, or the live parameters of the arena model,
    whose conv weights are OHWI in memory).  Edits them in place."""
    with torch.no_grad():
        params[PLANT_ZERO_BIAS].zero_()
        params[PLANT_TINY_BIAS].fill_(5e-10)
        one = params[PLANT_ONE_VALUE]
        one.zero_()
        one[3] = 1e-3
        w = params[PLANT_LARGE_CONV]
        q = w.detach().permute(0, 2, 3, 1).contiguous().view(-1)   # the arena's memory order
        q[:100] = 0.0
        q[-100:] = 0.0
        w.copy_(q.view(w.shape[0], w.shape[2], w.shape[3], w.shape[1]).permute(0, 3, 1, 2))
        params[PLANT_BETWEEN][::2] = 0.0
