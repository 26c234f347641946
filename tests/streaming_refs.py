"""float64 references and input builders for the step's streaming kernels and its attention (a helper module, not a test).

Every reference is float64 arithmetic on the very fp32 (or bf16) values the kernel is given; tests/test_streaming_edges_host.py
holds each of them, and each builder's stated properties, to torch on the CPU, so the GPU tests
(tests/test_streaming_edges_gpu.py, tests/test_attention_gpu.py) rest on references that were checked without a GPU.

Bars of the kind "k x fp32-CPU" are derived here too: the same formula evaluated by torch in fp32 on the CPU, its error
against the float64 reference, times k, with a floor.  A bar never depends on what the kernel under test returns.
"""
from __future__ import annotations

import functools
import math

import torch


# ---------------------------------------------------------------------------------------------------- measures, recording
def rel(a, b) -> float:
    """tensor-relative error: max |a - b| / max |b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def rel_to(a, b, scale: float) -> float:
    """max |a - b| on a scale given from outside (for references that are about zero)"""
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max() / scale)


def row_rel(a, b, den) -> torch.Tensor:
    """per row: max |a - b| / max |den|   (rows = all but the last dimension)"""
    a, b, den = a.detach().double().cpu(), b.detach().double().cpu(), den.detach().double().cpu()
    return (a - b).abs().amax(-1) / (den.abs().amax(-1) + 1e-300)


def bar(k: float, fp32_cpu: float, floor: float) -> float:
    return max(k * fp32_cpu, floor)


def record(kind: str, key: str, value) -> None:
    """measured figures of this run, kept the way tests/test_engine_gpu.py keeps its parity figures (same file, kinds prefixed
    "streaming_edges/"; collected into profiles/streaming_edges_measured.json); nothing is written where that test writes nothing"""
    from test_engine_gpu import _record
    _record("streaming_edges/" + kind, key, value)


def check(kind: str, key: str, measured: float, limit: float, fp32_cpu=None, strict: bool = True) -> None:
    """print and record the kernel's figure next to its bar, then assert it"""
    entry = {"measured": measured, "bar": limit}
    if fp32_cpu is not None:
        entry["fp32_cpu"] = fp32_cpu
    print(f"{kind} {key}: measured {measured:.3e} bar {limit:.3e}" + ("" if fp32_cpu is None else f" (fp32 CPU {fp32_cpu:.3e})"))
    record(kind, key, entry)
    ok = measured < limit if strict else measured <= limit
    assert ok and not math.isnan(measured), (kind, key, entry)


def r16(t: torch.Tensor) -> torch.Tensor:
    """the fp32 tensor with every value rounded to bf16 (what a bf16 kernel multiplies)"""
    return t.bfloat16().float()


# ---------------------------------------------------------------------------------------------------- clip + AdamW, sqnorm
ADAM = dict(betas=(0.9, 0.999), eps=1e-8, wd=1e-2)
ADAM_N = 100003
ADAM_STEPS = [(0.0, 3.0), (1e-3, 1e-3), (5e-4, 3.0), (1e-3, 1e-5), (1e-3, 3.0)]   # (lr, gradient scale) of steps 1..5
ADAM_BAND = slice(0, 3000)   # g == 0 | |g| ~ 1e-8: sqrt(v) is of the size of eps, so eps decides the update
ADAM_GRID_N = 8192 * 256 * 4 + 1203   # more float4s than the capped grid has threads (grid-stride trips), and a 3-element tail


def adam_params(n: int, seed: int = 3) -> torch.Tensor:
    """weights of the size real layers have (0.05 N(0,1)): an update of lr = 1e-3 is then 1e-2 of a value, not 2e-4"""
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.05


def adam_grad(n: int, scale: float, seed: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(n, generator=gen) * scale
    if n >= 3000:
        g[:1000] = 0.0
        g[1000:3000] = torch.randn(2000, generator=gen) * 1e-8
    return g


def sqnorm_ref64(g: torch.Tensor) -> float:
    return float((g.double().cpu() ** 2).sum())


def clip_coef64(sqnorm64: float, max_norm: float) -> float:
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); no clipping for max_norm <= 0"""
    return min(1.0, max_norm / (math.sqrt(sqnorm64) + 1e-6)) if max_norm > 0 else 1.0


def adamw_ref64(p, g, m, v, sqnorm64, max_norm, lr, betas, eps, wd, step):
    """one clip_grad_norm_(max_norm) + torch.optim.AdamW step in float64 from fp32 state -> (p, m, v) float64"""
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    b1, b2 = betas
    gg = g * clip_coef64(sqnorm64, max_norm)
    m2 = m + (gg - m) * (1.0 - b1)
    v2 = v * b2 + (1.0 - b2) * gg * gg
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    den = v2.sqrt() / math.sqrt(bc2) + eps
    return p * (1.0 - lr * wd) - (lr / bc1) * (m2 / den), m2, v2


def adamw_torch32(p, g, m, v, max_norm, lr, betas, eps, wd, step):
    """the same step by torch itself in fp32 on the CPU (clip_grad_norm_ + torch.optim.AdamW, state injected) -> (p, m, v):
    the arithmetic whose own distance from float64 sets the bars"""
    pr = torch.nn.Parameter(p.detach().float().cpu().clone())
    opt = torch.optim.AdamW([pr], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[pr] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.detach().float().cpu().clone(),
                     "exp_avg_sq": v.detach().float().cpu().clone()}
    pr.grad = g.detach().float().cpu().clone()
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_([pr], max_norm)
    opt.step()
    st = opt.state[pr]
    return pr.detach(), st["exp_avg"], st["exp_avg_sq"]


def update_error(p, p64, p_prev, sl=slice(None)) -> float:
    """E = max |p - p64| / max |p64 - p_prev|: the error on the scale of the UPDATE.  A step that must leave p alone (lr = 0)
    has E = 0 when it did, inf otherwise."""
    p, p64, p_prev = (t.detach().double().cpu()[sl] for t in (p, p64, p_prev))
    err, d = float((p - p64).abs().max()), float((p64 - p_prev).abs().max())
    if d == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return err / d


# ---------------------------------------------------------------------------------------------------- bf16 rounding table
BF16_HI = (0x3f80, 0x3f81, 0x0080, 0x0001, 0x0000, 0x7f7f, 0x7f00, 0x8000, 0xbf80, 0x0040, 0xff7f)
BF16_LO = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)
BF16_SPECIAL = (0x7f800000, 0xff800000, 0x7fc00000)   # +inf, -inf, one NaN
BF16_LENGTHS = (1, 7, 8, 9, 66, 1031)


def f32_from_bits(bits) -> torch.Tensor:
    return torch.tensor(list(bits), dtype=torch.int64).to(torch.int32).view(torch.float32)


def bits_of_f32(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().contiguous().view(torch.int32).to(torch.int64) & 0xffffffff


def bf16_from_bits(bits) -> torch.Tensor:
    return torch.tensor(list(bits), dtype=torch.int64).to(torch.int16).view(torch.bfloat16)


def bits_of_bf16(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xffff


def bf16_table_bits():
    """fp32 bit patterns around every rounding decision: exact, just above exact, just below / at / just above the tie, all
    ones, under bf16 values with an even and an odd last bit, normal, smallest normal, subnormal, zero, largest finite"""
    return [(hi << 16) | lo for hi in BF16_HI for lo in BF16_LO] + list(BF16_SPECIAL)


def rne_bf16_bits(u: torch.Tensor) -> torch.Tensor:
    """round to nearest even on the integer pattern of a non-NaN fp32 value (int64 tensor of patterns)"""
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff


def bf16_table(n: int, rot: int = 0) -> torch.Tensor:
    """the table, starting at entry `rot`, repeated to length n (69 entries: odd, so over 8 x 69 elements every entry meets
    every lane of an 8-wide body)"""
    t = bf16_table_bits()
    return f32_from_bits(t[(rot + i) % len(t)] for i in range(n))


def bf16_rotations(n: int):
    """rotations of the table such that the launches of length n see every entry between them"""
    return range(0, len(bf16_table_bits()), n)


def same_bf16(got: torch.Tensor, want: torch.Tensor) -> bool:
    """bit for bit, except that a NaN only has to be a NaN"""
    g, w = bits_of_bf16(got), bits_of_bf16(want)
    nan = want.detach().cpu().float().isnan()
    return bool(torch.equal(g[~nan], w[~nan])) and bool(got.detach().cpu().float()[nan].isnan().all())


def bf16_add_pairs():
    """bf16 pairs (a, b) as bit patterns, a multiple of 4 of them.  The fp32 sum of two bf16 numbers is exact unless their
    exponents lie more than 16 apart, so the sum reaches the bf16 rounding either exactly (ties, and the nearest
    representable neighbours of ties) or already rounded once to fp32 (the far-apart pairs, where the result is rounded
    twice: a kernel that keeps or drops the wrong sticky bit shows there); overflow, subnormals and cancellation follow."""
    pairs = [
        (0x3f80, 0x3b80), (0x3f81, 0x3b80),   # 1 + 2^-8, (1 + 2^-7) + 2^-8: ties, to the even value below / above
        (0x3f80, 0xbb00), (0x3f81, 0xbb80),   # 1 - 2^-9 (tie in the binade below), (1 + 2^-7) - 2^-8
        (0x3f80, 0x3b81), (0x3f80, 0x3b7f),   # a tie + 2^-15, a tie - 2^-16
        (0x3f81, 0x3b81), (0x3f81, 0x3b7f),
        (0x437f, 0x4000), (0x437f, 0x4040),   # 255 + 2 = 257: tie after a carry; 255 + 3
        (0x3f80, 0x3380), (0x3f80, 0x32ff), (0x3f80, 0xb2ff), (0x3f81, 0x3300),   # fp32 sum inexact: rounded twice
        (0x3f80, 0x3300), (0x3f80, 0xb300), (0x3f80, 0xb380), (0x4b00, 0x3f00),   # 1 +- 2^-25 / 2^-24; 2^23 + 0.5 (fp32 tie)
        (0x7f7f, 0x7f7f), (0x7f7f, 0x7b00), (0x7f7f, 0x7aff), (0xff7f, 0xfb00),   # overflow; a tie at the largest finite
        (0x0001, 0x0001), (0x0080, 0x807f), (0x0040, 0x0040), (0x0001, 0x8001),   # subnormal sums, x - x = +0
        (0x0000, 0x8000), (0x8000, 0x8000), (0x7f80, 0x3f80), (0x7f80, 0xff80),   # signed zeros, inf + 1, inf - inf = NaN
        (0x7fc0, 0x3f80), (0x0080, 0x0080), (0x3f80, 0xbf80), (0x00ff, 0x0001),
        (0x3f80, 0x3c00), (0x3f81, 0x3c00),   # exact sums
    ]
    gen = torch.Generator().manual_seed(16)
    ra = torch.randint(0, 0x10000, (4096,), generator=gen).tolist()   # any pattern: every exponent gap, NaNs and infs too
    rb = torch.randint(0, 0x10000, (4096,), generator=gen).tolist()
    rc = torch.randint(-3, 4, (4096,), generator=gen).tolist()        # and pairs of nearby exponents (ties are frequent there)
    near = [((a & 0x807f) | (0x3f80 + (c << 7)), b) for a, b, c in zip(ra, [(x & 0x807f) | 0x3f80 for x in rb], rc)]
    pairs = pairs + list(zip(ra, rb)) + near
    assert len(pairs) % 4 == 0
    return bf16_from_bits(p[0] for p in pairs), bf16_from_bits(p[1] for p in pairs)


# ---------------------------------------------------------------------------------------------------- softmax
SOFTMAX_COLS = (1, 25, 63, 64, 65, 255, 256, 257, 1024, 4032)
SOFTMAX_ROWS = ("n3", "n3_plus_1e4", "n90", "one_hot", "every_second_minus_inf")


def softmax_inputs(cols: int):
    """five rows (SOFTMAX_ROWS; a single column cannot hold a -inf next to a finite value: its fifth row stays N(0,3)) and a
    dP for them"""
    gen = torch.Generator().manual_seed(cols)
    S = torch.randn(5, cols, generator=gen) * 3
    S[1] = S[0] + 1e4
    S[2] = torch.randn(cols, generator=gen) * 90
    S[3] = -1e30
    S[3, cols // 2] = 0.0
    if cols > 1:
        S[4, ::2] = float("-inf")
    dP = torch.randn(5, cols, generator=gen)
    return S, dP


def softmax_ref(S: torch.Tensor, dt=torch.float64) -> torch.Tensor:
    return torch.softmax(S.to(dt), -1)


def softmax_bwd_ref(P: torch.Tensor, dP: torch.Tensor, dt=torch.float64) -> torch.Tensor:
    P, dP = P.to(dt), dP.to(dt)
    return P * (dP - (P * dP).sum(-1, keepdim=True))


# ---------------------------------------------------------------------------------------------------- sample + KL, MSE
SAMPLE_SHAPES = ((3, 5, 5, 4), (2, 16, 16, 4), (3, 10, 25, 4))   # hw * L = 100 (part of one block), 1024 (4 whole), 1000 (3 + a part)
LV_PLANTS = (-30.0, 20.0, -30.5, 20.5, 19.99)    # at the clamp bounds (gradient passes), beyond them (gradient 0), just inside


def sample_inputs(B, h, w, L, planted: bool):
    """moments [B,h,w,2L] (NHWC: mean | log-variance), eps, dz [B,h,w,L], and the mask of planted log-variances: the first
    pixels of image 0 and the last pixels of the last image (the last, partial block)"""
    gen = torch.Generator().manual_seed(B * 1000 + h * w)
    mom = torch.randn(B, h, w, 2 * L, generator=gen) * 2
    eps = torch.randn(B, h, w, L, generator=gen)
    dz = torch.randn(B, h, w, L, generator=gen)
    mask = torch.zeros(B, h * w, 2 * L, dtype=torch.bool)
    if planted:
        flat = mom.view(B, h * w, 2 * L)
        for i, val in enumerate(LV_PLANTS):
            for b, pix, l in ((0, i, i % L), (B - 1, h * w - 1 - i, (i + 1) % L)):
                flat[b, pix, L + l] = val
                mask[b, pix, :] = True
    return mom, eps, dz, mask.view(B, h, w, 2 * L)


def sample_kl_ref(mom, eps, dt=torch.float64):
    """-> z [B,h,w,L], kl [B] (0.5 sum(mu^2 + var - 1 - logvar) over the image, log-variance clamped to [-30, 20])"""
    mom = mom.to(dt)
    L = mom.shape[-1] // 2
    mu, lv = mom[..., :L], mom[..., L:].clamp(-30.0, 20.0)
    z = mu if eps is None else mu + torch.exp(0.5 * lv) * eps.to(dt)
    kl = 0.5 * (mu * mu + torch.exp(lv) - 1.0 - lv).sum(dim=(1, 2, 3))
    return z, kl


def sample_kl_bwd_ref(mom, eps, dz, klw: float, dt=torch.float64):
    """gradient of sum(z * dz) + klw * mean_b(kl) with respect to the moments; the clamp passes the gradient AT its bounds"""
    mom = mom.to(dt)
    B, L = mom.shape[0], mom.shape[-1] // 2
    mu, lvr = mom[..., :L], mom[..., L:]
    lv = lvr.clamp(-30.0, 20.0)
    g = torch.zeros_like(mu) if dz is None else dz.to(dt)
    e = torch.zeros_like(mu) if eps is None else eps.to(dt)
    dlv = g * e * 0.5 * torch.exp(0.5 * lv) + (klw / B) * 0.5 * (torch.exp(lv) - 1.0)
    dlv = torch.where((lvr >= -30.0) & (lvr <= 20.0), dlv, torch.zeros_like(dlv))
    return torch.cat([g + (klw / B) * mu, dlv], dim=-1)


MSE_SIZES = (7, 4097, 3 * 3 * 40 * 40)


def mse_inputs(n: int):
    gen = torch.Generator().manual_seed(n)
    recon, target = torch.randn(n, generator=gen), torch.rand(n, generator=gen) * 2 - 1
    klp = torch.rand(3, 2, generator=gen) * 50 + 1
    return recon, target, klp


def loss_ref(recon, target, klp, klw: float, dt=torch.float64) -> torch.Tensor:
    """[mse mean, kl mean over the images, mse + klw * kl]"""
    d = recon.to(dt) - target.to(dt)
    mse, kl = (d * d).sum() / d.numel(), klp.to(dt).sum() / klp.shape[0]
    return torch.stack([mse, kl, mse + klw * kl])


# ---------------------------------------------------------------------------------------------------- attention
ATTN_C = 512
ATTN_SCALE = ATTN_C ** -0.5
ATTN_T = (64, 192, 576)            # 1, 3 and 9 row blocks of 64: one block, an odd count, several
ATTN_MATERIALISED_T = (25, 36, 49, 64, 100, 225)   # (R / 8)^2 tokens at R = 40, 48, 56, 64, 80, 120
ATTN_PLACEMENTS = ("first", "last", "scattered")
ATTN_CASES = ("plain",) + tuple(f"{w}_g{g}" for w in ATTN_PLACEMENTS for g in (12, 40)) + ("shift", "uniform")


def attention_ref(q, k, v, do, scale, dt=torch.float64):
    """-> o, row log-sum-exp, dq, dk, dv, P of softmax(scale q k^T) v in the precision `dt` on the CPU"""
    q, k, v = (t.detach().cpu().to(dt).clone().requires_grad_(True) for t in (q, k, v))
    s = torch.bmm(q, k.transpose(1, 2)) * scale
    p = torch.softmax(s, dim=-1)
    o = torch.bmm(p, v)
    o.backward(do.detach().cpu().to(dt))
    return o.detach(), torch.logsumexp(s, dim=-1).detach(), q.grad, k.grad, v.grad, p.detach()


def planted_column(T: int, where: str) -> torch.Tensor:
    i = torch.arange(T)
    return {"first": i % 32, "last": T - 32 + i % 32, "scattered": (37 * i + 5) % T}[where]


def attn_inputs(case: str, T: int, B: int = 2):
    """q, k, v, do [B,T,512] fp32, scaled (2, 2, 1, 1) as the existing attention tests: scores with a spread of several units.
    plain      iid Gaussian
    <where>_g<g>  q_i += g k_j / (scale |k_j|^2): score (i, j(i)) rises by g.  j(i) lies in the first streamed block of 32 keys
               (every later block leaves the running maximum alone), in the last one (everything accumulated before is rescaled
               by about e^-g) or anywhere.  g = 12: the planted entry holds most of the row; g = 40: the row is one-hot
    shift      q += 2 sqrt(512) c, k += 2 sqrt(512) c for a unit vector c: every score rises by about 90, past exp's fp32 range
    uniform    every 7th query is zero: its row of P is exactly uniform, its log-sum-exp log T, its output the mean of v"""
    gen = torch.Generator().manual_seed(T)
    q, k, v, do = (torch.randn(B, T, ATTN_C, generator=gen) * s for s in (2.0, 2.0, 1.0, 1.0))
    if case == "plain":
        pass
    elif case == "shift":
        c = torch.randn(ATTN_C, generator=gen)
        c = c / c.norm()
        q, k = q + 2.0 * math.sqrt(ATTN_C) * c, k + 2.0 * math.sqrt(ATTN_C) * c
    elif case == "uniform":
        q[:, ::7, :] = 0.0
    else:
        where, g = case.rsplit("_g", 1)
        kj = k[:, planted_column(T, where), :]
        q = q + float(g) / ATTN_SCALE * kj / (kj * kj).sum(-1, keepdim=True)
    return q, k, v, do


def gemm_kernel_names(T: int, bf16: bool):
    """kernel instantiations of the materialised attention's three GEMM forms at T tokens, z = 2:
    nt [T,512] x [T,512]^T (contracts over the 512 channels: vectorised at every T), nn [T,T] x [T,512] and tn [T,T]^T x [T,512]
    (contract over T: 16-byte loads need T % 4 == 0; in bf16 mode every other T runs the unvectorised FP32 kernel)"""
    vec = T % 4 == 0
    tf = {True: "true", False: "false"}
    nt_tile = "128,32,4,1" if T <= 32 else "128,128,4,2"
    tn_tile = "32,128,1,4" if T <= 32 else "128,128,4,2"
    if bf16:
        return (f"igemm_rows_bf16_kernel<{nt_tile},false,0>",
                "igemm_rows_bf16_kernel<128,128,4,2,true,0>" if vec else "igemm_rows_kernel<128,128,4,2,true,false,0>",
                f"wgrad_bf16_kernel<{tn_tile},0>" if vec else f"wgrad_kernel<{tn_tile},false,0>")
    return (f"igemm_rows_kernel<{nt_tile},false,true,0>", f"igemm_rows_kernel<128,128,4,2,true,{tf[vec]},0>",
            f"wgrad_kernel<{tn_tile},{tf[vec]},0>")


@functools.lru_cache(maxsize=None)
def attn_case(case: str, T: int, rounded: bool):
    """(inputs, float64 reference) of a case, computed once per session; rounded: the reference takes the bf16-rounded
    operands.  The tensors are shared between tests: read, never written."""
    ins = attn_inputs(case, T)
    return ins, attention_ref(*((r16(t) for t in ins) if rounded else ins), ATTN_SCALE)
