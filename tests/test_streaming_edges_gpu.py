"""The step's non-convolution kernels (csrc/elementwise.hip, the batched GEMMs of csrc/igemm.hip in the attention position)
against the float64 references of tests/streaming_refs.py, at the sizes and values where such kernels go wrong: tails, a
single partial block, several blocks, grid-stride trips, clamp bounds, ties, overflow, -inf, one-hot rows.

Errors are measured on the scale that matters (an AdamW step against the UPDATE, a softmax row against its own maximum);
bars of the kind "k x fp32-CPU" come from torch's fp32 arithmetic on the CPU, never from the kernel.  Every figure is
recorded (streaming_refs.record; kept as profiles/streaming_edges_measured.json)."""
import pytest
import torch

import streaming_refs as sr
from test_attention_gpu import _ref as attention_ref64

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- AdamW / sqnorm
def _sqnorm(ops, gd):
    """vae_sqnorm with its workspace pre-filled with NaN: every workgroup, idle ones included, must write its partial"""
    ws = torch.full((2048,), float("nan"), device=gd.device)
    out = torch.full((1,), float("nan"), device=gd.device)
    ops.sqnorm(gd, out, ws)
    return out


def _check_sqnorm(key, sq, g):
    ref = sr.sqnorm_ref64(g)
    cpu = abs(float((g * g).sum()) - ref) / ref
    sr.check("sqnorm", key, abs(float(sq.item()) - ref) / ref, sr.bar(4, cpu, 1e-6), cpu)


def _adam_step(ops, key, p, g, m, v, max_norm, lr, step, band=False, ulp_floor=False):
    """one kernel step on device state (updated in place), checked from the kernel's own previous state.
    ulp_floor (the few-element cases): twice torch's error on one to five elements is twice a draw of rounding luck, so the bar
    is at least what the format allows a correct kernel: p * decay and the subtraction round a value of p's size once each,
    half an ulp apiece = 2^-23 max|p| in all (the update term's own error is 1e-3 of that), on the scale of the update."""
    prev, m0, v0 = p.detach().cpu().clone(), m.detach().cpu().clone(), v.detach().cpu().clone()
    gd = g.cuda()
    sq = None
    if max_norm > 0:
        sq = _sqnorm(ops, gd)
        _check_sqnorm(key, sq, g)
    ops.adamw(p, gd, m, v, sq, max_norm, lr, *sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"], step)
    args = (max_norm, lr, sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"], step)
    p64, m64, v64 = sr.adamw_ref64(prev, g, m0, v0, sr.sqnorm_ref64(g), *args)
    pt, mt, vt = sr.adamw_torch32(prev, g, m0, v0, *args)
    for name, sl in (("p_update", slice(None)),) + ((("p_update_band", sr.ADAM_BAND),) if band else ()):
        cpu = sr.update_error(pt, p64, prev, sl)
        floor = 2.0 ** -23 * float(prev.abs().max()) / float((p64 - prev.double()).abs().max()) if ulp_floor else 0.0
        # (lr = 0: the update is zero, torch leaves p alone and so must the kernel -- measured 0 against a bar of 0)
        sr.check("adamw", f"{key},{name}", sr.update_error(p, p64, prev, sl), max(2 * cpu, floor), cpu, strict=False)
    for name, got, ref, t32 in (("m", m, m64, mt), ("v", v, v64, vt)):
        cpu = sr.rel(t32, ref)
        sr.check("adamw", f"{key},{name}", sr.rel(got, ref), sr.bar(4, cpu, 1e-6), cpu)


@pytest.mark.parametrize("max_norm", [1.0, 0.0])
def test_adamw_update_and_the_band_where_eps_decides(cuda, max_norm):
    """five steps on weights of real size (0.05 N(0,1)), the error relative to the largest UPDATE of the step (whole tensor,
    and the band g = 0 / |g| ~ 1e-8 alone, where sqrt(v) is of the size of eps) against twice torch-fp32's own; max_norm = 0
    runs without a norm pointer"""
    from vaehip import ops
    n = sr.ADAM_N
    p = sr.adam_params(n).cuda()
    m, v = torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    for step, (lr, gs) in enumerate(sr.ADAM_STEPS, start=1):
        _adam_step(ops, f"n={n},max_norm={max_norm},step={step}", p, sr.adam_grad(n, gs, 100 + step), m, v, max_norm, lr, step, band=True)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1024, 1027, sr.ADAM_GRID_N])
def test_adamw_and_sqnorm_sizes(cuda, n):
    """no float4 at all, exactly one, one and a tail, whole float4s only, and more float4s than the capped grid has threads"""
    from vaehip import ops
    gen = torch.Generator().manual_seed(n)
    p = sr.adam_params(n, seed=n).cuda()
    m = (torch.randn(n, generator=gen) * 0.1).cuda()
    v = (torch.rand(n, generator=gen) * 1e-2).cuda()
    g = torch.randn(n, generator=gen) * 3.0
    _adam_step(ops, f"n={n},max_norm=1.0,step=2", p, g, m, v, 1.0, 1e-3, 2, ulp_floor=n < 1024)


def test_adamw_late_step_and_sqnorm_outlier(cuda):
    from vaehip import ops
    n = 1027
    gen = torch.Generator().manual_seed(7)
    p = sr.adam_params(n, seed=7).cuda()
    m = (torch.randn(n, generator=gen) * 0.1).cuda()
    v = (torch.rand(n, generator=gen) * 1e-2).cuda()
    _adam_step(ops, f"n={n},max_norm=1.0,step=100000", p, torch.randn(n, generator=gen) * 3.0, m, v, 1.0, 1e-3, 100000)
    g = torch.randn(sr.ADAM_N, generator=gen) * 1e-3
    g[54321] = 1e4
    _check_sqnorm("one_1e4_among_1e-3", _sqnorm(ops, g.cuda()), g)


# ---------------------------------------------------------------------------------------------------- GEMMs at attention sizes
def _gemm_operands(T):
    gen = torch.Generator().manual_seed(T)
    A = torch.randn(2, T, 512, generator=gen)      # q / do
    Bt = torch.randn(2, T, 512, generator=gen)     # k / v
    Pm = torch.randn(2, T, T, generator=gen)       # scores / their gradient
    return A, Bt, Pm


def _names(prof):
    return [rec[0] for rec in prof.records]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("T", sr.ATTN_MATERIALISED_T)
def test_gemms_in_the_attention_position(cuda, monkeypatch, T, mode):
    """[T,512] x [T,512]^T, [T,T] x [T,512] and [T,T]^T x [T,512] at T = (R/8)^2 tokens against float64, and the kernel each
    launch ran.  The reference has the operands the pinned kernel multiplies: in bf16 mode the bf16 kernels round them to bf16
    (exact products, fp32 sums: the fp32 bar holds), and the forms that contract over a T that is no multiple of 4 run the fp32
    kernel on the fp32 values -- against the rounded operands those launches are 2^-9 away, which is recorded, not asserted."""
    from vaehip import ops
    bf = mode == "bf16"
    A, Bt, Pm = _gemm_operands(T)
    prof = ops.LaunchProfiler()
    monkeypatch.setattr(ops, "PROFILER", prof)
    with ops.precision(ops.PREC_BF16 if bf else ops.PREC_F32):
        nt = ops.gemm_nt(A.cuda(), Bt.cuda(), 512 ** -0.5)
        nn = ops.gemm_nn(Pm.cuda(), Bt.cuda())
        tn = ops.gemm_tn(Pm.cuda(), Bt.cuda())
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "PROFILER", None)
    names = _names(prof)
    assert tuple(names) == sr.gemm_kernel_names(T, bf), names
    if bf:
        assert names[0].startswith("igemm_rows_bf16_kernel")
        assert names[1].startswith("igemm_rows_bf16_kernel" if T % 4 == 0 else "igemm_rows_kernel<128,128,4,2,true,false,")
        assert names[2].startswith("wgrad_bf16_kernel" if T % 4 == 0 else "wgrad_kernel<") and (T % 4 == 0 or ",false," in names[2])
    d = torch.float64
    for form, got, name, ref_of in (
            ("nt", nt, names[0], lambda f: 512 ** -0.5 * f(A).to(d) @ f(Bt).to(d).transpose(1, 2)),
            ("nn", nn, names[1], lambda f: f(Pm).to(d) @ f(Bt).to(d)),
            ("tn", tn, names[2], lambda f: f(Pm).to(d).transpose(1, 2) @ f(Bt).to(d))):
        rounds = "bf16" in name
        sr.check("gemm", f"T={T},{mode},{form},{name}", sr.rel(got, ref_of(sr.r16 if rounds else (lambda t: t))), 2e-5)
        if bf and not rounds:
            sr.record("gemm_fp32_kernel_in_bf16_mode_vs_rounded_operands", f"T={T},{form},{name}", sr.rel(got, ref_of(sr.r16)))


def _materialised(ops, q, k, v, do, scale):
    """the engine's sequence for short token counts (vaehip/engine.py:_attention, forward and its tape entry)"""
    P = ops.softmax_rows_(ops.gemm_nt(q, k, scale))
    o = ops.gemm_nn(P, v)
    dP = ops.gemm_nt(do, v)
    dv = ops.gemm_tn(P, do)
    dS = ops.softmax_bwd_rows_(P, dP)
    return o, ops.gemm_nn(dS, k, scale), ops.gemm_tn(dS, q, scale), dv


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("T", sr.ATTN_MATERIALISED_T)
def test_materialised_attention_at_ragged_token_counts(cuda, T, mode):
    """scores -> softmax -> context and the backward chain as the engine runs them below ATTN_BLOCKWISE_MIN_T, against the
    float64 attention of tests/test_attention_gpu.py: fp32 1e-4; bf16 mode on bf16-rounded operands with that file's bars"""
    from vaehip import ops
    bf = mode == "bf16"
    gen = torch.Generator().manual_seed(1000 + T)
    q, k, v, do = (torch.randn(2, T, 512, generator=gen) * s for s in (2.0, 2.0, 1.0, 1.0))
    scale = 512 ** -0.5
    with ops.precision(ops.PREC_BF16 if bf else ops.PREC_F32):
        got = _materialised(ops, q.cuda(), k.cuda(), v.cuda(), do.cuda(), scale)
    torch.cuda.synchronize()
    f = sr.r16 if bf else (lambda t: t)
    ro, _, rq, rk, rv = attention_ref64(f(q), f(k), f(v), f(do), scale)
    for name, g, r, tol in (("o", got[0], ro, 4e-3 if bf else 1e-4), ("dq", got[1], rq, 1e-2 if bf else 1e-4),
                            ("dk", got[2], rk, 1e-2 if bf else 1e-4), ("dv", got[3], rv, 1e-2 if bf else 1e-4)):
        sr.check("materialised_attention", f"T={T},{mode},{name}", sr.rel(g, r), tol)


# ---------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("cols", sr.SOFTMAX_COLS)
def test_softmax_rows_edges(cuda, cols):
    """fewer columns than one wave, than the workgroup, one more, several trips; rows offset by 1e4, of spread 90, one-hot,
    half -inf.  Forward per row on the scale of the row's own maximum; backward per row on the scale of dP (dS of a one-hot row
    is about 0), from the float64 P rounded to fp32."""
    from vaehip import ops
    S, dP = sr.softmax_inputs(cols)
    P64 = sr.softmax_ref(S)
    P = ops.softmax_rows_(S.clone().cuda()).cpu()
    assert not bool(P.isnan().any())
    assert bool((P[S == float("-inf")] == 0).all())
    cpu = sr.row_rel(sr.softmax_ref(S, torch.float32), P64, P64)
    err = sr.row_rel(P, P64, P64)
    sums = (P.double().sum(-1) - 1).abs()
    Pin = P64.float()
    dS64 = sr.softmax_bwd_ref(Pin, dP)
    dS = ops.softmax_bwd_rows_(Pin.cuda(), dP.clone().cuda()).cpu()
    cpub = sr.row_rel(sr.softmax_bwd_ref(Pin, dP, torch.float32), dS64, dP)
    errb = sr.row_rel(dS, dS64, dP)
    for r, row in enumerate(sr.SOFTMAX_ROWS):
        sr.check("softmax_fwd", f"cols={cols},{row}", float(err[r]), sr.bar(8, float(cpu[r]), 2e-6), float(cpu[r]))
        sr.check("softmax_rowsum", f"cols={cols},{row}", float(sums[r]), 1e-6)
        sr.check("softmax_bwd", f"cols={cols},{row}", float(errb[r]), sr.bar(8, float(cpub[r]), 2e-6), float(cpub[r]))


# ---------------------------------------------------------------------------------------------------- sample + KL, MSE, layout, pool
@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("shape", sr.SAMPLE_SHAPES)
def test_sample_kl_blocks_and_clamp_bounds(cuda, shape, planted):
    """one partial block, four whole ones, three and a part (kl_partial indexed per image with nblk > 1); log-variances at,
    beyond and just inside the clamp bounds.  A planted exp(20) owns the tensor maximum, so values and gradients are held to
    1e-6 twice: over the planted pixels and over all the others."""
    from vaehip import ops
    B, h, w, L = shape
    mom, eps, dz, mask = sr.sample_inputs(B, h, w, L, planted)
    klw = 1e-3
    md, ed, dd = mom.cuda(), eps.cuda(), dz.cuda()
    key = f"B={B},hwL={h * w * L},planted={planted}"
    regions = (("planted", mask), ("rest", ~mask)) if planted else (("all", ~mask),)
    for vname, e_cpu, e_dev in (("eps", eps, ed), ("eps=None", None, None)):
        z, klp = ops.sample_kl(md, e_dev)
        assert klp.shape == (B, (h * w * L + 255) // 256)
        z64, kl64 = sr.sample_kl_ref(mom, e_cpu)
        for rname, mk in regions:
            sr.check("sample_z", f"{key},{vname},{rname}", sr.rel(z.cpu()[mk[..., :L]], z64[mk[..., :L]]), 1e-6)
        kl32 = sr.sample_kl_ref(mom, e_cpu, torch.float32)[1]
        cpu = float(((kl32.double() - kl64).abs() / kl64.abs()).max())
        got = float(((klp.double().cpu().sum(1) - kl64).abs() / kl64.abs()).max())
        sr.check("sample_kl", f"{key},{vname}", got, sr.bar(4, cpu, 1e-6), cpu)
    for vname, e_cpu, e_dev, d_cpu, d_dev in (("eps,dz", eps, ed, dz, dd), ("eps,dz=None", eps, ed, None, None), ("eps=None,dz", None, None, dz, dd)):
        dm = ops.sample_kl_bwd(md, e_dev, d_dev, klw).cpu()
        dm64 = sr.sample_kl_bwd_ref(mom, e_cpu, d_cpu, klw)
        for rname, mk in regions:
            sr.check("sample_kl_bwd", f"{key},{vname},{rname}", sr.rel(dm[mk], dm64[mk]), 1e-6)
        lv = mom[..., L:]
        assert bool((dm[..., L:][(lv < -30.0) | (lv > 20.0)] == 0).all())
        if planted and (d_cpu is not None):
            assert bool((dm[..., L:][(lv == -30.0) | (lv == 20.0)] != 0).all())   # torch passes the gradient at the bounds


@pytest.mark.parametrize("n", sr.MSE_SIZES)
def test_mse_loss_scalars_and_scaled_gradient(cuda, n):
    from vaehip import ops
    recon, target, klp = sr.mse_inputs(n)
    klw = 1e-3
    ref = sr.loss_ref(recon, target, klp, klw)
    cpu32 = sr.loss_ref(recon, target, klp, klw, torch.float32)
    sc = ops.mse_kl_loss(recon.cuda(), target.cuda(), klp.cuda(), klw).cpu()
    for i, name in enumerate(("mse", "kl", "total")):
        cpu = abs(float(cpu32[i]) - float(ref[i])) / abs(float(ref[i]))
        sr.check("loss_scalars", f"n={n},{name}", abs(float(sc[i]) - float(ref[i])) / abs(float(ref[i])), sr.bar(4, cpu, 1e-6), cpu)
    for scale in (1.0, 0.25):   # 0.25: a micro-batch of four in gradient accumulation
        d = ops.mse_bwd(recon.cuda(), target.cuda(), scale)
        sr.check("mse_bwd", f"n={n},scale={scale}", sr.rel(d, 2.0 * scale / n * (recon.double() - target.double())), 1e-6)


@pytest.mark.parametrize("shape,cpad", [((3, 3, 17, 19), 4), ((2, 8, 5, 5), None), ((3, 4, 33, 9), None), ((2, 8, 5, 5), 12)])
def test_layout_conversion_is_exact(cuda, shape, cpad):
    """more pixels than one workgroup (3 x 17 x 19 = 969, 3 x 33 x 9 = 891) and fewer; bit-equal, pad lanes exactly 0"""
    from vaehip import ops
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[2]))
    x[0, 0, 0, 0], x[-1, -1, -1, -1] = -0.0, float("inf")
    y = ops.nchw_to_nhwc(x.cuda(), cpad).cpu()
    Cc = shape[1]
    assert y.shape == (shape[0], shape[2], shape[3], cpad or Cc)
    assert torch.equal(sr.bits_of_f32(y[..., :Cc]), sr.bits_of_f32(x.permute(0, 2, 3, 1)))
    if cpad:
        assert int(sr.bits_of_f32(y[..., Cc:]).abs().max()) == 0
    back = ops.nhwc_to_nchw(y[..., :Cc].contiguous().cuda()).cpu()
    assert torch.equal(sr.bits_of_f32(back), sr.bits_of_f32(x))


@pytest.mark.parametrize("B,H,W,Cc", [(2, 5, 7, 4), (1, 3, 9, 132)])
def test_sumpool2x2_odd_maps(cuda, B, H, W, Cc):
    from vaehip import ops
    from vaehip.lib import lib
    s = torch.randn(B, 2 * H, 2 * W, Cc, generator=torch.Generator().manual_seed(H * W))
    out = torch.full((B, H, W, Cc), float("nan"), device=cuda)
    lib.call("vae_sumpool2x2", ops._p(s.cuda()), B, H, W, Cc, ops._p(out), ops._stream())
    sr.check("sumpool2x2", f"{B}x{H}x{W}x{Cc}", sr.rel(out, s.double().view(B, H, 2, W, 2, Cc).sum(dim=(2, 4))), 1e-6)


# ---------------------------------------------------------------------------------------------------- bf16 rounding, bit for bit
@pytest.mark.parametrize("n", sr.BF16_LENGTHS)
def test_pack_bf16_is_torch_rounding_bit_for_bit(cuda, n):
    """the device's fp32 -> bf16 conversion against tensor.bfloat16() on the CPU -- the definition every bf16-mode conv test
    takes for the rounded operand: ties, neighbours of ties, overflow to inf, subnormals; every entry in the 8-wide body and
    in the tail"""
    from vaehip import ops
    runs = []
    for rot in sr.bf16_rotations(n):
        x = sr.bf16_table(n, rot)
        dst = torch.full((n,), -1, dtype=torch.int16, device=cuda).view(torch.bfloat16)
        runs.append((x, ops.pack_bf16(x.cuda(), dst)))
    bad = []
    for x, got in runs:
        want = x.bfloat16()
        if not sr.same_bf16(got, want):
            g, w = sr.bits_of_bf16(got).tolist(), sr.bits_of_bf16(want).tolist()
            bad += [(hex(b), hex(gi), hex(wi)) for b, gi, wi in zip(sr.bits_of_f32(x).tolist(), g, w) if gi != wi]
    sr.record("pack_bf16", f"n={n}", {"launches": len(runs), "mismatches (fp32 bits, device, torch)": sorted(set(bad))[:40]})
    assert not bad, sorted(set(bad))[:40]


@pytest.mark.parametrize("n", sr.BF16_LENGTHS)
def test_unpack_bf16_is_exact(cuda, n):
    """n % 4 = 1, 3, 0, 1, 2, 3: the 4-wide body and every tail"""
    from vaehip import ops
    his = list(sr.BF16_HI) + [0x7f80, 0xff80, 0x7fc0, 0x0000, 0x807f]
    x = sr.bf16_from_bits(his[(3 * i) % len(his)] for i in range(n))
    got = ops.to_f32(x.cuda()).cpu()
    want = x.float()
    nan = want.isnan()
    assert torch.equal(sr.bits_of_f32(got)[~nan], sr.bits_of_f32(want)[~nan]) and bool(got[nan].isnan().all())


def test_add_bf16_rounds_the_fp32_sum_once(cuda):
    from vaehip import ops
    a, b = sr.bf16_add_pairs()
    got = ops.add(a.cuda(), b.cuda())
    want = (a.float() + b.float()).bfloat16()
    assert got.dtype == torch.bfloat16
    g, w = sr.bits_of_bf16(got), sr.bits_of_bf16(want)
    nan = want.float().isnan()
    bad = [(hex(x), hex(y), hex(gi), hex(wi)) for x, y, gi, wi, s in
           zip(sr.bits_of_bf16(a).tolist(), sr.bits_of_bf16(b).tolist(), g.tolist(), w.tolist(), nan.tolist()) if gi != wi and not s]
    sr.record("add_bf16", f"n={a.numel()}", {"mismatches (a, b, device, torch)": bad[:40]})
    assert not bad, bad[:40]
    assert bool(got.cpu().float()[nan].isnan().all())
