"""tests/streaming_refs.py without a GPU: every float64 reference against torch on the CPU, every input builder for the
properties the GPU tests rely on, and the kernel the library selects for each attention GEMM at the ragged token counts."""
import ctypes as C
import math

import pytest
import torch

import streaming_refs as sr


# ---------------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("max_norm", [1.0, 0.0])
def test_adamw_reference_follows_torch_adamw(max_norm):
    """torch.optim.AdamW (+ clip_grad_norm_) in fp32 over the five steps of the GPU test, each step against adamw_ref64 from
    torch's own previous state.  fp32 rounds p (|p| < 0.25: 2^-24 * 0.25 = 1.5e-8) and the update (1e-3 * 2^-24) -- on the
    scale of an update of lr = 5e-4 .. 1e-3 that is 3e-5; 1e-4 leaves the reference no room for a wrong term: dropping eps,
    or 0.1 % of the update, is 1e-3 or more (below)."""
    n = sr.ADAM_N
    pr = torch.nn.Parameter(sr.adam_params(n))
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=sr.ADAM["betas"], eps=sr.ADAM["eps"], weight_decay=sr.ADAM["wd"])
    m, v = torch.zeros(n), torch.zeros(n)
    for step, (lr, gs) in enumerate(sr.ADAM_STEPS, start=1):
        g = sr.adam_grad(n, gs, 100 + step)
        assert float(g[:1000].abs().max()) == 0.0 and 0.0 < float(g[1000:3000].abs().max()) < 1e-7
        prev = pr.detach().clone()
        pr.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pr], max_norm)
        for grp in opt.param_groups:
            grp["lr"] = lr
        opt.step()
        args = (sr.sqnorm_ref64(g), max_norm, lr, sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"], step)
        p64, m64, v64 = sr.adamw_ref64(prev, g, m, v, *args)
        st = opt.state[pr]
        for sl in (slice(None), sr.ADAM_BAND):
            assert sr.update_error(pr, p64, prev, sl) < 1e-4, (step, sl)
        # (torch's clip coefficient comes from an fp32 norm: its error enters m once and v twice)
        assert sr.rel(st["exp_avg"], m64) < 5e-6 and sr.rel(st["exp_avg_sq"], v64) < 1e-5
        # the state-injected single step the GPU test derives its bars from is this optimizer, bit for bit
        p1, m1, v1 = sr.adamw_torch32(prev, g, m, v, max_norm, lr, sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"], step)
        assert torch.equal(p1, pr.detach()) and torch.equal(m1, st["exp_avg"]) and torch.equal(v1, st["exp_avg_sq"])
        if lr > 0:
            # the measure sees what "max error / max |p|" could not: no eps (in the band), 99.9 % of the update, no 1e-6 in the clip
            no_eps = sr.adamw_ref64(prev, g, m, v, args[0], max_norm, lr, sr.ADAM["betas"], 0.0, sr.ADAM["wd"], step)[0]
            assert sr.update_error(torch.nan_to_num(no_eps, nan=0.0), p64, prev, sr.ADAM_BAND) > 1e-2, step
            assert sr.update_error(prev.double() + 0.999 * (p64 - prev.double()), p64, prev) > 9e-4, step
        m, v = st["exp_avg"].clone(), st["exp_avg_sq"].clone()


def test_clip_coefficient():
    assert sr.clip_coef64(4.0, 0.0) == 1.0 and sr.clip_coef64(4.0, -1.0) == 1.0
    assert sr.clip_coef64(0.25, 1.0) == 1.0
    assert sr.clip_coef64(4.0, 1.0) == 1.0 / (2.0 + 1e-6)
    g = torch.full((5,), 2.0)
    pr = torch.nn.Parameter(torch.zeros(5, dtype=torch.float64))
    pr.grad = g.double()
    torch.nn.utils.clip_grad_norm_([pr], 1.0)
    assert abs(float(pr.grad[0]) - 2.0 * sr.clip_coef64(sr.sqnorm_ref64(g), 1.0)) < 1e-15


# ---------------------------------------------------------------------------------------------------- bf16
def test_bf16_table_is_integer_round_to_nearest_even():
    bits = sr.bf16_table_bits()
    assert len(bits) == len(sr.BF16_HI) * len(sr.BF16_LO) + 3 and len(bits) % 2 == 1
    x = sr.f32_from_bits(bits)
    assert torch.equal(sr.bits_of_f32(x), torch.tensor(bits))
    nan = x.isnan()
    assert int(nan.sum()) == 1
    got = sr.bits_of_bf16(x.bfloat16())
    assert torch.equal(got[~nan], sr.rne_bf16_bits(torch.tensor(bits))[~nan])
    assert bool(x.bfloat16().float()[nan].isnan().all())
    # what the table is for: ties both ways, overflow to inf by rounding, subnormals that survive
    r = dict(zip(bits, got.tolist()))
    assert r[0x3f808000] == 0x3f80 and r[0x3f818000] == 0x3f82 and r[0x3f807fff] == 0x3f80 and r[0x3f808001] == 0x3f81
    assert r[0x7f7f8000] == 0x7f80 and r[0xff7fffff] == 0xff80 and r[0x7f7f7fff] == 0x7f7f
    assert r[0x00018001] == 0x0002 and r[0x00008001] == 0x0001 and r[0x00008000] == 0x0000 and r[0x0040ffff] == 0x0041
    for n in sr.BF16_LENGTHS:   # every entry is seen at every length, and at 1031 by every lane of an 8-wide body
        seen = set()
        for rot in sr.bf16_rotations(n):
            seen.update(sr.bits_of_f32(sr.bf16_table(n, rot)).tolist())
        assert seen == set(bits), n
    lanes = {(b, i % 8) for i, b in enumerate(sr.bits_of_f32(sr.bf16_table(1031))[:1024].tolist())}
    assert len(lanes) == 8 * len(bits)
    assert sr.same_bf16(x.bfloat16(), x.bfloat16()) and not sr.same_bf16(sr.bf16_from_bits([0x3f80]), sr.bf16_from_bits([0x3f81]))


def test_bf16_add_pairs_hold_ties_and_inexact_sums():
    a, b = sr.bf16_add_pairs()
    assert a.numel() == b.numel() and a.numel() % 4 == 0
    s = a.float() + b.float()
    low = sr.bits_of_f32(s) & 0xffff
    fin = s.isfinite()
    assert int(((low == 0x8000) & fin).sum()) >= 8            # ties
    exact = (a.double() + b.double()) == s.double()
    assert int((~exact & fin).sum()) >= 100                      # sums fp32 rounds before bf16 does
    assert int((s.abs() < 2.0 ** -126)[fin].sum()) >= 4 and int(s.bfloat16().isinf().sum()) >= 4 and int(s.isnan().sum()) >= 1
    # the definition: one rounding of the fp32 sum, round to nearest even
    want = sr.bits_of_bf16(s.bfloat16())
    ok = ~s.isnan()
    assert torch.equal(want[ok], sr.rne_bf16_bits(sr.bits_of_f32(s))[ok])


# ---------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("cols", sr.SOFTMAX_COLS)
def test_softmax_inputs_and_reference(cols):
    S, dP = sr.softmax_inputs(cols)
    assert S.shape == (5, cols) and len(sr.SOFTMAX_ROWS) == 5
    assert float(S[1].min()) > 9.9e3 and float(S[2].std()) > 30 if cols > 1 else True
    P = sr.softmax_ref(S)
    assert not bool(P.isnan().any()) and float((P.sum(-1) - 1).abs().max()) < 1e-14
    assert float(P[3, cols // 2]) == 1.0 and float(P[3].sum()) == 1.0
    if cols > 1:
        assert bool(S[4, ::2].isinf().all()) and float(P[4, ::2].abs().max()) == 0.0 and bool(S[4, 1::2].isfinite().all())
    Sd = S.double().clone().requires_grad_(True)
    torch.softmax(Sd, -1).backward(dP.double())
    assert sr.rel(sr.softmax_bwd_ref(P, dP), torch.nan_to_num(Sd.grad, nan=0.0)) < 1e-13


# ---------------------------------------------------------------------------------------------------- sample + KL, MSE
@pytest.mark.parametrize("shape", sr.SAMPLE_SHAPES)
def test_sample_kl_reference_against_autograd(shape):
    B, h, w, L = shape
    mom, eps, dz, mask = sr.sample_inputs(B, h, w, L, True)
    lv = mom[..., L:]
    for val in sr.LV_PLANTS:
        assert int((lv == val).sum()) == 2
    assert int(mask.sum()) == 2 * len(sr.LV_PLANTS) * 2 * L
    assert not bool(sr.sample_inputs(B, h, w, L, False)[3].any())
    klw = 1e-3
    for e, d in ((eps, dz), (None, dz), (eps, None)):
        md = mom.double().clone().requires_grad_(True)
        mu, lvc = md[..., :L], md[..., L:].clamp(-30, 20)
        z = mu + torch.exp(0.5 * lvc) * (e.double() if e is not None else 0.0)
        kl = 0.5 * torch.sum(mu ** 2 + lvc.exp() - 1 - lvc, dim=[1, 2, 3])
        total = klw * kl.mean() + ((z * d.double()).sum() if d is not None else 0.0)
        total.backward()
        z64, kl64 = sr.sample_kl_ref(mom, e)
        assert sr.rel(z64, z) < 1e-15 and sr.rel(kl64, kl) < 1e-15
        dm = sr.sample_kl_bwd_ref(mom, e, d, klw)
        assert sr.rel(dm, md.grad) < 1e-14
        # torch passes the gradient AT the bounds and stops it beyond them
        glv = dm[..., L:]
        assert bool((glv[(lv == -30.0) | (lv == 20.0)] != 0).all()) and bool((glv[(lv == -30.5) | (lv == 20.5)] == 0).all())


def test_loss_reference():
    recon, target, klp = sr.mse_inputs(4097)
    ref = sr.loss_ref(recon, target, klp, 1e-3)
    mse = torch.nn.functional.mse_loss(recon.double(), target.double())
    assert abs(float(ref[0] - mse)) < 1e-15 and abs(float(ref[1] - klp.double().sum(1).mean())) < 1e-12
    assert abs(float(ref[2] - (mse + 1e-3 * klp.double().sum(1).mean()))) < 1e-12


# ---------------------------------------------------------------------------------------------------- attention builders
@pytest.mark.parametrize("T", sr.ATTN_T)
def test_attention_builders_have_their_stated_properties(T):
    """planted maximum: where it is, how much of the row it holds, the log-sum-exp it gives; common shift: log-sum-exp past
    fp32 exp overflow (88.7) and an fp32 CPU evaluation still well inside the 1e-4 the kernels are held to; zero queries:
    log T exactly.  The fp32 CPU figures are the margin the GPU bars assume: they are asserted here at a third of the bars."""
    base = sr.attn_case("plain", T, False)[1]
    for case in sr.ATTN_CASES:
        (q, k, v, do), r64 = sr.attn_case(case, T, False)
        o, lse, dq, dk, dv, P = r64
        r32 = sr.attention_ref(q, k, v, do, sr.ATTN_SCALE, torch.float32)
        assert sr.rel(r32[0], o) < 3.3e-5 and sr.rel(r32[1], lse) < 3.3e-6 and sr.rel(r32[4], dv) < 3.3e-5, case
        one_hot = case.endswith("_g40")
        for i, ref in ((2, dq), (3, dk)):   # one-hot rows: dq, dk are about 0, measured on the scale of the plain case
            den = float(base[i].abs().max()) if one_hot else float(ref.abs().max())
            assert sr.rel_to(r32[i], ref, den) < 3.3e-5, (case, i)
        if "_g" in case:
            where, g = case.rsplit("_g", 1)
            j = sr.planted_column(T, where)
            hit = float((P.argmax(-1) == j).float().mean())   # g = 12 against scores of spread 4: many rows, not all
            assert hit == 1.0 if g == "40" else hit > 0.4, (case, hit)
            if where == "first":
                assert int(j.max()) < 32
            if where == "last":
                assert int(j.min()) >= T - 32
            med = float(P.amax(-1).median())
            if g == "12":
                assert 0.5 < med < 0.95, (case, med)   # (0.6 .. 0.8 at T = 192 and 576, 0.9 among 64 keys)
            else:
                assert med > 0.999999 and 20.0 < float(lse.min()) and float(lse.max()) < 60.0 and 38.0 < float(lse.median()) < 42.0, (case, med)
                assert float(dq.abs().max()) < 1e-3 * float(base[2].abs().max())
        if case == "shift":
            assert 80.0 < float(lse.min()) and float(lse.max()) < 125.0 and float(lse.median()) > 95.0, (float(lse.min()), float(lse.max()))
        if case == "uniform":
            assert float((lse[:, ::7] - math.log(T)).abs().max()) < 1e-13
            assert float((o[:, ::7] - v.double().mean(1, keepdim=True)).abs().max()) < 1e-14
            assert float((lse[:, 1::7] - math.log(T)).abs().min()) > 1e-3


def test_attention_case_cache_shares_one_reference():
    a, b = sr.attn_case("plain", 64, True), sr.attn_case("plain", 64, True)
    assert a is b
    (q, _, _, _), _ = a
    assert not torch.equal(sr.r16(q), q)
    assert sr.rel(sr.attn_case("plain", 64, True)[1][0], sr.attn_case("plain", 64, False)[1][0]) > 1e-4   # rounding is visible


# ---------------------------------------------------------------------------------------------------- kernel selection
@pytest.mark.parametrize("T", sr.ATTN_MATERIALISED_T)
def test_library_selects_the_pinned_attention_gemm_kernels(T):
    """what csrc/dispatch.cpp answers for the three GEMM forms of the materialised attention at T tokens (no launch): in bf16
    mode the forms that contract over T (nn, tn) need T % 4 == 0 for the bf16 kernel and otherwise run the unvectorised fp32
    kernel; the form that contracts over the 512 channels (nt) is vectorised at every T."""
    from vaehip import ops
    ptr = C.c_void_p(256)
    for prec, bf in ((ops.PREC_F32, False), (ops.PREC_BF16, True)):
        nt = ops.gemm_rows_args(T, T, 512, False, 1.0, 2, prec=prec)
        nn = ops.gemm_rows_args(T, 512, T, True, 1.0, 2, prec=prec)
        tn = ops.gemm_tn_args(T, 512, T, 1.0, 2, prec=prec)
        nt.A = nt.W = nt.C = nn.A = nn.W = nn.C = ptr
        tn.dY = tn.X = tn.out = ptr
        names = (ops._kernel_name("vae_igemm_kernel_name", nt), ops._kernel_name("vae_igemm_kernel_name", nn),
                 ops._kernel_name("vae_wgrad_kernel_name", tn))
        assert names == sr.gemm_kernel_names(T, bf), (T, bf, names)
