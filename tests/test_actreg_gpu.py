"""ops.actreg_stats / ops.actreg_inject (csrc/actreg.hip) against the float64 references and the derived bounds of
tests/actreg_refs.py, the exact identities (a zero coefficient passes the gradient on bit for bit), non-finite operands,
repeatability, guarded memory and argument refusals; then Engine.add_activation_penalty on the small synthetic VAE against the
float64 oracle with the same penalties added to its loss through forward hooks, and what must not change (a step without a
penalty, a weight of zero, checkpointing, a frozen encoder, eval); then src/train.py on
configs/experiment_synthetic_activation_penalty.yaml.

Oracle bars (test_engine_against_the_float64_oracle): 2x the worst figure measured on MI355X per mode
(profiles/actreg_measured.json, "oracle"), the rule of tests/test_engine_gpu.py and tests/test_changrad_gpu.py: the penalty
value and every per-target value relative to the oracle's, every parameter gradient relative to the tensor's own maximum
(tensors whose maximum is below 1e-5 of the model's largest gradient entry relative to that entry: attention to_k.bias has a
mathematically zero gradient)."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import actreg_refs as R
import chanhist_refs as HR
from guarded import GuardedPool, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (3, 4, 8, 128, 256, 260, 512)  # scalar path, one quad lane, two, one tile, a partial second tile, two full tiles
SHAPES = [(1, 5, 7), (2, 16, 16), (3, 33, 31)]  # the tail loop alone, whole trips, chunks that do not divide
F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
SPECS = [("ceiling", 0.5, 1.0), ("floor", 0.3, 10.0)]
# measured on MI355X (profiles/actreg_measured.json "oracle"): worst relative error of the penalty values / of a parameter
# gradient (of its own maximum) / of a small tensor (of the model's maximum); the bars are 2x
ORACLE_MEASURED = {"no": (6.766e-06, 1.465e-05, 1.847e-10), "bf16": (9.773e-03, 5.250e-02, 1.462e-06)}
ORACLE_TOL = {k: tuple(2.0 * x for x in v) for k, v in ORACLE_MEASURED.items()}


def _nch(a):
    from vaehip import ops
    B, H, W, Cc = a.shape
    return ops.actreg_chunks(B, H * W, Cc)


def _stats(a, kind, thr, weight, channels=None, gs=1.0, **kw):
    from vaehip import ops
    mask = None if channels is None else torch.as_tensor(R.mask_of(a.shape[-1], channels), dtype=F32).to(a.device)
    got = ops.actreg_stats(a, kind, thr, weight, mask, gs)
    return got, R.check_stats(got, a, kind, thr, weight, _nch(a), channels, gs, **kw)


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_sweep_within_the_derived_bounds(cuda, Cc, B, H, W):
    """every storage of a, g and out, both kinds, a mask, grad_scale 0.5"""
    from vaehip import ops
    a0, g0 = R.draw((B, H, W, Cc), Cc * 131 + B * 7 + H)
    ws = wi = 0.0
    for kind, thr, weight in SPECS:
        channels = None if kind == "ceiling" else tuple(range(0, Cc, 2))
        for da in (F32, BF16):
            a = a0.to(cuda).to(da)
            (sums, pen, coef), worst = _stats(a, kind, thr, weight, channels, 0.5)
            ws = max(ws, worst)
            assert float(coef.abs().max()) > 0 and float(pen.sum()) > 0  # the draw puts channels on both sides of either threshold
            for dg in (F32, BF16):
                g = g0.to(cuda).to(dg)
                out = ops.actreg_inject(a, g, kind, thr, coef)
                wi = max(wi, R.check_inject(out, a, g, kind, thr, coef))
                assert not R.same_bits(out, g)
    print(f"C={Cc} {B}x{H}x{W}: worst error / bound: statistics {ws:.3f}, inject {wi:.3f}")


@pytest.mark.parametrize("da,dg", PAIRS)
@pytest.mark.parametrize("kind,thr,weight", SPECS)
def test_channel_prefix_views(cuda, kind, thr, weight, da, dg):
    """4 of 8 channels (vector path, ld > C) and 3 of 4 (scalar path) of wider buffers, read in place: the pad channels (1e6)
    must not leak, and the results are those of a contiguous copy bit for bit"""
    from vaehip import ops
    for wide, Cc in ((8, 4), (4, 3)):
        a8, g8 = R.draw((3, 7, 13, wide), 5)
        a8[..., Cc:] = 1e6
        g8[..., Cc:] = 1e6
        a8, g8 = a8.to(cuda).to(da), g8.to(cuda).to(dg)
        a, g = a8[..., :Cc], g8[..., :Cc]
        assert a.stride(2) == wide and R.vector_path(a, g) == (Cc == 4)
        got, _ = _stats(a, kind, thr, weight)
        ref, _ = _stats(a.contiguous(), kind, thr, weight)
        assert all(R.same_bits(x, y) for x, y in zip(got, ref))
        assert float(got[0][1].max()) < 1e4
        for aa, gg in ((a, g), (a, g.contiguous()), (a.contiguous(), g)):
            out = ops.actreg_inject(aa, gg, kind, thr, got[2])
            R.check_inject(out, a, g, kind, thr, got[2])
            assert R.same_bits(out, ops.actreg_inject(a.contiguous(), g.contiguous(), kind, thr, got[2]))
            assert float(out.float().abs().max()) < 10.0


@pytest.mark.parametrize("da,dg", PAIRS)
@pytest.mark.parametrize("kind,thr,weight", SPECS)
def test_offset_view_takes_the_scalar_path(cuda, kind, thr, weight, da, dg):
    """4 of 5 channels at a one-element offset: C % 4 == 0 but neither base address nor stride allows a vector access; the
    results are those of a contiguous copy (the vector path), the statistics within both paths' bounds"""
    from vaehip import ops
    a5, g5 = R.draw((2, 9, 11, 5), 6)
    a5[..., 0] = 1e6
    g5[..., 0] = 1e6
    a5, g5 = a5.to(cuda).to(da), g5.to(cuda).to(dg)
    a, g = a5[..., 1:], g5[..., 1:]
    assert not R.vector_path(a) and R.vector_path(a.contiguous())
    got, _ = _stats(a, kind, thr, weight)
    ref, _ = _stats(a.contiguous(), kind, thr, weight)
    assert R.same_bits(got[0][2], ref[0][2])  # the counts; the sums have another association order, each within its bound
    for x, y in zip(got, ref):
        assert torch.allclose(x.double(), y.double(), rtol=1e-5, atol=0)
    want = ops.actreg_inject(a.contiguous(), g.contiguous(), kind, thr, ref[2])
    for aa, gg in ((a, g), (a.contiguous(), g), (a, g.contiguous())):
        out = ops.actreg_inject(aa, gg, kind, thr, ref[2])
        assert R.same_bits(out, want)  # element-wise arithmetic: the same bits on either path
        R.check_inject(out, a, g, kind, thr, ref[2])
    # a coefficient vector that is not 16-byte aligned sends a vector-capable pair down the scalar path too
    c5 = torch.zeros(5, device=cuda)
    c5[1:] = ref[2]
    assert R.same_bits(ops.actreg_inject(a.contiguous(), g.contiguous(), kind, thr, c5[1:]), want)


@pytest.mark.parametrize("kind,thr,weight", SPECS)
@pytest.mark.parametrize("da", [F32, BF16])
@pytest.mark.parametrize("Cc,B,H,W,layout", HR.FRAME_CASES)
def test_at_the_edges_of_the_shared_frame(cuda, Cc, B, H, W, layout, da, kind, thr, weight):
    """the statistics of an output in every layout; the gradient it is injected into is a plain tensor of the other storage"""
    from vaehip import ops
    a, g = R.draw((B, H, W, Cc), Cc * 131 + B * 7 + H)
    a, g = HR.frame_layout(a.to(cuda).to(da), layout), g.to(cuda).to(BF16 if da == F32 else F32)
    (sums, pen, coef), _ = _stats(a, kind, thr, weight)
    R.check_inject(ops.actreg_inject(a, g, kind, thr, coef), a, g, kind, thr, coef)


@pytest.mark.parametrize("da,dg", PAIRS)
@pytest.mark.parametrize("Cc", [3, 8, 260])
def test_exact_identities(cuda, Cc, da, dg):
    from vaehip import ops
    a, g = R.draw((2, 9, 11, Cc), 21)
    g[0, 0, 0, 0] = -0.0  # a zero keeps its sign too
    g[1, 2, 3, 1] = 0.0
    a, g = a.to(cuda).to(da), g.to(cuda).to(dg)
    amax = float(a.float().abs().max())
    for kind, thr in (("ceiling", 0.5), ("floor", 0.3)):
        # weight 0: out is g and the penalty is exactly 0
        sums, pen, coef = ops.actreg_stats(a, kind, thr, 0.0)
        assert bool((pen == 0).all()) and bool((coef == 0).all()) and not bool(torch.signbit(coef).any())
        assert R.same_bits(ops.actreg_inject(a, g, kind, thr, coef), g)
    # a ceiling above max |a|: nothing over it, the penalty is exactly 0 and out is g although the coefficients are not 0
    sums, pen, coef = ops.actreg_stats(a, "ceiling", amax * 1.5, 1.0)
    assert bool((sums[0] == 0).all()) and bool((sums[2] == 0).all()) and bool((pen == 0).all()) and bool((coef > 0).all())
    assert R.same_bits(ops.actreg_inject(a, g, "ceiling", amax * 1.5, coef), g)
    sums, pen, coef = ops.actreg_stats(a, "ceiling", amax, 1.0)  # |a| <= t is not over t
    assert bool((sums[2] == 0).all()) and R.same_bits(ops.actreg_inject(a, g, "ceiling", amax, coef), g)
    # a floor under every channel's mean |a|: coef exactly 0, out is g
    m = a.float().abs().double().mean(dim=(0, 1, 2))
    sums, pen, coef = ops.actreg_stats(a, "floor", float(m.min()) * 0.5, 10.0)
    assert bool((coef == 0).all()) and bool((pen == 0).all()) and R.same_bits(ops.actreg_inject(a, g, "floor", 0.3, coef), g)
    # the mask zeroes exactly the unlisted channels' coef and pen, and leaves the others as they were
    listed = [0, Cc - 1]
    mask = torch.zeros(Cc, device=cuda)
    mask[listed] = 1.0
    for kind, thr in (("ceiling", 0.05), ("floor", 100.0)):
        full = ops.actreg_stats(a, kind, thr, 2.0)
        part = ops.actreg_stats(a, kind, thr, 2.0, mask)
        assert bool((full[2] != 0).all())
        assert R.same_bits(part[0], full[0])
        for c in range(Cc):
            if c in listed:
                assert R.same_bits(part[2][c], full[2][c]) and R.same_bits(part[1][c], full[1][c])
            else:
                assert part[2][c].item() == 0 and part[1][c].item() == 0
        out = ops.actreg_inject(a, g, kind, thr, part[2])
        rest = [c for c in range(Cc) if c not in listed]
        assert R.same_bits(out[..., rest].contiguous(), g[..., rest].contiguous())
        assert not R.same_bits(out[..., listed].contiguous(), g[..., listed].contiguous())


@pytest.mark.parametrize("da", [F32, BF16])
@pytest.mark.parametrize("Cc", [3, 4, 132])
def test_nan_and_inf_stay_where_they_are(cuda, Cc, da):
    from vaehip import ops
    a, g = R.draw((2, 9, 11, Cc), 11)
    a[1, 3, 4, 1] = float("-inf")
    a[0, 8, 10, 2] = float("nan")
    g[1, 0, 0, 0] = float("nan")
    g[0, 1, 1, 0] = float("inf")
    a, g = a.to(cuda).to(da), g.to(cuda).to(da)
    rest = [c for c in range(Cc) if c not in (1, 2)]
    for kind, thr, weight in SPECS:
        (sums, pen, coef), _ = _stats(a, kind, thr, weight, skip_channels=(1, 2))
        s = sums.cpu().numpy()
        assert np.isposinf(s[0, 1]) and np.isposinf(s[1, 1]) and np.isnan(s[0, 2]) and np.isnan(s[1, 2])
        ref = R.stats_ref(a, kind, thr, weight)["sums"][2]
        assert s[2, 1] == ref[1] and s[2, 2] == ref[2]  # both count as over the threshold, exactly once
        assert np.isfinite(s[:, rest]).all() and bool(torch.isfinite(pen[rest]).all()) and bool(torch.isfinite(coef[rest]).all())
        if kind == "ceiling":
            assert np.isposinf(pen[1].item()) and np.isnan(pen[2].item()) and bool(torch.isfinite(coef).all())
        else:
            assert pen[1].item() == 0 and coef[1].item() == 0 and np.isnan(pen[2].item()) and np.isnan(coef[2].item())
        # inject with finite coefficients: a non-finite a or g changes its own element and no other
        cf = torch.full((Cc,), 1e-3 if kind == "ceiling" else -1e-3, device=cuda)
        out = ops.actreg_inject(a, g, kind, thr, cf)
        bad = torch.zeros(a.shape, dtype=torch.bool)
        bad[1, 3, 4, 1] = bad[0, 8, 10, 2] = bad[1, 0, 0, 0] = bad[0, 1, 1, 0] = True
        R.check_inject(out, a, g, kind, thr, cf, skip=bad.numpy())
        o = out.float().cpu()
        assert torch.isnan(o[0, 8, 10, 2]) and torch.isnan(o[1, 0, 0, 0]) and torch.isposinf(o[0, 1, 1, 0])
        assert torch.isneginf(o[1, 3, 4, 1]) if kind == "ceiling" else torch.isfinite(o[1, 3, 4, 1])
        assert bool(torch.isfinite(o[~bad]).all())


def test_repeatable(cuda):
    from vaehip import ops
    torch.manual_seed(6)
    for da, dg in ((F32, F32), (BF16, BF16), (F32, BF16)):
        a = torch.randn((3, 40, 56, 256), device=cuda).to(da)
        g = (torch.randn((3, 40, 56, 256), device=cuda) * 0.01).to(dg)
        for kind, thr, weight in SPECS:
            thr = thr * 2.5  # (a unit normal: mean |a| = 0.8)
            x, y = ops.actreg_stats(a, kind, thr, weight), ops.actreg_stats(a, kind, thr, weight)
            assert all(R.same_bits(p, q) for p, q in zip(x, y))
            R.check_stats(x, a, kind, thr, weight, _nch(a))
            assert R.same_bits(ops.actreg_inject(a, g, kind, thr, x[2]), ops.actreg_inject(a, g, kind, thr, x[2]))


@pytest.mark.parametrize("kind,thr,weight", SPECS)
@pytest.mark.parametrize("case", ["c260_f32_f32", "c512_bf16_bf16", "c128_f32_bf16", "c8_bf16_f32", "c3_f32_f32", "c3_bf16_bf16",
                                  "view3of4_bf16_f32", "offset4of5_f32_f32", "c4_1pixel"])
def test_guarded_memory(cuda, case, kind, thr, weight):
    """operands, workspace and results in guarded, poisoned blocks, on the vector and the scalar path: no store outside a
    block, no unwritten result or workspace word, no operand changed, and the results are those of the plain run bit for bit"""
    from vaehip import ops
    pool = GuardedPool(cuda)
    dt = {"f32": F32, "bf16": BF16}
    if case.startswith("view3of4"):
        a4, g4 = R.draw((2, 12, 20, 4), 70)
        a4[..., 3] = g4[..., 3] = 1e6
        a = pool.put(a4.to(BF16), "a4")[..., :3]
        g = pool.put(g4[..., :3].contiguous(), "g")
    elif case.startswith("offset4of5"):
        a5, g5 = R.draw((2, 12, 20, 5), 71)
        a5[..., 0] = g5[..., 0] = 1e6
        a, g = pool.put(a5, "a5")[..., 1:], pool.put(g5, "g5")[..., 1:]
    elif case == "c4_1pixel":
        a, g = (pool.put(t, n) for t, n in zip(R.draw((2, 1, 1, 4), 72), "ag"))
    else:
        c, da, dg = case.split("_")
        a, g = R.draw((2, 12, 20, int(c[1:])), 74)
        a, g = pool.put(a.to(dt[da]), "a"), pool.put(g.to(dt[dg]), "g")
    plain = ops.actreg_stats(a, kind, thr, weight)
    plain_out = ops.actreg_inject(a, g, kind, thr, plain[2])
    torch.cuda.synchronize()
    pool.snapshot()
    with guarded(pool, ops):
        got = ops.actreg_stats(a, kind, thr, weight)
        out = ops.actreg_inject(a, g, kind, thr, got[2])
    torch.cuda.synchronize()
    assert len(pool.blocks) == 7  # the operands, the workspace, three statistics results and the injected gradient
    assert pool.violations() == [] and pool.changed() == []
    assert pool.unwritten_report() == []
    for t in (*got, out):
        pool.block_of(t)  # the results are pool tensors
    assert all(R.same_bits(x, y) for x, y in zip(got, plain)) and R.same_bits(out, plain_out)
    R.check_stats(got, a, kind, thr, weight, _nch(a))
    R.check_inject(out, a, g, kind, thr, got[2])


def test_argument_errors_are_refused_and_nothing_is_launched(cuda):
    from vaehip import ops
    from vaehip.lib import lib, VaeHipError
    B, H, W, Cc, nch = 2, 8, 8, 8, 2
    a, g = (t.to(cuda) for t in R.draw((B, H, W, Cc), 12))
    ws = torch.full((B * nch * Cc * 3 + 4,), -1, device=cuda, dtype=torch.int32)
    sums = torch.full((3, Cc), -1.0, device=cuda, dtype=torch.float64)
    pen = torch.full((Cc,), -1.0, device=cuda, dtype=torch.float64)
    coef = torch.full((Cc,), -1.0, device=cuda)
    out = torch.full((B, H, W, Cc), -1.0, device=cuda)
    p, st = ops._p, ops._stream

    def partial(ap=p(a), lda=Cc, B=B, HW=H * W, Cc=Cc, nch=nch, thr=0.5, wsp=p(ws)):
        lib.call("vae_actreg_partial", ap, 0, lda, B, HW, Cc, nch, thr, wsp, st())

    def final(wsp=p(ws), nch=nch, kind=0, thr=0.5, weight=1.0, gs=1.0, sp=p(sums), pp=p(pen), cp=p(coef)):
        lib.call("vae_actreg_final", wsp, B, H * W, Cc, nch, kind, thr, weight, None, gs, sp, pp, cp, st())

    def inject(ap=p(a), lda=Cc, gp=p(g), ldg=Cc, cp=p(coef), rows=B * H * W, Cc=Cc, kind=0, thr=0.5, op=p(out)):
        lib.call("vae_actreg_inject", ap, 0, lda, gp, 0, ldg, cp, rows, Cc, kind, thr, op, st())

    for fn, name, cases in [
            (partial, "actreg_partial", [(dict(ap=None), "null args"), (dict(wsp=None), "null args"), (dict(lda=Cc - 1), "pixel stride"),
                                         (dict(nch=H * W // 2 + 1), "empty chunk"), (dict(wsp=ws.data_ptr() + 4), "unaligned workspace"),
                                         (dict(B=32768, HW=65536), "2\\^31"), (dict(Cc=0), "bad args"), (dict(thr=0.0), "threshold"),
                                         (dict(thr=float("nan")), "threshold")]),
            (final, "actreg_final", [(dict(wsp=None), "null args"), (dict(sp=None), "null args"), (dict(pp=None), "null args"),
                                     (dict(cp=None), "null args"), (dict(wsp=ws.data_ptr() + 4), "unaligned workspace"),
                                     (dict(nch=H * W // 2 + 1), "empty chunk"), (dict(kind=2), "kind=2"), (dict(thr=-1.0), "threshold"),
                                     (dict(weight=-1.0), "weight"), (dict(weight=float("inf")), "weight"), (dict(gs=float("nan")), "grad_scale")]),
            (inject, "actreg_inject", [(dict(ap=None), "null args"), (dict(gp=None), "null args"), (dict(cp=None), "null args"),
                                       (dict(op=None), "null args"), (dict(rows=0), "bad args"), (dict(Cc=0), "bad args"),
                                       (dict(kind=-1), "kind=-1"), (dict(thr=float("inf")), "threshold"), (dict(lda=Cc - 1), "pixel stride"),
                                       (dict(ldg=Cc - 1), "pixel stride"), (dict(op=p(g)), "out of place"), (dict(op=p(a)), "out of place")])]:
        for kw, msg in cases:
            with pytest.raises(VaeHipError, match=name + ".*" + msg):
                fn(**kw)
    torch.cuda.synchronize()
    # nothing was launched by any of them
    assert bool((ws == -1).all()) and bool((sums == -1).all()) and bool((pen == -1).all()) and bool((coef == -1).all())
    assert bool((out == -1).all())
    with pytest.raises(ValueError, match="contiguous channels"):
        ops.actreg_stats(a.permute(0, 3, 1, 2), "ceiling", 0.5, 1.0)
    with pytest.raises(ValueError, match="contiguous channels"):
        ops.actreg_inject(a, g.permute(0, 2, 1, 3), "ceiling", 0.5, coef)
    with pytest.raises(ValueError, match="differ"):
        ops.actreg_inject(a, g[:, :4], "ceiling", 0.5, coef)
    with pytest.raises(ValueError, match="CUDA tensor"):
        ops.actreg_stats(a.double(), "ceiling", 0.5, 1.0)
    with pytest.raises(ValueError, match="CUDA tensor"):
        ops.actreg_inject(a, g.cpu(), "ceiling", 0.5, coef)
    with pytest.raises(ValueError, match="weight -1.0 is not a finite number >= 0"):
        ops.actreg_stats(a, "ceiling", 0.5, -1.0)
    with pytest.raises(ValueError, match="grad_scale"):
        ops.actreg_stats(a, "ceiling", 0.5, 1.0, None, float("nan"))
    with pytest.raises(ValueError, match=r"mask: expected a contiguous fp32 \[8\]"):
        ops.actreg_stats(a, "ceiling", 0.5, 1.0, torch.ones(7, device=cuda))
    with pytest.raises(ValueError, match=r"mask: expected a contiguous fp32 \[8\]"):
        ops.actreg_stats(a, "ceiling", 0.5, 1.0, torch.ones(8))
    with pytest.raises(ValueError, match=r"coef: expected a contiguous fp32 \[8\]"):
        ops.actreg_inject(a, g, "ceiling", 0.5, coef.double())
    with pytest.raises(ValueError, match=r"coef: expected a contiguous fp32 \[8\]"):
        ops.actreg_inject(a, g, "ceiling", 0.5, torch.ones(16, device=cuda)[::2])
    # and the same arguments, valid, run
    partial()
    final()
    R.check_stats((sums, pen, coef), a, "ceiling", 0.5, 1.0, nch)
    inject()
    R.check_inject(out, a, g, "ceiling", 0.5, coef)


# ---------------------------------------------------------------------------------------------------- engine
def _specs(targets):
    from vaehip.actreg import ActivationPenalty
    return [(n, ActivationPenalty(s["kind"], s["threshold"], s["weight"], s.get("channels"))) for n, s in targets]


def _setup(cuda, mode, targets, **trainer_kw):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.trainer import HipTrainer
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), R.SEED))
    w.to(cuda)
    tr = HipTrainer(w, lr=1e-4, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mode, kl_weight=R.KL,
                    activation_penalties=_specs(targets) if targets else None, **trainer_kw)
    return w, tr


def _batch(cuda, step=1):
    import vae_oracle as vo
    return vo.synthetic_pixels(R.B_, R.R_, 5, step).to(cuda), vo.synthetic_eps(R.B_, R.R_, 5, step).to(cuda)


def _bits(t):
    return t.detach().clone().view(torch.int32)


class _Spy:
    """counts the calls of ops.<name> and keeps (arguments, result)"""

    def __init__(self, *names):
        from vaehip import ops
        self.ops, self.names, self.calls = ops, names, {n: [] for n in names}

    def __enter__(self):
        self.real = {n: getattr(self.ops, n) for n in self.names}
        for n in self.names:
            def spy(*a, _n=n, **kw):
                out = self.real[_n](*a, **kw)
                self.calls[_n].append((a, out))
                return out
            setattr(self.ops, n, spy)
        return self

    def __exit__(self, *exc):
        for n in self.names:
            setattr(self.ops, n, self.real[n])


@pytest.fixture(scope="module")
def oracle():
    return R.oracle_pass(R.ENGINE_TARGETS)


def _against_oracle(w, res, oracle, scale, mode, tag):
    """-> (worst relative error of the penalty values, of a parameter gradient, of a small tensor), printing every figure"""
    got_terms = {n: float(v) for (n, _), (_, v) in zip(R.ENGINE_TARGETS, _by_name(w, res))}
    worst_v = abs(float(res["activation_penalty"]) - oracle["penalty"]) / oracle["penalty"]
    print(f"{tag} {mode}: penalty {float(res['activation_penalty']):.6e} (oracle {oracle['penalty']:.6e}): {worst_v:.3e}")
    for n, v in got_terms.items():
        rel = abs(v - oracle["terms"][n]) / oracle["terms"][n]
        print(f"{tag} {mode}: penalty of {n}: {rel:.3e}")
        worst_v = max(worst_v, rel)
    sc = res["scalars"].double().cpu()
    assert abs(float(sc[2]) - (float(sc[0]) + R.KL * float(sc[1]) + float(res["activation_penalty"]))) <= 1e-6 * float(sc[2])  # scalars[2] carries the penalty
    assert abs(float(sc[2]) - oracle["total"]) <= 0.05 * oracle["total"]
    gmax = max(float(g.abs().max()) for g in oracle["grads"].values()) * scale
    worst, worst_small, where = 0.0, 0.0, None
    for name, p in w.vae.named_parameters():
        ref = oracle["grads"][name] * scale
        err = float((p.grad.detach().double().cpu() - ref).abs().max())
        rmax = float(ref.abs().max())
        if rmax < 1e-5 * gmax:
            worst_small = max(worst_small, err / gmax)
            print(f"{tag} {mode}: grad {name}: {err / gmax:.3e} of the model's maximum (small tensor)")
        else:
            print(f"{tag} {mode}: grad {name}: {err / rmax:.3e} of the tensor's maximum")
            if err / rmax > worst:
                worst, where = err / rmax, name
    print(f"{tag} {mode}: WORST values {worst_v:.3e} gradients {worst:.3e} ({where}) small {worst_small:.3e}")
    return worst_v, worst, worst_small


def _by_name(w, res):
    """the step's (handle, value) terms in the order of R.ENGINE_TARGETS"""
    terms = {id(h.module): (h, v) for h, v in res["activation_penalty_terms"]}
    return [terms[id(w.get_submodule(n))] for n, _ in R.ENGINE_TARGETS]


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_against_the_float64_oracle(cuda, mode, scale, oracle):
    """scale 0.5: grad_scale = 0.5 against the oracle with the loss halved (its gradients times 0.5, exactly), at the same bar"""
    w, tr = _setup(cuda, mode, R.ENGINE_TARGETS)
    with _Spy("actreg_stats", "actreg_inject") as spy:
        res = w.vae.engine.forward_backward(*_batch(cuda), R.KL, grad_scale=scale)
    assert len(spy.calls["actreg_stats"]) == len(spy.calls["actreg_inject"]) == len(R.ENGINE_TARGETS)
    assert res["activation_penalty"].dtype == torch.float64 and res["activation_penalty"].dim() == 0
    assert len(res["activation_penalty_terms"]) == len(R.ENGINE_TARGETS)
    for (n, s), (h, v) in zip(R.ENGINE_TARGETS, _by_name(w, res)):
        assert h.last[1] is v and h.last[0].shape == (3, h.channels) and h.spec.kind == s["kind"]
    figs = _against_oracle(w, res, oracle, scale, mode, f"oracle scale={scale}")
    tol = ORACLE_TOL[mode]
    assert all(f <= t for f, t in zip(figs, tol)), (figs, tol)


NOT_UNFUSING = [t for t in R.ENGINE_TARGETS if not t[0].endswith(".conv2")]  # conv2's penalty un-fuses its residual add


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_registered_and_removed_is_bitwise_never_registered(cuda, mode):
    w, tr = _setup(cuda, mode, None)
    eng = w.vae.engine
    x, eps = _batch(cuda)
    with _Spy("actreg_stats", "actreg_inject") as spy:
        r0 = eng.forward_backward(x, eps, R.KL)
    assert spy.calls == {"actreg_stats": [], "actreg_inject": []}
    assert r0["activation_penalty"] is None and r0["activation_penalty_terms"] is None
    s0, g0 = _bits(r0["scalars"]), _bits(w.vae.arena.grad)
    hs = [eng.add_activation_penalty(w.get_submodule(n), s) for n, s in _specs(R.ENGINE_TARGETS)]
    r1 = eng.forward_backward(x, eps, R.KL)
    assert float(r1["activation_penalty"]) > 0 and not torch.equal(_bits(w.vae.arena.grad), g0)
    for h in hs:
        h.remove()
    assert not eng._penalties
    with _Spy("actreg_stats", "actreg_inject") as spy:
        r2 = eng.forward_backward(x, eps, R.KL)
    assert spy.calls == {"actreg_stats": [], "actreg_inject": []} and r2["activation_penalty"] is None
    assert torch.equal(_bits(r2["scalars"]), s0) and torch.equal(_bits(w.vae.arena.grad), g0)


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_weight_zero_gives_bitwise_equal_gradients(cuda, mode):
    w, tr = _setup(cuda, mode, None)
    eng = w.vae.engine
    x, eps = _batch(cuda)
    r0 = eng.forward_backward(x, eps, R.KL)
    s0, g0 = _bits(r0["scalars"]), _bits(w.vae.arena.grad)
    for n, s in NOT_UNFUSING:
        eng.add_activation_penalty(w.get_submodule(n), _specs([(n, dict(s, weight=0.0))])[0][1])
    with _Spy("actreg_inject") as spy:
        r1 = eng.forward_backward(x, eps, R.KL)
    assert len(spy.calls["actreg_inject"]) == len(NOT_UNFUSING)  # the gradient did pass through the kernel
    assert float(r1["activation_penalty"]) == 0.0
    assert torch.equal(_bits(r1["scalars"]), s0) and torch.equal(_bits(w.vae.arena.grad), g0)


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_weight_zero_on_a_fused_conv2_equals_the_unfused_step(cuda, mode):
    """a penalty on a resnet's conv2 un-fuses its residual add, which moves the step's bits whatever the weight (the add and the
    next GroupNorm's statistics are computed by other kernels): the weight-0 identity holds against the step with the same add
    un-fused by a gradient tracker on conv2, which only reads"""
    name = "vae.decoder.up_blocks.1.resnets.0.conv2"
    w, tr = _setup(cuda, mode, None)
    eng = w.vae.engine
    x, eps = _batch(cuda)
    h = eng.add_grad_tracker(w.get_submodule(name), lambda sums, absmax: None, ["mean_abs_gradient_per_channel"])
    with _Spy("add") as spy0:
        r0 = eng.forward_backward(x, eps, R.KL)
    s0, g0 = _bits(r0["scalars"]), _bits(w.vae.arena.grad)
    h.remove()
    eng.add_activation_penalty(w.get_submodule(name), _specs([(name, dict(R.CEILING, weight=0.0))])[0][1])
    with _Spy("add", "actreg_inject") as spy:
        r1 = eng.forward_backward(x, eps, R.KL)
    assert len(spy.calls["actreg_inject"]) == 1 and len(spy.calls["add"]) == len(spy0.calls["add"])
    assert float(r1["activation_penalty"]) == 0.0
    assert torch.equal(_bits(r1["scalars"]), s0) and torch.equal(_bits(w.vae.arena.grad), g0)


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_checkpointed_decoder_is_bitwise_the_same(cuda, mode):
    w, tr = _setup(cuda, mode, R.ENGINE_TARGETS)
    eng = w.vae.engine
    x, eps = _batch(cuda)
    r0 = eng.forward_backward(x, eps, R.KL)
    p0, t0, g0 = r0["activation_penalty"].clone(), [v.clone() for _, v in _by_name(w, r0)], _bits(w.vae.arena.grad)
    eng.checkpoint_decoder = True
    try:
        with _Spy("actreg_stats", "actreg_inject") as spy:
            r1 = eng.forward_backward(x, eps, R.KL)
    finally:
        eng.checkpoint_decoder = False
    # the replayed segments run their statistics pass again for the coefficients, and add nothing to the value
    assert len(spy.calls["actreg_inject"]) == len(R.ENGINE_TARGETS) < len(spy.calls["actreg_stats"])
    assert len(r1["activation_penalty_terms"]) == len(R.ENGINE_TARGETS)
    assert R.same_bits(r1["activation_penalty"], p0) and all(R.same_bits(v, t) for (_, v), t in zip(_by_name(w, r1), t0))
    assert torch.equal(_bits(r1["scalars"]), _bits(r0["scalars"])) and torch.equal(_bits(w.vae.arena.grad), g0)


def test_engine_frozen_encoder_reports_the_value_and_injects_nothing_there(cuda):
    enc = [t for t in R.ENGINE_TARGETS if t[0].startswith("vae.encoder") or t[0] == "vae.quant_conv"]
    assert len(enc) == 2
    w, tr = _setup(cuda, "no", R.ENGINE_TARGETS, trainable="decoder")
    w1, tr1 = _setup(cuda, "no", R.ENGINE_TARGETS)
    x, eps = _batch(cuda)
    with _Spy("actreg_stats", "actreg_inject") as spy:
        r = w.vae.engine.forward_backward(x, eps, R.KL)
    r1 = w1.vae.engine.forward_backward(x, eps, R.KL)
    assert len(spy.calls["actreg_stats"]) == len(R.ENGINE_TARGETS)
    assert len(spy.calls["actreg_inject"]) == len(R.ENGINE_TARGETS) - len(enc)  # nothing in the backward of the frozen prefix
    assert R.same_bits(r["activation_penalty"], r1["activation_penalty"])  # the value is reported all the same
    for (_, v), (_, v1) in zip(_by_name(w, r), _by_name(w1, r1)):
        assert R.same_bits(v, v1) and float(v) > 0
    for (name, p), (_, p1) in zip(w.vae.named_parameters(), w1.vae.named_parameters()):
        if p.requires_grad:  # the decoder's gradients do not depend on what is frozen upstream
            assert torch.equal(_bits(p.grad), _bits(p1.grad)), name


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_gradient_tracker_sees_the_total_gradient(cuda, mode):
    """a tracker on a penalised module (a composite one and a convolution) receives changrad(out, g') with g' the injected gradient"""
    names = ["vae.decoder.up_blocks.1.resnets.0", "vae.decoder.up_blocks.1.resnets.0.conv2", "vae.quant_conv"]
    w, tr = _setup(cuda, mode, [t for t in R.ENGINE_TARGETS if t[0] in names])
    eng = w.vae.engine
    got = {}
    for n in names:
        eng.add_grad_tracker(w.get_submodule(n), lambda sums, absmax, n=n: got.__setitem__(n, (sums, absmax)),
                             ["mean_abs_gradient_per_channel"])
    with _Spy("actreg_inject", "changrad") as spy:
        eng.forward_backward(*_batch(cuda), R.KL)
    assert len(spy.calls["actreg_inject"]) == len(spy.calls["changrad"]) == 3 and sorted(got) == sorted(names)
    injected = {id(out): args for args, out in spy.calls["actreg_inject"]}
    for (a, g), res in spy.calls["changrad"]:
        assert id(g) in injected, "the tracker was served a gradient that did not come out of actreg_inject"
        ia, ig = injected[id(g)][0], injected[id(g)][1]
        assert ia is a and not R.same_bits(g.float(), ig.float())  # the same kept output; the gradient did change


def test_eval_step_launches_nothing_new(cuda):
    w, tr = _setup(cuda, "no", R.ENGINE_TARGETS)
    w0, tr0 = _setup(cuda, "no", None)
    x, _ = _batch(cuda, 100)
    w.eval(), w0.eval()
    with _Spy("actreg_stats", "actreg_inject", "add") as spy:
        e = tr.eval_step(x)
    with _Spy("add") as spy0:
        e0 = tr0.eval_step(x)
    assert spy.calls["actreg_stats"] == [] and spy.calls["actreg_inject"] == []
    assert len(spy.calls["add"]) == len(spy0.calls["add"])  # no residual add is un-fused for a penalty that eval ignores
    for k in e0:
        if isinstance(e0[k], torch.Tensor):
            assert torch.equal(e[k], e0[k]), k
    with pytest.raises(NotImplementedError, match="an activation penalty is registered"):
        w.train()
        w(x, sample_posterior=False)
    with torch.no_grad():
        w(x, sample_posterior=False)  # not asked to record: served


# ---------------------------------------------------------------------------------------------------- CLI
def test_train_cli_with_the_activation_penalty_config(cuda, tmp_path):
    """src/train.py with configs/experiment_synthetic_activation_penalty.yaml: the log holds a finite positive
    train/activation_penalty, the CSV one row per target and logging step"""
    import yaml
    src = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
    c = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_activation_penalty.yaml")))
    c["output_dir"] = str(tmp_path)
    c["data"]["dataset_name"] = "synthetic:48"  # 6 steps/epoch x 2 epochs: logging steps 5 and 10
    c["data"]["resolution"] = 32
    cpath = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(c, open(cpath, "w"))
    env = dict(os.environ, PYTHONPATH=src)
    r = subprocess.run([sys.executable, os.path.join(src, "train.py"), "--config_path", cpath], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = tmp_path / c["run_name"]
    rows = list(csv.DictReader(open(out / "activation_penalty_history.csv")))
    names = [t["name"] for t in c["activation_penalty"]["targets"]]
    assert [(int(r_["step"]), r_["name"]) for r_ in rows] == [(s, n) for s in (5, 10) for n in names]
    assert list(rows[0]) == ["step", "name", "kind", "penalty", "elements_over_threshold", "channels_under_floor"]
    for r_ in rows:
        assert r_["kind"] == {names[0]: "ceiling", names[1]: "floor"}[r_["name"]]
        assert np.isfinite(float(r_["penalty"])) and float(r_["penalty"]) >= 0 and int(r_["elements_over_threshold"]) >= 0
        assert 0 <= int(r_["channels_under_floor"]) and (r_["name"] != names[1] or int(r_["channels_under_floor"]) <= 2)
    assert float(rows[0]["penalty"]) > 0 and int(rows[0]["elements_over_threshold"]) > 0
    logged = _logged(out)
    assert len(logged) == 2, logged
    for step, vals in logged:
        assert np.isfinite(vals["train/activation_penalty"]) and vals["train/activation_penalty"] > 0
        per = [vals[f"train/activation_penalty/{n}"] for n in names]
        assert abs(sum(per) - vals["train/activation_penalty"]) <= 1e-9 * vals["train/activation_penalty"]
        want = [float(r_["penalty"]) for r_ in rows if int(r_["step"]) == step]
        assert per == want


def _logged(out):
    """[(step, metrics)] of the logging steps that carry train/activation_penalty, from the metric logger's JSON lines"""
    import json
    found = []
    for line in open(out / "metrics.jsonl"):
        d = json.loads(line)
        if "train/activation_penalty" in d:
            found.append((int(d["step"]), d))
    return found
