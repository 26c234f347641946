"""ops.changrad (csrc/changrad.hip): per-channel mean |g|, max |g|, gain gradient sum a g and Taylor saliency of one backward pass
in one read of (output, gradient), against the float64 references and the derived bounds of tests/changrad_refs.py (max |g|
bit for bit); then the engine's gradient trackers (Engine.add_grad_tracker, capture point `output_grad`) on the small synthetic
VAE: every emitted pass against the reference of its own operands, the monitor's vectors against the float64 oracle on torch
hooks, and what must not change (the step itself, checkpointing, accumulation, a frozen encoder); then src/train.py on
configs/experiment_synthetic_channel_grad.yaml.

Oracle bars (test_engine_vectors_against_the_float64_oracle): 2x the worst error of any per-channel vector relative to that
vector's own maximum, measured on MI355X per mode (profiles/changrad_measured.json, "oracle"), as tests/test_engine_gpu.py sets
its parameter-gradient bars."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import changrad_refs as R
import chanhist_refs as HR
from guarded import GuardedPool, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ["mean_abs_gradient_per_channel", "abs_max_gradient_per_channel", "gain_gradient_per_channel", "taylor_saliency_per_channel"]
CHANNELS = (1, 3, 4, 8, 128, 256, 257, 512)
SHAPES = [(1, 1, 1), (1, 7, 13), (3, 7, 13), (3, 16, 16), (1, 32, 24)]
F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
# measured worst |vector - oracle vector| / max |oracle vector| over the targets and the four metrics, and the bar = 2x
ORACLE_MEASURED = {"no": 1.20e-5, "bf16": 4.11e-2}  # fp32: inside the parameter gradients' 2.5e-5 (profiles/r03_parity_measured.json)
ORACLE_TOL = {k: (None if v is None else 2.0 * v) for k, v in ORACLE_MEASURED.items()}


def _per(a):
    from vaehip import ops
    B, H, W, Cc = a.shape
    nch = ops.changrad_chunks(B, H * W, Cc)
    return (H * W + nch - 1) // nch


def _check(got, a, g, **kw):
    return R.check(got[0], got[1], a, g, _per(a), **kw)


# ---------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("da,dg", PAIRS)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_sweep_within_the_derived_bounds(cuda, Cc, da, dg, B, H, W):
    from vaehip import ops
    a, g = R.draw((B, H, W, Cc), Cc * 131 + B * 7 + H)
    a, g = a.to(cuda).to(da), g.to(cuda).to(dg)
    got = ops.changrad(a, g)
    assert got[0].shape == (3, Cc) and got[0].dtype == torch.float64 and got[1].shape == (Cc,) and got[1].dtype == F32
    worst = _check(got, a, g)
    print(f"C={Cc} a={str(da)[6:]} g={str(dg)[6:]} {B}x{H}x{W}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("da,dg", PAIRS)
@pytest.mark.parametrize("Cc,B,H,W,layout", HR.FRAME_CASES)
def test_at_the_edges_of_the_shared_frame(cuda, Cc, B, H, W, layout, da, dg):
    """the layout is that of the gradient; the output is a plain tensor (the operands' strides and alignments differ)"""
    from vaehip import ops
    a, g = R.draw((B, H, W, Cc), Cc * 131 + B * 7 + H)
    a, g = a.to(cuda).to(da), HR.frame_layout(g.to(cuda).to(dg), layout)
    _check(ops.changrad(a, g), a, g)


@pytest.mark.parametrize("da,dg", PAIRS)
@pytest.mark.parametrize("which", ["a", "g", "both"])
def test_channel_prefix_views(cuda, which, da, dg):
    """3 of 4 channels of a wider buffer on either operand, read in place: the pad channel (1e6) must not leak"""
    from vaehip import ops
    a4, g4 = R.draw((3, 7, 13, 4), 5)
    a4[..., 3] = 1e6
    g4[..., 3] = 1e6
    a4, g4 = a4.to(cuda).to(da), g4.to(cuda).to(dg)
    a = a4[..., :3] if which in ("a", "both") else a4[..., :3].contiguous()
    g = g4[..., :3] if which in ("g", "both") else g4[..., :3].contiguous()
    assert (a.stride(2), g.stride(2)) == {"a": (4, 3), "g": (3, 4), "both": (4, 4)}[which]  # different strides too
    got = ops.changrad(a, g)
    _check(got, a, g)
    assert float(got[1].max()) < 10.0 and float(got[0].abs().max()) < 1e4


@pytest.mark.parametrize("da,dg", PAIRS)
def test_offset_view_takes_the_scalar_path(cuda, da, dg):
    """4 of 5 channels at a one-element offset: C % 4 == 0 but neither base address nor stride allows a vector load"""
    from vaehip import ops
    a5, g5 = R.draw((2, 9, 11, 5), 6)
    a5[..., 0] = 1e6
    g5[..., 0] = 1e6
    a5, g5 = a5.to(cuda).to(da), g5.to(cuda).to(dg)
    a, g = a5[..., 1:], g5[..., 1:]
    got = ops.changrad(a, g)
    _check(got, a, g)
    assert float(got[1].max()) < 10.0
    # one operand a contiguous vector-capable tensor, the other the offset view
    _check(ops.changrad(a.contiguous(), g), a, g)
    _check(ops.changrad(a, g.contiguous()), a, g)


def test_per_image_sign_flips_tell_saliency_from_gain(cuda):
    """g of image 1 is minus g of image 0 on the same a: P[1] = -P[0], so the gain is (near) 0 while the saliency is |P[0]|"""
    from vaehip import ops
    a1, g1 = R.draw((1, 16, 16, 8), 9)
    a1 = a1.abs() + 0.5
    g1 = g1.abs() + 0.01  # one sign per image: no cancellation inside P[b]
    a = torch.cat([a1, a1]).to(cuda)
    g = torch.cat([g1, -g1]).to(cuda)
    got = ops.changrad(a, g)
    _check(got, a, g)
    gain, sal = got[0][1].cpu().numpy(), got[0][2].cpu().numpy()
    P0 = (a1.double() * g1.double()).sum(dim=(0, 1, 2)).numpy()
    assert (np.abs(gain) <= 1e-5 * P0).all() and (np.abs(sal - P0) <= 1e-5 * P0).all() and (sal > 0.1).all()


@pytest.mark.parametrize("da,dg", PAIRS)
def test_zero_gradient_channel_is_exactly_zero(cuda, da, dg):
    from vaehip import ops
    a, g = R.draw((2, 12, 20, 8), 10)
    g[..., 2] = 0.0
    g[..., 5] = -0.0
    a, g = a.to(cuda).to(da), g.to(cuda).to(dg)
    got = ops.changrad(a, g)
    _check(got, a, g)
    for c in (2, 5):
        assert got[0][:, c].tolist() == [0.0, 0.0, 0.0] and got[1][c].item() == 0.0
        assert not any(np.signbit(v) for v in got[0][:, c].tolist())


@pytest.mark.parametrize("dg", [F32, BF16])
@pytest.mark.parametrize("Cc", [4, 130])
def test_inf_and_nan_gradients_stay_in_their_channels(cuda, Cc, dg):
    from vaehip import ops
    a, g = R.draw((2, 9, 11, Cc), 11)
    g[1, 3, 4, 1] = float("-inf")
    g[0, 8, 10, 2] = float("nan")
    a, g = a.to(cuda), g.to(cuda).to(dg)
    got = ops.changrad(a, g)
    _check(got, a, g, skip_channels=(1, 2))
    amax = got[1].cpu().numpy()
    assert np.isposinf(amax[1]) and np.isnan(amax[2]) and np.isfinite(np.delete(amax, [1, 2])).all()
    assert amax.view(np.uint32)[2] == 0x7FC00000  # the canonical NaN, whatever the payload in memory


def test_repeatable(cuda):
    from vaehip import ops
    torch.manual_seed(6)
    for da, dg in ((F32, F32), (BF16, BF16), (F32, BF16)):
        a = torch.randn((3, 40, 56, 256), device=cuda).to(da)
        g = (torch.randn((3, 40, 56, 256), device=cuda) * 0.01).to(dg)
        x, y = ops.changrad(a, g), ops.changrad(a, g)
        assert torch.equal(x[0].view(torch.int64), y[0].view(torch.int64)) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))
        _check(x, a, g)


@pytest.mark.parametrize("case", ["c257_f32_f32", "c512_bf16_bf16", "c128_f32_bf16", "view3of4_bf16_f32", "offset4of5_f32_f32",
                                  "c4_1pixel", "c1_1x7x13"])
def test_guarded_memory(cuda, case):
    """operands, workspace and results in guarded, poisoned blocks: no store outside a block, no unwritten result or workspace
    word, no operand changed, and the values are still within bound (a load outside an operand would have met NaN)"""
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
    elif case == "c1_1x7x13":
        a, g = (pool.put(t, n) for t, n in zip(R.draw((1, 7, 13, 1), 73), "ag"))
    else:
        c, da, dg = case.split("_")
        a, g = R.draw((2, 12, 20, int(c[1:])), 74)
        a, g = pool.put(a.to(dt[da]), "a"), pool.put(g.to(dt[dg]), "g")
    pool.snapshot()
    with guarded(pool, ops):
        got = ops.changrad(a, g)
    torch.cuda.synchronize()
    assert len(pool.blocks) == 5  # the operands, the workspace and two results
    assert pool.violations() == [] and pool.changed() == []
    assert pool.unwritten_report() == []
    for t in got:
        pool.block_of(t)  # the results are pool tensors
    _check(got, a, g)


def test_argument_errors_are_refused_with_their_message(cuda):
    from vaehip import ops
    from vaehip.lib import lib, VaeHipError
    B, H, W, Cc, nch = 2, 8, 8, 8, 2
    a, g = (t.to(cuda) for t in R.draw((B, H, W, Cc), 12))
    ws = torch.full((B * nch * Cc * 3 + 4,), -1, device=cuda, dtype=torch.int32)
    sums = torch.full((3, Cc), -1.0, device=cuda, dtype=torch.float64)
    amax = torch.full((Cc,), -1.0, device=cuda)
    p = ops._p

    def partial(ap=p(a), gp=p(g), lda=Cc, ldg=Cc, B=B, HW=H * W, Cc=Cc, nch=nch, wsp=p(ws)):
        lib.call("vae_changrad_partial", ap, 0, lda, gp, 0, ldg, B, HW, Cc, nch, wsp, ops._stream())

    for kw, msg in [(dict(ap=None), "null args"), (dict(gp=None), "null args"), (dict(wsp=None), "null args"),
                    (dict(lda=Cc - 1), "pixel stride"), (dict(ldg=Cc - 1), "pixel stride"), (dict(nch=H * W // 2 + 1), "empty chunk"),
                    (dict(wsp=ws.data_ptr() + 4), "unaligned workspace"), (dict(B=32768, HW=65536), "2\\^31"), (dict(Cc=0), "bad args")]:
        with pytest.raises(VaeHipError, match="changrad_partial.*" + msg):
            partial(**kw)
    with pytest.raises(VaeHipError, match="changrad_final.*null args"):
        lib.call("vae_changrad_final", p(ws), B, H * W, Cc, nch, None, p(amax), ops._stream())
    with pytest.raises(VaeHipError, match="changrad_final.*null args"):
        lib.call("vae_changrad_final", p(ws), B, H * W, Cc, nch, p(sums), None, ops._stream())
    with pytest.raises(VaeHipError, match="changrad_final.*unaligned workspace"):
        lib.call("vae_changrad_final", ws.data_ptr() + 4, B, H * W, Cc, nch, p(sums), p(amax), ops._stream())
    with pytest.raises(VaeHipError, match="changrad_final.*empty chunk"):
        lib.call("vae_changrad_final", p(ws), B, H * W, Cc, H * W // 2 + 1, p(sums), p(amax), ops._stream())
    with pytest.raises(VaeHipError, match="changrad_final.*2\\^31"):
        lib.call("vae_changrad_final", p(ws), 32768, 65536, Cc, 1, p(sums), p(amax), ops._stream())
    torch.cuda.synchronize()
    # nothing was launched by any of them
    assert bool((ws == -1).all()) and bool((sums == -1).all()) and bool((amax == -1).all())
    with pytest.raises(ValueError, match="contiguous channels"):
        ops.changrad(a.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match="differ"):
        ops.changrad(a, g[:, :4])
    with pytest.raises(ValueError, match="CUDA tensors"):
        ops.changrad(a, g.double())
    # and the same arguments, valid, run
    partial()
    lib.call("vae_changrad_final", p(ws), B, H * W, Cc, nch, p(sums), p(amax), ops._stream())
    R.check(sums, amax, a, g, H * W // nch)


# ---------------------------------------------------------------------------------------------------- engine
RES = "vae.decoder.up_blocks.1.resnets.0"
CONFIG_TARGETS = [RES, RES + ".conv1", "vae.decoder.up_blocks.1.upsamplers.0", "vae.decoder", "vae.quant_conv"]  # the new config's
ENCODER_TARGETS = ["vae.encoder.down_blocks.0.resnets.0", "vae.encoder.mid_block.attentions.0", "vae.encoder", "vae.quant_conv"]
# ... and a mid block, a whole up block, an attention and a convolution whose residual add is un-fused by the tracker
ALL_TARGETS = CONFIG_TARGETS + ENCODER_TARGETS[:3] + ["vae.decoder.mid_block", "vae.decoder.up_blocks.0", RES + ".conv2"]
R_, B_, SEED = 32, 2, 7


def _cfg(names):
    return {"enabled": True, "track_interval": 1,
            "target_layers": [{"name": n, "capture_point": "output_grad", "metrics": list(FOUR)} for n in names]}


def _setup(cuda, mode, names, **trainer_kw):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from vaehip.trainer import HipTrainer
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), SEED))
    w.to(cuda)
    tr = HipTrainer(w, lr=1e-4, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mode, **trainer_kw)
    mon = ActivityMonitor(w, _cfg(names)) if names is not None else None
    return w, tr, mon


def _batch(cuda, step):
    import vae_oracle as vo
    return vo.synthetic_pixels(B_, R_, 5, step).to(cuda), vo.synthetic_eps(B_, R_, 5, step).to(cuda)


def _buffered(mon):
    """layer id -> the (sums, absmax) device pairs buffered since the last step(), one per backward pass"""
    return {lid: [e.t for e in d[FOUR[0]]] for lid, d in mon.hook_collected_buffer.items()}


def _same(x, y):
    return (torch.equal(x[0].view(torch.int64), y[0].view(torch.int64)) and
            torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)))


def _oracle_shapes(names):
    """NHWC output shape -> how many of the targets have it (a forward of the oracle with hooks)"""
    import vae_oracle as vo
    o = vo.OracleWrapper(seed=SEED)
    shapes, hooks = {}, []
    for n in names:
        def hook(m, i, out):
            k = (out.shape[0], out.shape[2], out.shape[3], out.shape[1])
            shapes[k] = shapes.get(k, 0) + 1
        hooks.append(o.get_submodule(n).register_forward_hook(hook))
    with torch.no_grad():
        o(vo.synthetic_pixels(B_, R_, 5, 1), sample_posterior=True, eps=vo.synthetic_eps(B_, R_, 5, 1))
    for h in hooks:
        h.remove()
    return shapes


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_one_pass_per_target_and_backward_within_bound(cuda, mode):
    from vaehip import ops
    w, tr, mon = _setup(cuda, mode, ALL_TARGETS)
    assert sorted(mon.device_layers) == sorted(n + ".output_grad" for n in ALL_TARGETS)
    assert [n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks] == []
    real, calls = ops.changrad, []

    def spy(a, g):
        out = real(a, g)
        calls.append((a.clone(), g.clone(), out))
        return out
    ops.changrad = spy
    try:
        for s in (1, 2):
            tr.train_step(*_batch(cuda, s))
            assert len(calls) == len(ALL_TARGETS) * s  # one pass per target and backward
        w.eval()
        tr.eval_step(_batch(cuda, 100)[0])
        w.train()
        assert len(calls) == len(ALL_TARGETS) * 2  # an eval forward computes no gradient: nothing is emitted
    finally:
        ops.changrad = real
    torch.cuda.synchronize()
    buf = _buffered(mon)
    assert sorted(buf) == sorted(mon.device_layers) and all(len(v) == 2 for v in buf.values())
    want, seen = _oracle_shapes(ALL_TARGETS), {}
    for a, g, out in calls:
        assert a.shape == g.shape and a.dtype in (F32, BF16) and g.dtype in (F32, BF16)
        if mode == "no":
            assert a.dtype == F32  # fp32 storage: only a gradient may be a bf16-only image (gn_bwd(want16))
        seen[tuple(a.shape)] = seen.get(tuple(a.shape), 0) + 1
        worst = _check(out, a, g)
        print(f"{mode}: {tuple(a.shape)} a={str(a.dtype)[6:]} g={str(g.dtype)[6:]} ld=({a.stride(2)}, {g.stride(2)}): "
              f"worst error / bound {worst:.3f}")
    assert seen == {k: 2 * v for k, v in want.items()}, (seen, want)
    log = mon.step(2)
    for n in ALL_TARGETS:
        base = f"tracking/{n}.output_grad/"
        for k in (FOUR[0] + "_overall_mean", FOUR[0] + "_overall_max", FOUR[1] + "_overall_max", FOUR[2] + "_overall_mean",
                  FOUR[3] + "_overall_mean", FOUR[3] + "_overall_max"):
            assert np.isfinite(log[base + k]), (n, k)
    assert len(log) == 6 * len(ALL_TARGETS) and not mon.hook_collected_buffer
    mon.remove_hooks()
    assert not any(d.get("output_grad") for d in w.vae.engine._gtrackers.values())


@pytest.fixture(scope="module")
def oracle_vectors():
    """the monitor on torch hooks on the float64 oracle: same synthetic weights, pixels and eps, one backward pass"""
    import torch.nn.functional as F
    import vae_oracle as vo
    from tracking.monitor import ActivityMonitor
    o = vo.OracleWrapper(seed=SEED).double()
    mon = ActivityMonitor(o, _cfg(ALL_TARGETS))
    assert mon.device_layers == [] and len(mon.hooks) == len(ALL_TARGETS)
    x, eps = vo.synthetic_pixels(B_, R_, 5, 1).double(), vo.synthetic_eps(B_, R_, 5, 1).double()
    out = o(x, sample_posterior=True, eps=eps)
    (F.mse_loss(out["reconstruction"], x) + 1e-6 * out["latent_dist"].kl().mean()).backward()
    mon.step(1)
    data = mon.get_data_for_step(1)
    mon.remove_hooks()
    return data


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_vectors_against_the_float64_oracle(cuda, mode, oracle_vectors):
    w, tr, mon = _setup(cuda, mode, ALL_TARGETS, kl_weight=1e-6)
    tr.train_step(*_batch(cuda, 1))
    mon.step(1)
    data = mon.get_data_for_step(1)
    mon.remove_hooks()
    assert sorted(data) == sorted(oracle_vectors)
    worst, where = 0.0, None
    for lid in sorted(data):
        for m in FOUR:
            got, ref = data[lid][m].astype(np.float64), oracle_vectors[lid][m].astype(np.float64)
            assert got.shape == ref.shape, (lid, m, got.shape, ref.shape)
            rel = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"{mode}: {lid} {m}: {rel:.3e} of the vector's maximum")  # the figures profiles/changrad_measured.json records
            if rel > worst:
                worst, where = rel, (lid, m)
    print(f"{mode}: worst {worst:.3e} at {where}")
    assert ORACLE_TOL[mode] is not None and worst <= ORACLE_TOL[mode], (where, worst, ORACLE_TOL[mode])


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_step_is_bitwise_the_same_with_and_without_gradient_trackers(cuda, mode):
    """none of the new config's five targets un-fuses a residual add: the trackers only read"""
    from tracking.monitor import ActivityMonitor
    w, tr, _ = _setup(cuda, mode, None)
    eng = w.vae.engine
    x, eps = _batch(cuda, 1)
    r0 = eng.forward_backward(x, eps, 1e-6)
    s0, g0 = r0["scalars"].clone(), w.vae.arena.grad.clone()
    mon = ActivityMonitor(w, _cfg(CONFIG_TARGETS))
    r1 = eng.forward_backward(x, eps, 1e-6)
    assert len(_buffered(mon)) == len(CONFIG_TARGETS)
    assert torch.equal(r1["scalars"].view(torch.int32), s0.view(torch.int32))
    assert torch.equal(w.vae.arena.grad.view(torch.int32), g0.view(torch.int32))
    mon.remove_hooks()


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_checkpointed_decoder_buffers_bitwise_the_same(cuda, mode):
    w, tr, mon = _setup(cuda, mode, ALL_TARGETS)
    eng = w.vae.engine
    x, eps = _batch(cuda, 1)
    eng.forward_backward(x, eps, 1e-6)
    plain = _buffered(mon)
    mon.hook_collected_buffer.clear()
    eng.checkpoint_decoder = True
    try:
        eng.forward_backward(x, eps, 1e-6)
    finally:
        eng.checkpoint_decoder = False
    ck = _buffered(mon)
    assert sorted(ck) == sorted(plain) and len(plain) == len(ALL_TARGETS)
    for lid in plain:
        assert len(ck[lid]) == len(plain[lid]) == 1 and _same(ck[lid][0], plain[lid][0]), lid
    mon.remove_hooks()


def test_engine_accumulation_buffers_one_entry_per_micro_batch(cuda):
    w, tr, mon = _setup(cuda, "no", CONFIG_TARGETS, gradient_accumulation_steps=2)
    w1, tr1, mon1 = _setup(cuda, "no", CONFIG_TARGETS)
    tr1.train_step(*_batch(cuda, 1))
    tr.train_step(*_batch(cuda, 1))
    assert not tr.sync_gradients and all(len(v) == 1 for v in _buffered(mon).values())
    tr.train_step(*_batch(cuda, 2))
    assert tr.sync_gradients
    buf, one = _buffered(mon), _buffered(mon1)
    assert sorted(buf) == sorted(n + ".output_grad" for n in CONFIG_TARGETS) and all(len(v) == 2 for v in buf.values())
    for lid in buf:  # g carries the 1 / gradient_accumulation_steps factor
        full, half = one[lid][0][1].double(), buf[lid][0][1].double()
        assert float((half - 0.5 * full).abs().max()) <= 1e-3 * float(full.max()), lid
    data = (mon.step(1), mon.get_data_for_step(1))[1]
    for lid, pairs in buf.items():  # step(): the unweighted mean of the sums over the passes, the maximum of the maxima
        stack = np.mean(np.stack([p[0].cpu().numpy().astype(np.float32) for p in pairs]), axis=0)  # as step() does
        assert np.array_equal(data[lid][FOUR[0]], stack[0]) and np.array_equal(data[lid][FOUR[2]], stack[1])
        assert np.array_equal(data[lid][FOUR[3]], stack[2])
        assert np.array_equal(data[lid][FOUR[1]], torch.stack([p[1] for p in pairs]).amax(dim=0).cpu().numpy())
    mon.remove_hooks()
    mon1.remove_hooks()


def test_engine_frozen_encoder_emits_nothing_for_encoder_targets(cuda):
    names = CONFIG_TARGETS + ENCODER_TARGETS[:3]
    w, tr, mon = _setup(cuda, "no", names, trainable="decoder")
    w1, tr1, mon1 = _setup(cuda, "no", names)
    tr.train_step(*_batch(cuda, 1))
    tr1.train_step(*_batch(cuda, 1))
    frozen, full = _buffered(mon), _buffered(mon1)
    assert sorted(full) == sorted(n + ".output_grad" for n in names)
    decoder = sorted(n + ".output_grad" for n in names if n.startswith("vae.decoder"))
    assert sorted(frozen) == decoder  # no entry (and no error) where the gradient is not computed
    for lid in decoder:
        assert _same(frozen[lid][0], full[lid][0]), lid
    data = (mon.step(1), mon.get_data_for_step(1))[1]
    assert sorted(data) == decoder
    mon.remove_hooks()
    mon1.remove_hooks()


# ---------------------------------------------------------------------------------------------------- CLI
def test_train_cli_with_the_channel_grad_config(cuda, tmp_path):
    """src/train.py with configs/experiment_synthetic_channel_grad.yaml: the CSV carries the new record kinds for every
    output_grad layer"""
    import yaml
    src = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
    c = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_channel_grad.yaml")))
    c["output_dir"] = str(tmp_path)
    c["data"]["dataset_name"] = "synthetic:48"  # 6 steps/epoch x 2 epochs: the tracker fires at step 10
    c["data"]["resolution"] = 32
    cpath = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(c, open(cpath, "w"))
    env = dict(os.environ, PYTHONPATH=src)
    r = subprocess.run([sys.executable, os.path.join(src, "train.py"), "--config_path", cpath], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = list(csv.DictReader(open(tmp_path / c["run_name"] / "tracked_activation_stats.csv")))
    val = {(row["layer_identifier"], row["metric_type"]): row["metric_value"] for row in rows}
    layers = [e["name"] + ".output_grad" for e in c["tracking"]["target_layers"] if e["capture_point"] == "output_grad"]
    assert len(layers) == 5
    for lid in layers:
        for kind in ("mean_abs_gradient", "abs_max_gradient", "gain_gradient", "taylor_saliency"):
            for k in ("_overall_mean", "_overall_min", "_overall_max"):
                assert (lid, kind + k) in val, (lid, kind + k)
        assert float(val[(lid, "mean_abs_gradient_overall_mean")]) > 0 and int(float(val[(lid, "mean_abs_gradient_zero_channels")])) == 0
        assert float(val[(lid, "abs_max_gradient_overall_max")]) >= float(val[(lid, "mean_abs_gradient_overall_max")])
        assert float(val[(lid, "taylor_saliency_overall_min")]) >= 0 and int(float(val[(lid, "taylor_saliency_argmax_channel")])) >= 0
        assert (lid[:-len("_grad")], "per_channel_overall_mean") in val  # the forward metric on the same layer
