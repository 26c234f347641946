"""ops.changroup (csrc/changroup.hip): float64 sums of y, y^2 and |y| per (sample, channel) in one read, and the five
ActivityMonitor metrics derived from them (ops.changroup_metrics).

The sums are held to the float64 references of tests/changroup_refs.py within the radius derived there from the kernel's
addition chains (and, behind a GroupNorm transform, from the fp32 evaluation of y); the metrics to the interval those radii
leave them, which must also hold the two-pass float64 value computed straight from the tensor.  At every shape of the sweep and
in the mean = 10^3 sigma case the derived bound of the variance share must stay below 1 % of the uniform share
(changroup_refs.assert_share_bound_small): the condition on the accumulation scheme.

Then the engine on the small synthetic VAE (device path against the torch formulas on the same layer's full_activation_map, a
planted outlier filter, nothing launched and the step bitwise unchanged when no target names the metrics) and src/train.py on
the new config."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import changroup_refs as R
from changroup_refs import ACTIVE, DOM, FIVE, NRMS, SHARE, VARIATION
from guarded import GuardedPool, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
SHAPES = [(1, 1), (5, 7), (16, 16), (33, 31)]
EPS, TAU = 1e-6, 0.5


def _groups(Cc):
    """the GroupNorm(32) of the model where the channels allow it, 4 groups for 8 channels, none for 3 and 4 wide tensors"""
    return 32 if Cc % 32 == 0 else (4 if Cc % 4 == 0 and Cc > 4 else (33 if Cc == 132 else None))


def _stats(B, ld, dev, seed):
    from vaehip.ops import Stats
    sc, sh = R.stats_rows(B, ld, seed)
    return Stats(None, None, sc.to(dev), sh.to(dev))


def _check(got, x, st=None, xf=0, groups="auto", vec=None, tau=TAU):
    """device sums against the reference within the radius; the metrics of the device sums inside the interval, which holds
    the two-pass value; the share bound condition.  -> worst |error| / radius of the sums"""
    from vaehip import ops
    B, H, W, Cc = x.shape
    sums, rad, acc = R.ref_sums(x, st.scale if st is not None else None, st.shift if st is not None else None, xf, vec, parts=True)
    worst = R.assert_sums_close(got.cpu().numpy(), sums, rad)
    G = _groups(Cc) if groups == "auto" else groups
    if np.isfinite(sums).all():
        bounds = R.metric_bounds(sums, rad, H * W, G, EPS, tau)
        mine = R.metrics_from_ops(ops.changroup_metrics(got, H * W, G, EPS, tau), G)
        y = R.values(x, st.scale if st is not None else None, st.shift if st is not None else None, xf)[0]
        R.assert_within(mine, bounds, R.ref_metrics(y, G, EPS, tau))
        if G is not None:
            width = R.assert_share_bound_small(R.metric_bounds(sums, acc, H * W, G, EPS, tau), Cc, G)  # the scheme's own bound
            print(f"C={Cc} {str(x.dtype)[6:]} xf={xf} {B}x{H}x{W}: sums {worst:.2f} of the radius, share bound {width:.2e} (1 / cg = {G / Cc:.3f})")
    return worst


# ---------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("xf", [0, 1, 2])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc", [3, 4, 8, 32, 64, 132, 512])
def test_sums_and_metrics_against_the_float64_references(cuda, Cc, dt, xf, B, H, W):
    """C = 3 is the prefix view x4[..., :3] of a 4-channel buffer whose pad channel holds 1e6"""
    from vaehip import ops
    seed = Cc * 131 + xf * 7 + B * 3 + H
    if Cc == 3:
        x4 = R.draw((B, H, W, 4), seed).to(dt)
        x4[..., 3] = 1e6
        x = x4.to(cuda)[..., :3]
    else:
        x = R.draw((B, H, W, Cc), seed).to(dt).to(cuda)
    st = _stats(B, x.stride(2), cuda, Cc + xf) if xf else None
    got = ops.changroup(x, st, xf)
    assert got.shape == (B, Cc, 3) and got.dtype == torch.float64 and got.is_cuda
    _check(got, x, st, xf)


@pytest.mark.parametrize("Cc,B,H,W,layout,dt,xf", R.HR.frame_params((0, 1, 2)))
def test_at_the_edges_of_the_shared_frame(cuda, Cc, B, H, W, layout, dt, xf):
    from vaehip import ops
    x = R.HR.frame_layout(R.draw((B, H, W, Cc), Cc * 131 + xf * 7 + B * 3 + H).to(dt).to(cuda), layout)
    st = _stats(B, x.stride(2), cuda, Cc + xf) if xf else None
    _check(ops.changroup(x, st, xf), x, st, xf, vec=False if layout == "offset" else None)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,W,Cc,G", [(3, 33, 31, 32, 8), (2, 16, 16, 64, 32), (1, 40, 40, 8, 2), (2, 33, 31, 132, 33)])
def test_a_mean_a_thousand_sigma_keeps_its_variance(cuda, B, H, W, Cc, G, dt):
    """every channel at mean 10^3 (channel 1 at -10^3) with sigma 1 (bf16 storage: the stored values, spaced 4 and 8 apart around
    10^3, are what is summed): sum y^2 is 10^6 n, the variance a millionth of it"""
    from vaehip import ops
    g = torch.Generator(device="cpu").manual_seed(Cc + B)
    x = torch.randn((B, H, W, Cc), generator=g) + 1000.0
    x[..., 1] -= 2000.0
    x = x.to(dt).to(cuda)
    got = ops.changroup(x)
    _check(got, x, groups=G)
    # and the variance itself, per (b, c), against the two-pass value: S2 - S1^2 / n within what the radii of S1 and S2 allow
    # (plus the roundings of this line): some 1e-8 of it, where fp32 sums would have lost it whole
    y = R.values(x)[0]
    n = H * W
    var = ((y - y.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    s = got.cpu().numpy()
    sums, rad = R.ref_sums(x)
    mine = s[:, :, 1] - s[:, :, 0] ** 2 / n
    tol = rad[:, :, 1] + (2.0 * np.abs(sums[:, :, 0]) * rad[:, :, 0] + rad[:, :, 0] ** 2) / n + 4.0 * R.U64 * sums[:, :, 1]
    assert (np.abs(mine - var) <= tol).all() and (tol <= 1e-6 * var).all(), (np.abs(mine - var).max(), tol.max(), var.min())


@pytest.mark.parametrize("dt", DTYPES)
def test_constant_channels_and_a_group_constant_in_one_sample(cuda, dt):
    """C = 32 in 32 groups: a channel is its own group, a constant one has v exactly 0: its share is 0, not NaN.  C = 8 in 2 groups:
    group 1 is constant (one value) in sample 0 only: its four shares there are 0, not NaN, and 1 / 4 each is not invented"""
    from vaehip import ops
    x = R.draw((2, 9, 11, 32), 1).to(dt)
    x[:, :, :, 3] = 0.75
    x[0, :, :, 7] = -3.5
    x[..., 9] = 0.0
    x = x.to(cuda)
    chan, grp, S = ops.changroup_metrics(ops.changroup(x), 99, 32, EPS, TAU)
    chan, grp = chan.cpu().numpy(), grp.cpu().numpy()
    assert np.isfinite(chan).all() and np.isfinite(grp).all()
    assert chan[0, 3] == 0.0 and chan[1, 3] == 0.0 and grp[3] == 0.0 and chan[0, 9] == 0.0
    assert chan[0, 7] == 1.0 and grp[7] == 1.0  # constant in sample 0 (share 0), alive in sample 1 (share 1)
    assert (np.delete(chan[0], [3, 7, 9]) == 2.0).all()  # cg = 1: every live channel owns its group in both samples
    x = R.draw((2, 9, 11, 8), 2).to(dt)
    x[0, :, :, 4:] = 0.25
    x = x.to(cuda)
    got = ops.changroup(x)
    _check(got, x, groups=2)
    chan, grp, S = ops.changroup_metrics(got, 99, 2, EPS, TAU)
    chan, grp = chan.cpu().numpy(), grp.cpu().numpy()
    assert np.isfinite(chan).all() and np.isfinite(grp).all()
    one = ops.changroup_metrics(got[:1], 99, 2, EPS, TAU)
    assert one[0][0, 4:].tolist() == [0.0] * 4 and one[0][1, 4:].tolist() == [0.0] * 4 and one[1][1].item() == 0.0
    assert chan[0, 4:].sum() == pytest.approx(1.0, rel=1e-12)  # sample 1 alone contributes


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc,G", [(8, 2), (132, 33), (3, None)])
def test_nan_and_inf_stay_where_they_are(cuda, Cc, G, dt):
    """a NaN in (1, 5), +inf in (2, 0), +inf and -inf in (0, 2): the sums of exactly those (b, c) are non-finite (as IEEE sums
    are), the group metrics of exactly those (b, group), the sample metrics of exactly those channels"""
    from vaehip import ops
    x = R.draw((3, 7, 13, Cc), Cc).to(dt)
    marks = [(1, min(5, Cc - 1), float("nan")), (2, 0, float("inf"))]
    for b, c, v in marks:
        x[b, 3, 4, c] = v
    x[0, 1, 1, 2], x[0, 5, 2, 2] = float("inf"), float("-inf")
    marks.append((0, 2, None))
    x = x.to(cuda)
    got = ops.changroup(x)
    _check(got, x, groups=G)
    s = got.cpu().numpy()
    bad = {(b, c) for b, c, _ in marks}
    assert {(b, c) for b in range(3) for c in range(Cc) if not np.isfinite(s[b, c]).all()} == bad
    assert np.isnan(s[0, 2, 0]) and s[0, 2, 1] == np.inf and s[0, 2, 2] == np.inf and s[2, 0, 0] == np.inf
    for b in range(3):
        chan, grp, _ = ops.changroup_metrics(got[b:b + 1], 7 * 13, G, EPS, TAU)
        chan, grp = chan.cpu().numpy(), grp.cpu().numpy()
        cols = {c for bb, c in bad if bb == b}
        assert {c for c in range(Cc) if not np.isfinite(chan[2:4, c]).all()} == cols
        if G is not None:
            cg = Cc // G
            assert {g for g in range(G) if not (np.isfinite(chan[:2, g * cg:(g + 1) * cg]).all() and np.isfinite(grp[g]))} == {c // cg for c in cols}


def test_repeatable(cuda):
    from vaehip import ops
    torch.manual_seed(6)
    for dt, xf in ((F32, 0), (BF16, 2), (F32, 1)):
        x = torch.randn((3, 40, 56, 256), device=cuda).to(dt)
        st = _stats(3, 256, cuda, 1) if xf else None
        a, b = ops.changroup(x, st, xf), ops.changroup(x, st, xf)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    x = torch.randn((2, 9, 11, 3), device=cuda)
    assert torch.equal(ops.changroup(x).view(torch.int64), ops.changroup(x).view(torch.int64))


@pytest.mark.parametrize("dt", DTYPES)
def test_offset_and_prefix_views_are_read_in_place(cuda, dt):
    """x5[..., 1:] (4 channels, pixel stride 5, base 4 / 2 bytes off: the single-channel path), x12[..., 4:8] (the vector path at a
    stride of 12), x4[..., :3] behind a transform with rows as wide as the buffer; what lies around the view is 1e6 or NaN"""
    from vaehip import ops
    x5 = R.draw((2, 7, 13, 5), 71).to(dt)
    x5[..., 0] = float("nan")
    x = x5.to(cuda)[..., 1:]
    _check(ops.changroup(x), x, vec=False)
    x12 = R.draw((2, 7, 13, 12), 72).to(dt)
    x12[..., :4], x12[..., 8:] = 1e6, float("nan")
    x = x12.to(cuda)[..., 4:8]
    _check(ops.changroup(x), x, vec=True)
    x4 = R.draw((3, 7, 13, 4), 73).to(dt)
    x4[..., 3] = 1e6
    dev4 = x4.to(cuda)
    x = dev4[..., :3]
    st = _stats(3, 4, cuda, 9)
    _check(ops.changroup(x, st, 2), x, st, 2)
    assert torch.equal(dev4.cpu().view(torch.int16 if dt == BF16 else torch.int32), x4.view(torch.int16 if dt == BF16 else torch.int32))


@pytest.mark.parametrize("case", ["c260_f32", "c512_bf16_silu", "c128_f32_affine", "c8_bf16", "c3_f32", "c3_bf16", "view3of4_bf16_silu",
                                  "offset4of5_f32", "c4_1pixel"])
def test_guarded_memory(cuda, case):
    """operands, workspace and result in guarded, poisoned blocks, on the vector and the scalar path: no store outside a block, no
    unwritten result or workspace word, no operand changed, and the result is that of the plain run bit for bit"""
    from vaehip import ops
    from vaehip.ops import Stats
    pool = GuardedPool(cuda)
    dt = BF16 if "bf16" in case else F32
    xf = 2 if "silu" in case else (1 if "affine" in case else 0)
    vec = None
    if case.startswith("view3of4"):
        x4 = R.draw((2, 12, 20, 4), 70).to(dt)
        x4[..., 3] = 1e6
        x, ld = pool.put(x4, "x4")[..., :3], 4
    elif case.startswith("offset4of5"):
        x5 = R.draw((2, 12, 20, 5), 71).to(dt)
        x5[..., 0] = 1e6
        x, ld, vec = pool.put(x5, "x5")[..., 1:], 5, False
    elif case == "c4_1pixel":
        x, ld = pool.put(R.draw((2, 1, 1, 4), 72), "x"), 4
    else:
        Cc = int(case.split("_")[0][1:])
        x, ld = pool.put(R.draw((2, 12, 20, Cc), 74).to(dt), "x"), Cc
    st = Stats(None, None, *(pool.put(t, n) for t, n in zip(R.stats_rows(2, ld, 3), ("scale", "shift")))) if xf else None
    plain = ops.changroup(x, st, xf)
    torch.cuda.synchronize()
    pool.snapshot()
    with guarded(pool, ops):
        got = ops.changroup(x, st, xf)
    torch.cuda.synchronize()
    assert len(pool.blocks) == (5 if xf else 3)  # the operand(s), the workspace and the result
    assert pool.violations() == [] and pool.changed() == []
    assert pool.unwritten_report() == []
    pool.block_of(got)  # the result is a pool tensor
    assert torch.equal(got.view(torch.int64), plain.view(torch.int64))
    _check(got, x, st, xf, vec=vec)


def test_argument_errors_are_refused_and_nothing_is_launched(cuda):
    from vaehip import ops
    from vaehip.lib import lib, VaeHipError
    B, H, W, Cc, nch = 2, 8, 8, 8, 2
    x = R.draw((B, H, W, Cc), 12).to(cuda)
    one = torch.ones((B, Cc), device=cuda)
    ws = torch.full((B * nch * Cc * 3 + 2,), -1.0, device=cuda, dtype=torch.float64)
    sums = torch.full((B, Cc, 3), -1.0, device=cuda, dtype=torch.float64)
    p = ops._p

    def partial(xp=p(x), sc=None, sh=None, xf=0, B=B, HW=H * W, Cc=Cc, ld=Cc, nch=nch, wsp=p(ws)):
        lib.call("vae_changroup_partial", xp, 0, sc, sh, xf, B, HW, Cc, ld, nch, wsp, ops._stream())

    for kw, msg in [(dict(xp=None), "null args"), (dict(wsp=None), "null args"), (dict(ld=Cc - 1), "pixel stride"),
                    (dict(nch=H * W // 2 + 1), "empty chunk"), (dict(xf=1), "xf needs scale and shift"),
                    (dict(xf=2, sh=p(one)), "xf needs scale and shift"), (dict(xf=3, sc=p(one), sh=p(one)), "xf=3"),
                    (dict(wsp=ws.data_ptr() + 8), "unaligned workspace"), (dict(B=32768, HW=65536), "2\\^31"), (dict(Cc=0), "bad args")]:
        with pytest.raises(VaeHipError, match="changroup_partial.*" + msg):
            partial(**kw)
    with pytest.raises(VaeHipError, match="changroup_final.*null args"):
        lib.call("vae_changroup_final", p(ws), B, H * W, Cc, nch, None, ops._stream())
    with pytest.raises(VaeHipError, match="changroup_final.*unaligned workspace"):
        lib.call("vae_changroup_final", ws.data_ptr() + 8, B, H * W, Cc, nch, p(sums), ops._stream())
    with pytest.raises(VaeHipError, match="changroup_final.*2\\^31"):
        lib.call("vae_changroup_final", p(ws), 32768, 65536, Cc, 1, p(sums), ops._stream())
    torch.cuda.synchronize()
    assert bool((ws == -1).all()) and bool((sums == -1).all())  # nothing was launched by any of them
    with pytest.raises(ValueError, match="changroup: a GroupNorm transform \\(xf\\) needs its stats"):
        ops.changroup(x, None, 2)
    with pytest.raises(ValueError, match="changroup: expected NHWC rows with contiguous channels"):
        ops.changroup(x.permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match="changroup: expected a 4-D NHWC fp32 / bf16 CUDA tensor"):
        ops.changroup(x.double())
    with pytest.raises(ValueError, match="changroup: stats rows"):
        ops.changroup(x, _stats(B, Cc + 1, cuda, 1), 1)
    # and the same arguments, valid, run
    partial()
    lib.call("vae_changroup_final", p(ws), B, H * W, Cc, nch, p(sums), ops._stream())
    s, rad = R.ref_sums(x)
    R.assert_sums_close(sums.cpu().numpy(), s, rad * 2)  # (two chunks where the op takes one: a chain of D + 1 <= 2 D additions)


# ---------------------------------------------------------------------------------------------------- engine
NORM_IN = "vae.decoder.up_blocks.1.resnets.0.norm2"   # a GroupNorm's input: the output of the convolution below
CONV_OUT = "vae.decoder.up_blocks.1.resnets.0.conv1"  # a convolution that feeds a GroupNorm
OLD = ["mean_abs_activation_per_channel", "abs_max_activation_per_channel"]


class _Spy:
    """counts the calls of ops.changroup and keeps (arguments, result)"""

    def __enter__(self):
        from vaehip import ops
        self.ops, self.real, self.calls = ops, ops.changroup, []

        def spy(x, *a, **kw):
            out = self.real(x, *a, **kw)
            self.calls.append(((x.clone(),) + a, out))  # a copy: the engine may reuse the buffer
            return out
        ops.changroup = spy
        return self

    def __exit__(self, *exc):
        self.ops.changroup = self.real


def _setup(cuda, mode, targets, device_metrics=True):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from vaehip.trainer import HipTrainer
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), 7))
    w.to(cuda)
    tr = HipTrainer(w, lr=1e-4, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mode)
    cfg = {"enabled": True, "track_interval": 1, "device_metrics": device_metrics, "near_zero_threshold": TAU, "target_layers": targets}
    return w, tr, (ActivityMonitor(w, cfg) if targets is not None else None)


def _batch(cuda, B=3, step=1):
    import vae_oracle as vo
    return vo.synthetic_pixels(B, 32, 5, step).to(cuda), vo.synthetic_eps(B, 32, 5, step).to(cuda)


def _map_metrics(fmap, G, eps, tau=TAU):
    """the torch formulas (the hook path's) on a full_activation_map [B, C, H, W] -> (metrics, bounds from the accumulation of a
    device pass over the same values)"""
    from tracking.monitor import changroup_summary, per_sample_sums
    from vaehip import ops
    t = fmap if isinstance(fmap, torch.Tensor) else torch.from_numpy(np.asarray(fmap))
    B, Cc, H, W = t.shape
    chan, grp, S = ops.changroup_metrics(per_sample_sums(t), H * W, G, eps, tau)
    nhwc = t.permute(0, 2, 3, 1).contiguous()
    sums, rad = R.ref_sums(nhwc)
    return changroup_summary(chan.numpy(), grp.numpy(), S), R.metric_bounds(sums, rad, H * W, G, eps, tau), R.ref_metrics(R.values(nhwc)[0], G, eps, tau)


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_device_metrics_against_the_torch_formulas_on_the_full_map(cuda, mode):
    """one forward per step(): the map is the tensor the pass read (an fp32 copy, exact for bf16 storage), so the device metrics
    must lie in the interval the accumulation leaves around the float64 values of that map; the hook path's values too"""
    targets = [{"name": NORM_IN, "capture_point": "input", "metrics": FIVE + ["full_activation_map"]},
               {"name": CONV_OUT, "capture_point": "output", "metrics": ["full_activation_map"] + FIVE, "groups": 8}]
    w, tr, mon = _setup(cuda, mode, targets)
    ids = [NORM_IN + ".input", CONV_OUT + ".output"]
    assert mon.device_layers == ids and not [n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks]
    norm = w.get_submodule(NORM_IN)
    with _Spy() as spy:
        tr.train_step(*_batch(cuda))
        log = mon.step(1)
    assert len(spy.calls) == 2 and all(c[1].shape == (3, norm.num_channels, 3) for c in spy.calls)  # one pass per point and forward
    data = mon.get_data_for_step(1)
    for lid, G, eps in ((ids[0], norm.num_groups, norm.eps), (ids[1], 8, 1e-6)):
        got = data[lid]
        assert [k for k in got if k != "full_activation_map"] == FIVE
        mine, bounds, ref = _map_metrics(got["full_activation_map"], G, eps)
        R.assert_within(got, bounds, ref)
        R.assert_within(mine, bounds)
        R.assert_share_bound_small(bounds, norm.num_channels, G)
        assert got[DOM].shape == (G,) and all(got[k].dtype == np.float32 for k in FIVE)
        assert f"tracking/{lid}/{SHARE}_squashed_channels" in log and f"tracking/{lid}/{DOM}_most_dominated_group" in log
    # the two points see the same tensor: their sample metrics agree bit for bit
    assert np.array_equal(data[ids[0]][ACTIVE], data[ids[1]][ACTIVE]) and np.array_equal(data[ids[0]][VARIATION], data[ids[1]][VARIATION])
    mon.remove_hooks()
    # the same targets on torch hooks give the same keys and, from the same weights and batch, values inside the same intervals
    w2, tr2, mon2 = _setup(cuda, mode, targets, device_metrics=False)
    assert mon2.device_layers == []
    with _Spy() as spy:
        tr2.train_step(*_batch(cuda))
        log2 = mon2.step(1)
    assert spy.calls == [] and set(log2) == set(log)
    for lid, G, eps in ((ids[0], norm.num_groups, norm.eps), (ids[1], 8, 1e-6)):
        _, bounds, ref = _map_metrics(mon2.get_data_for_step(1)[lid]["full_activation_map"], G, eps)
        R.assert_within(mon2.get_data_for_step(1)[lid], bounds, ref)
    mon2.remove_hooks()


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_planted_outlier_filter(cuda, mode):
    """one filter row (its bias with it: the channel times 100) of a convolution that feeds a GroupNorm times 100: the channel takes over its group's variance, its
    group-mates all but vanish behind the norm, and no other group notices.  The row is the one whose output has the smallest
    |mean| / sigma before (read from the baseline sums): a channel far off the group's mean would, scaled, drag that mean along
    and inflate its mates' deviations too -- what GroupNorm does with it, but not the case this test plants"""
    targets = [{"name": CONV_OUT, "capture_point": "output", "metrics": [SHARE, NRMS, DOM]}]
    w, tr, mon = _setup(cuda, mode, targets)
    conv, norm = w.get_submodule(CONV_OUT), w.get_submodule(NORM_IN)
    G, Cc = norm.num_groups, norm.num_channels
    cg = Cc // G
    x = _batch(cuda)[0]
    w.eval()
    with _Spy() as spy:
        tr.eval_step(x)
    mon.step(1)
    base = mon.get_data_for_step(1)[CONV_OUT + ".output"]
    s = spy.calls[0][1].cpu().numpy()
    n = spy.calls[0][0][0].shape[1] * spy.calls[0][0][0].shape[2]
    mean, var = s[:, :, 0] / n, np.maximum(s[:, :, 1] / n - (s[:, :, 0] / n) ** 2, 0)
    o = int(np.argmin((np.abs(mean) / np.sqrt(var)).max(axis=0)))
    with torch.no_grad():
        conv.weight[o] *= 100.0
        conv.bias[o] *= 100.0
    with _Spy() as spy2:
        tr.eval_step(x)
    mon.step(2)
    got = mon.get_data_for_step(2)[CONV_OUT + ".output"]
    g = o // cg
    mates = [c for c in range(g * cg, (g + 1) * cg) if c != o]
    print(f"{mode}: row {o} of group {g}: share {base[SHARE][o]:.3f} -> {got[SHARE][o]:.4f}, mates' normalized rms "
          f"{base[NRMS][mates]} -> {got[NRMS][mates]}")
    assert got[SHARE][o] > 0.9 and got[DOM][g] > 0.9
    assert (got[NRMS][mates] < 0.1 * base[NRMS][mates]).all()
    # the other groups: their sums may move by the accumulation's radius at most (the convolution computes a channel from its own
    # filter row), and so their metrics stay inside the interval around the baseline's sums
    s2 = spy2.calls[0][1].cpu().numpy()
    nhwc = spy.calls[0][0][0]
    sums, rad = R.ref_sums(nhwc)
    others = np.array([c for c in range(Cc) if c // cg != g])
    R.assert_sums_close(s2[:, others], sums[:, others], rad[:, others])
    bounds = R.metric_bounds(sums, rad, n, G, norm.eps, TAU)
    for k in (SHARE, NRMS):
        lo, hi = bounds[k]
        assert ((lo[others] <= got[k][others]) & (got[k][others] <= hi[others])).all(), k
    lo, hi = bounds[DOM]
    og = np.array([q for q in range(G) if q != g])
    assert ((lo[og] <= got[DOM][og]) & (got[DOM][og] <= hi[og])).all()
    mon.remove_hooks()


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_without_a_target_launches_nothing_and_the_step_is_bitwise_the_same(cuda, mode):
    """a monitor whose targets name none of the five metrics never calls ops.changroup, and its step's scalars and gradients are
    bit for bit those of a step without a monitor; trackers that do name them only read: the same bits again"""
    bits = lambda t: t.detach().clone().view(torch.int32)  # noqa: E731
    old = [{"name": NORM_IN, "capture_point": "input", "metrics": OLD}, {"name": CONV_OUT, "capture_point": "output", "metrics": OLD}]
    w, tr, _ = _setup(cuda, mode, None)
    x, eps = _batch(cuda)
    r0 = w.vae.engine.forward_backward(x, eps, 1e-6)
    s0, g0 = bits(r0["scalars"]), bits(w.vae.arena.grad)
    w1, tr1, mon1 = _setup(cuda, mode, old)
    with _Spy() as spy:
        r1 = w1.vae.engine.forward_backward(x, eps, 1e-6)
        log1 = mon1.step(1)
    assert spy.calls == [] and not any(m in k for k in log1 for m in FIVE)
    assert torch.equal(bits(r1["scalars"]), s0) and torch.equal(bits(w1.vae.arena.grad), g0)
    assert set(mon1.get_data_for_step(1)[NORM_IN + ".input"]) == set(OLD)
    mon1.remove_hooks()
    new = [dict(t, metrics=t["metrics"] + FIVE) for t in old]
    w2, tr2, mon2 = _setup(cuda, mode, new)
    with _Spy() as spy:
        r2 = w2.vae.engine.forward_backward(x, eps, 1e-6)
        log2 = mon2.step(1)
    assert len(spy.calls) == 2
    assert torch.equal(bits(r2["scalars"]), s0) and torch.equal(bits(w2.vae.arena.grad), g0)
    assert {k: v for k, v in log2.items() if not any(m in k for m in FIVE)}.keys() == log1.keys()  # the old keys, unchanged
    mon2.remove_hooks()
    with _Spy() as spy:
        w2.vae.engine.forward_backward(x, eps, 1e-6)
    assert spy.calls == []  # removed: nothing is launched any more


def test_engine_shares_one_pass_among_the_trackers_of_a_point(cuda):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    w = SDXLVAEWrapper("synthetic:1")
    w.to(cuda)
    eng = w.vae.engine
    norm1 = w.vae.encoder.down_blocks[0].resnets[0].norm1
    seen = {"a": [], "b": [], "old": []}
    hs = [eng.add_tracker(norm1, "output", lambda m, f, changroup=None: seen["a"].append((m, f, changroup)), metrics=[SHARE]),
          eng.add_tracker(norm1, "output", lambda m, f, changroup=None: seen["b"].append((m, f, changroup)), metrics=[ACTIVE, "mean_activation"]),
          eng.add_tracker(norm1, "output", lambda m, f: seen["old"].append((m, f)), metrics=["std_activation"])]
    with _Spy() as spy:
        try:
            with torch.no_grad():
                w.vae.encode(vo.synthetic_pixels(2, 32, 1, 1).to(cuda))
        finally:
            for h in hs:
                h.remove()
    assert len(spy.calls) == 1 and len(seen["a"]) == len(seen["b"]) == len(seen["old"]) == 1
    assert seen["a"][0][2] is seen["b"][0][2] and seen["a"][0][0] is None and seen["b"][0][0] is seen["old"][0][0]
    sums, HW = seen["a"][0][2]
    assert sums.shape == (2, 128, 3) and sums.dtype == torch.float64 and HW == 32 * 32
    assert spy.calls[0][0][2] == 1 and spy.calls[0][0][1] is not None  # the GroupNorm's output is never materialised: the pass applies the affine itself


# ---------------------------------------------------------------------------------------------------- CLI
def test_train_cli_with_the_group_dynamics_config(cuda, tmp_path):
    """src/train.py with configs/experiment_synthetic_group_dynamics.yaml: the CSV carries the five metrics' record kinds for the
    three capture points, with values in their ranges"""
    import yaml
    src = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
    c = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_group_dynamics.yaml")))
    assert c["tracking"]["device_metrics"] is True
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
    names = {SHARE: "group_variance_share", NRMS: "normalized_rms", DOM: "group_dominance", ACTIVE: "active_sample_fraction",
             VARIATION: "sample_variation"}
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    model = SDXLVAEWrapper(c["model"]["pretrained_vae_name"])
    for name, point in (("vae.decoder.up_blocks.0.resnets.0.norm1", "input"), ("vae.decoder.conv_norm_out", "input"),
                        ("vae.decoder.up_blocks.1.resnets.0.conv1", "output")):
        lid, mod = f"{name}.{point}", model.get_submodule(name)
        uniform = 32.0 / (mod.out_channels if hasattr(mod, "out_channels") else mod.num_channels)  # 1 / cg
        for n in names.values():
            for sfx in ("_overall_mean", "_overall_min", "_overall_max"):
                assert (lid, n + sfx) in val, (lid, n + sfx)
        for k in ("group_variance_share_squashed_channels", "group_dominance_argmax_group", "active_sample_fraction_silent_channels"):
            assert (lid, k) in val, (lid, k)
        assert 0.0 <= float(val[(lid, "group_variance_share_overall_min")]) <= float(val[(lid, "group_variance_share_overall_max")]) <= 1.0
        # the shares of a group sum to 1 in every sample: their mean over the channels is 1 / cg
        assert float(val[(lid, "group_variance_share_overall_mean")]) == pytest.approx(uniform, rel=1e-5)
        assert uniform * (1 - 1e-6) <= float(val[(lid, "group_dominance_overall_min")]) and float(val[(lid, "group_dominance_overall_max")]) <= 1.0
        assert 0 <= int(float(val[(lid, "group_dominance_argmax_group")])) < 32
        assert 0.0 <= float(val[(lid, "active_sample_fraction_overall_min")]) <= float(val[(lid, "active_sample_fraction_overall_max")]) <= 1.0
        assert float(val[(lid, "sample_variation_overall_min")]) >= 0.0 and float(val[(lid, "normalized_rms_overall_max")]) > 0.0
    assert ("vae.decoder.conv_norm_out.input", "scalar") in val  # the all-metrics run's rows are still there
    assert ("vae.encoder.down_blocks.0.resnets.0.norm1.output", "per_channel_overall_mean") in val
