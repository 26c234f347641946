"""ops.chanhist (csrc/chanhist.hip): per-channel magnitude histogram, near-zero count and max |y| in one read.

Untransformed input: integer / bit equality with tests/chanhist_refs.ref_exact.  Transformed input (GroupNorm affine, with or
without SiLU): the device evaluates y in fp32 (v_exp / v_rcp), so an element within its error radius of a bin edge or of tau may
be counted on either side; the reference evaluates y in float64 with a radius per element (chanhist_refs.ref_transformed) and
every device count must lie between the certain count and certain + uncertain.  The radii: one rounding per product and per sum
for the affine (2^-21 (|x scale| + |shift|), four times the two half-ulp roundings), and for SiLU 10 % more plus 2^-20 |y| for
the few ulp of exp and rcp.  Over all transformed cases together at most 1e-4 of the elements may be uncertain
(test_uncertain_share_of_the_transformed_cases, last of its group): 2.2e-5 on the moments suite's generators.

Then the engine (hook path against device path on the small synthetic VAE) and src/train.py on the new config."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chanhist_refs as R
from guarded import GuardedPool, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIST, AMAX, NZ = "log2_histogram_per_channel", "abs_max_activation_per_channel", "near_zero_fraction_per_channel"
THREE = [HIST, AMAX, NZ]
CHANNELS = (1, 3, 4, 8, 128, 256, 257, 512)
SHAPES = [(1, 7, 13), (3, 16, 16), (3, 7, 13), (1, 32, 24)]
DTYPES = [torch.float32, torch.bfloat16]
TAU = 1e-3
TALLY = {"uncertain": 0, "n": 0, "cases": 0}


def _stats(B, ld, dev, seed):
    from vaehip.ops import Stats
    sc, sh = R.stats_rows(B, ld, seed)
    return Stats(None, None, sc.to(dev), sh.to(dev))


def _wide(shape, seed):
    """values over every bin: the moments suite's randn * 1.3 + 0.4 times 2^k, k uniform in [-40, 22], and a few exact zeros"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 1.3 + 0.4) * torch.pow(2.0, torch.randint(-40, 23, shape, generator=g).float())
    x[torch.rand(shape, generator=g) < 0.02] = 0.0
    return x


def _same_bits(got: np.ndarray, ref: np.ndarray):
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


def _assert_exact(got, x, tau=TAU):
    hist, nz, amax = (t.cpu().numpy() for t in got)
    rh, rn, ra = R.ref_exact(x, tau)
    assert hist.dtype == np.int64 and nz.dtype == np.int64 and amax.dtype == np.float32
    assert hist.shape == rh.shape and (hist.sum(axis=1) == x.shape[0] * x.shape[1] * x.shape[2]).all()
    assert np.array_equal(hist, rh), np.argwhere(hist != rh)[:8]
    assert np.array_equal(nz, rn)
    assert _same_bits(amax, ra), (amax, ra)


# ---------------------------------------------------------------------------------------------------- untransformed: exact
@pytest.mark.parametrize("B,H,W", SHAPES + [(1, 1, 1)])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_exact_against_the_bit_pattern_reference(cuda, Cc, dt, B, H, W):
    from vaehip import ops
    x = _wide((B, H, W, Cc), Cc * 131 + B * 7 + H).to(cuda).to(dt)
    _assert_exact(ops.chanhist(x, tau=TAU), x)


@pytest.mark.parametrize("Cc,B,H,W,layout,dt,xf", R.frame_params((0, 1, 2)))
def test_at_the_edges_of_the_shared_frame(cuda, Cc, B, H, W, layout, dt, xf):
    """exact without a transform, inside the float64 bounds with one"""
    from vaehip import ops
    if xf == 0:
        x = R.frame_layout(_wide((B, H, W, Cc), Cc * 131 + B * 7 + H).clamp(-6e4, 6e4).to(cuda).to(dt), layout)
        _assert_exact(ops.chanhist(x, tau=TAU), x)
    else:
        g = torch.Generator(device="cpu").manual_seed(Cc * 131 + xf * 7 + B)
        x = R.frame_layout((torch.randn((B, H, W, Cc), generator=g) * 1.3 + 0.4).to(cuda).to(dt), layout)
        st = _stats(B, x.stride(2), cuda, Cc + xf)
        _assert_bounded(ops.chanhist(x, st, xf, TAU), x, st, xf)


@pytest.mark.parametrize("dt", DTYPES)
def test_exact_on_a_channel_prefix_view(cuda, dt):
    """the encoder's input: the 3-channel view x4[..., :3] of a 4-channel buffer, read in place; the pad channel must not leak"""
    from vaehip import ops
    x4 = _wide((3, 7, 13, 4), 5).clamp(-6e4, 6e4).to(cuda).to(dt)
    x4[..., 3] = 1e6  # would land in the top bin, which nothing else here reaches
    x = x4[..., :3]
    got = ops.chanhist(x)
    assert got[0].shape == (3, 48) and int(got[0][:, 47].sum()) == 0 and float(got[2].max()) <= 6e4
    _assert_exact(got, x)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc", [3, 4, 130])
def test_exact_on_the_bin_edges(cuda, Cc, dt):
    """zeros, a denormal, 2^-30, 1, 65504, 2^16 and their neighbours, infinities and a NaN, rolled along the pixels per channel;
    every second channel has its NaN replaced, so both a NaN maximum and an infinite one are produced"""
    from vaehip import ops
    v = R.edge_values()
    n = len(v)
    x = torch.stack([torch.roll(v, c) for c in range(Cc)], dim=1).reshape(1, 1, n, Cc).repeat(2, 3, 1, 1).contiguous()
    x[..., 0::2] = torch.nan_to_num(x[..., 0::2], nan=1.0, posinf=float("inf"), neginf=float("-inf"))
    if dt == torch.bfloat16:  # the fp32 neighbours of the edges round onto the edges: add the bf16 numbers just below 2^-30 and 2^16
        x = x.to(dt)
        x[0, 0, :2, 0] = torch.tensor([0x307F, 0x477F], dtype=torch.int16).view(dt)
    x = x.to(cuda)
    got = ops.chanhist(x)
    _assert_exact(got, x)
    hist = got[0].cpu().numpy()
    want = np.bincount([b for _, b in R.EDGES], minlength=48) * 6
    if dt == torch.float32:
        assert np.array_equal(hist[1], want)                       # a channel with the NaN
        assert np.isnan(got[2].cpu().numpy()[1::2]).all() and np.isinf(got[2].cpu().numpy()[0::2]).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc,B,H,W", [(128, 3, 16, 16), (4, 2, 16, 24), (1, 1, 40, 40), (257, 1, 7, 13)])
def test_exact_when_every_lane_hits_one_counter(cuda, Cc, B, H, W, dt):
    """a dead channel and a constant one: all their values fall into one bin, the worst case for the LDS atomics"""
    from vaehip import ops
    x = _wide((B, H, W, Cc), 11 + Cc)
    x[..., 0] = 3.0
    if Cc > 1:
        x[..., 1] = 0.0
    x = x.to(cuda).to(dt)
    got = ops.chanhist(x)
    _assert_exact(got, x)
    n = B * H * W
    hist, nz, amax = (t.cpu().numpy() for t in got)
    assert hist[0, 32] == n and nz[0] == 0 and amax[0] == 3.0
    if Cc > 1:
        assert hist[1, 0] == n and nz[1] == n and amax[1] == 0.0


def test_tau_is_compared_in_fp32(cuda):
    from vaehip import ops
    for tau in (1e-3, 0.25, 0.0):
        v = R.tau_edge_values(tau) if tau else torch.tensor([0.0, -0.0, 1e-45, 1.0, -1.0, 2.0])
        x = v.reshape(1, 1, -1, 1).repeat(1, 2, 1, 4).contiguous().to(cuda)
        got = ops.chanhist(x, tau=tau)
        _assert_exact(got, x, tau)
        assert got[1].tolist() == [4 if tau else 0] * 4


# ---------------------------------------------------------------------------------------------------- transformed: bounded
def _assert_bounded(got, x, st, xf, tau=TAU):
    hist, nz, amax = (t.cpu().numpy() for t in got)
    y, d = R.ref_transformed(x, st.scale, st.shift, xf)
    bd = R.check_within_bounds(hist, nz, amax, y, d, tau, x.shape[0] * x.shape[1] * x.shape[2])
    return bd


@pytest.mark.parametrize("B,H,W", SHAPES + [(1, 1, 1)])
@pytest.mark.parametrize("xf", [1, 2])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_transformed_within_the_float64_bounds(cuda, Cc, dt, xf, B, H, W):
    from vaehip import ops
    g = torch.Generator(device="cpu").manual_seed(Cc * 131 + xf * 7 + B)
    x = (torch.randn((B, H, W, Cc), generator=g) * 1.3 + 0.4).to(cuda).to(dt)
    st = _stats(B, Cc, cuda, Cc + xf)
    bd = _assert_bounded(ops.chanhist(x, st, xf, TAU), x, st, xf)
    print(f"C={Cc} {str(dt)[6:]} xf={xf} {B}x{H}x{W}: {bd['uncertain']} of {bd['n']} elements uncertain")
    TALLY["uncertain"] += bd["uncertain"]
    TALLY["n"] += bd["n"]
    TALLY["cases"] += 1


@pytest.mark.parametrize("xf", [1, 2])
@pytest.mark.parametrize("dt", DTYPES)
def test_transformed_channel_prefix_view(cuda, dt, xf):
    from vaehip import ops
    g = torch.Generator(device="cpu").manual_seed(5)
    x4 = (torch.randn((3, 7, 13, 4), generator=g) - 0.2).to(cuda).to(dt)
    x4[..., 3] = 1e6
    x = x4[..., :3]
    st = _stats(3, 4, cuda, 9)
    bd = _assert_bounded(ops.chanhist(x, st, xf), x, st, xf)
    TALLY["uncertain"] += bd["uncertain"]
    TALLY["n"] += bd["n"]
    TALLY["cases"] += 1


def test_uncertain_share_of_the_transformed_cases(cuda):
    """the bounds above say something only while almost every element is certain of its bin"""
    assert TALLY["cases"] == len(CHANNELS) * 2 * 2 * 5 + 4, "run this module whole: the tally is over all transformed cases"
    share = TALLY["uncertain"] / TALLY["n"]
    print(f"uncertain share {share:.3e} ({TALLY['uncertain']} of {TALLY['n']} elements, {TALLY['cases']} cases)")
    assert share <= 1e-4, share


# ---------------------------------------------------------------------------------------------------- other kernel checks
def test_repeatable(cuda):
    from vaehip import ops
    torch.manual_seed(6)
    for dt, xf in ((torch.float32, 0), (torch.bfloat16, 2)):
        x = torch.randn((3, 40, 56, 256), device=cuda).to(dt)
        st = _stats(3, 256, cuda, 1) if xf else None
        a = ops.chanhist(x, st, xf)
        b = ops.chanhist(x, st, xf)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
        assert int(a[0].sum()) == x.numel()
    x = torch.randn((2, 9, 11, 3), device=cuda)
    assert all(torch.equal(u, v) for u, v in zip(ops.chanhist(x), ops.chanhist(x)))


@pytest.mark.parametrize("case", ["c257_f32", "view3of4_f32", "view3of4_bf16_silu", "c128_bf16_silu", "c512_f32_affine", "c4_1pixel"])
def test_guarded_memory(cuda, case):
    """operands, workspace and results in guarded, poisoned blocks: no store outside a block, no unwritten result or workspace
    word, no operand changed, and the values are still right (a load outside an operand would have met NaN)"""
    from vaehip import ops
    from vaehip.ops import Stats
    pool = GuardedPool(cuda)
    g = torch.Generator().manual_seed(70)
    if case == "c257_f32":
        x, st, xf = pool.put(_wide((2, 12, 20, 257), 71), "x"), None, 0
    elif case.startswith("view3of4"):
        dt = torch.bfloat16 if "bf16" in case else torch.float32
        x4 = (torch.randn((2, 12, 20, 4), generator=g) + 0.4).to(dt)
        x4[..., 3] = 1e6
        x = pool.put(x4, "x4")[..., :3]
        xf = 2 if "silu" in case else 0
        st = Stats(None, None, *(pool.put(t, n) for t, n in zip(R.stats_rows(2, 4, 3), ("scale", "shift")))) if xf else None
    elif case == "c4_1pixel":
        x, st, xf = pool.put(_wide((2, 1, 1, 4), 72), "x"), None, 0
    else:
        Cc = 128 if "c128" in case else 512
        dt = torch.bfloat16 if "bf16" in case else torch.float32
        x = pool.put((torch.randn((2, 12, 20, Cc), generator=g) * 1.3 + 0.4).to(dt), "x")
        xf = 2 if "silu" in case else 1
        st = Stats(None, None, *(pool.put(t, n) for t, n in zip(R.stats_rows(2, Cc, 4), ("scale", "shift"))))
    pool.snapshot()
    with guarded(pool, ops):
        got = ops.chanhist(x, st, xf)
    torch.cuda.synchronize()
    assert len(pool.blocks) >= 5  # the operands, the workspace and three results
    assert pool.violations() == [] and pool.changed() == []
    assert pool.unwritten_report() == []
    for t in got:
        pool.block_of(t)  # the results are pool tensors
    if xf:
        _assert_bounded(got, x, st, xf)
    else:
        _assert_exact(got, x)


def test_argument_errors_are_refused_with_their_message(cuda):
    from vaehip import ops
    from vaehip.lib import lib, VaeHipError
    B, H, W, Cc, nch = 2, 8, 8, 8, 2
    x = torch.randn((B, H, W, Cc), device=cuda)
    one = torch.ones((B, Cc), device=cuda)
    ws = torch.full((B * nch * Cc * 50 + 4,), -1, device=cuda, dtype=torch.int32)
    hist = torch.full((Cc, 48), -1, device=cuda, dtype=torch.int64)
    nz = torch.full((Cc,), -1, device=cuda, dtype=torch.int64)
    amax = torch.full((Cc,), -1.0, device=cuda)
    p = ops._p

    def partial(xp=p(x), sc=None, sh=None, xf=0, B=B, HW=H * W, Cc=Cc, ld=Cc, nch=nch, tau=1e-3, wsp=p(ws)):
        lib.call("vae_chanhist_partial", xp, 0, sc, sh, xf, B, HW, Cc, ld, nch, tau, wsp, ops._stream())

    for kw, msg in [(dict(xp=None), "null args"), (dict(wsp=None), "null args"), (dict(ld=Cc - 1), "pixel stride"),
                    (dict(nch=H * W // 2 + 1), "empty chunk"), (dict(xf=1), "xf needs scale and shift"),
                    (dict(xf=2, sh=p(one)), "xf needs scale and shift"), (dict(wsp=ws.data_ptr() + 4), "unaligned workspace"),
                    (dict(tau=-0.5), "negative or NaN"), (dict(tau=float("nan")), "negative or NaN"),
                    (dict(B=32768, HW=65536), "2\\^31")]:
        with pytest.raises(VaeHipError, match="chanhist_partial.*" + msg):
            partial(**kw)
    with pytest.raises(VaeHipError, match="chanhist_final.*null args"):
        lib.call("vae_chanhist_final", p(ws), B, H * W, Cc, nch, p(hist), None, p(amax), ops._stream())
    with pytest.raises(VaeHipError, match="chanhist_final.*unaligned workspace"):
        lib.call("vae_chanhist_final", ws.data_ptr() + 4, B, H * W, Cc, nch, p(hist), p(nz), p(amax), ops._stream())
    with pytest.raises(VaeHipError, match="chanhist_final.*2\\^31"):
        lib.call("vae_chanhist_final", p(ws), 32768, 65536, Cc, 1, p(hist), p(nz), p(amax), ops._stream())
    torch.cuda.synchronize()
    # nothing was launched by any of them
    assert bool((ws == -1).all()) and bool((hist == -1).all()) and bool((nz == -1).all()) and bool((amax == -1).all())
    with pytest.raises(ValueError, match="needs its stats"):
        ops.chanhist(x, None, 2)
    with pytest.raises(ValueError, match="contiguous channels"):
        ops.chanhist(x.permute(0, 3, 1, 2))
    with pytest.raises(VaeHipError, match="negative or NaN"):
        ops.chanhist(x, tau=-1.0)
    # and the same arguments, valid, run
    partial()
    lib.call("vae_chanhist_final", p(ws), B, H * W, Cc, nch, p(hist), p(nz), p(amax), ops._stream())
    _assert_exact((hist, nz, amax), x)


# ---------------------------------------------------------------------------------------------------- engine
POINTS = [("vae.encoder.down_blocks.0.resnets.0.norm1", "output"),   # GroupNorm affine, fused: no tensor exists
          ("vae.encoder.down_blocks.0.resnets.0.conv1", "input"),    # ... + SiLU
          ("vae.encoder.down_blocks.0.resnets.0", "output"),
          ("vae.encoder", "input")]
KEY_OF = {(1, 128): "vae.encoder.down_blocks.0.resnets.0.norm1.output", (2, 128): "vae.encoder.down_blocks.0.resnets.0.conv1.input",
          (0, 128): "vae.encoder.down_blocks.0.resnets.0.output", (0, 3): "vae.encoder.input"}
ETAU = 0.05


def _run(cuda, device_metrics, mixed_precision, record=None):
    """steps 1 and 2 of a small run; step 2 buffers two forwards (a train step and an eval step)"""
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from vaehip import ops
    from vaehip.trainer import HipTrainer
    cfg = {"enabled": True, "track_interval": 1, "device_metrics": device_metrics, "near_zero_threshold": ETAU,
           "target_layers": [{"name": n, "capture_point": p, "metrics": list(THREE)} for n, p in POINTS]}
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), 7))
    w.to(cuda)
    tr = HipTrainer(w, lr=1e-4, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mixed_precision)
    mon = ActivityMonitor(w, cfg)
    real = ops.chanhist
    calls = []
    if record is not None:
        def spy(x, stats=None, xf=0, tau=1e-3):
            out = real(x, stats, xf, tau)
            calls.append((x.clone(), stats, xf, tau, out))
            return out
        ops.chanhist = spy
    logs, data = {}, {}
    R_, B = 32, 2
    try:
        for s in (1, 2):
            tr.train_step(vo.synthetic_pixels(B, R_, 5, s).to(cuda), vo.synthetic_eps(B, R_, 5, s).to(cuda))
            if s == 2:
                w.eval()
                tr.eval_step(vo.synthetic_pixels(B, R_, 5, 100).to(cuda))
                w.train()
            if record is not None:
                record[s] = list(calls)
                calls.clear()
            logs[s] = mon.step(s)
            data[s] = mon.get_data_for_step(s)
    finally:
        ops.chanhist = real
    torch.cuda.synchronize()
    recs = mon.export_all_processed_data_to_records()
    hooked = [n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks]
    layers = list(mon.device_layers)
    mon.remove_hooks()
    return logs, data, recs, hooked, layers


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_hook_path_against_device_path(cuda, mode):
    record = {}
    ld, dd, rd, hooked, layers = _run(cuda, True, mode, record)
    assert hooked == [] and sorted(layers) == sorted(KEY_OF.values())
    lh, dh, rh, hooked_h, layers_h = _run(cuda, False, mode)
    assert layers_h == [] and len(hooked_h) == 4
    n = 2 * 32 * 32
    for s, forwards in ((1, 1), (2, 2)):
        assert set(ld[s]) == set(lh[s]) and len(ld[s]) == 4 * 4  # step() returns the same keys from both paths
        assert list(dd[s]) == list(dh[s])
        calls = record[s]
        assert len(calls) == 4 * forwards  # one pass per capture point and forward
        assert all(c[3] == ETAU for c in calls)
        # every pass against its own reference, and the bounds of each layer summed over the step's forwards
        agg = {}
        for x, st, xf, tau, out in calls:
            lid = KEY_OF[(xf, x.shape[-1])]
            assert tuple(x.shape[:3]) == (2, 32, 32)
            if xf == 0:
                _assert_exact(out, x, tau)
                continue
            bd = _assert_bounded(out, x, st, xf, tau)
            y, d = R.ref_transformed(x, st.scale, st.shift, xf)
            k = np.abs(y).argmax(axis=0)
            a = agg.setdefault(lid, {"lo": 0, "unc": 0, "nzlo": 0.0, "nzhi": 0.0, "amax": [], "rad": []})
            a["lo"], a["unc"] = a["lo"] + bd["hist_lo"], a["unc"] + bd["hist_unc"]
            a["nzlo"], a["nzhi"] = a["nzlo"] + bd["nz_lo"] / n, a["nzhi"] + (bd["nz_lo"] + bd["nz_unc"]) / n
            a["amax"].append(np.abs(y)[k, np.arange(y.shape[1])])
            a["rad"].append(d[k, np.arange(y.shape[1])])
        for lid in dd[s]:
            got_d, got_h = dd[s][lid], dh[s][lid]
            assert list(got_d) == list(got_h) == THREE
            for got in (got_d, got_h):
                assert got[HIST].dtype == np.int64 and (got[HIST].sum(axis=1) == forwards * n).all()
            if lid not in agg:  # an untransformed capture point: the two paths read the same values
                assert np.array_equal(got_d[HIST], got_h[HIST]) and np.array_equal(got_d[NZ], got_h[NZ])
                assert _same_bits(got_d[AMAX], got_h[AMAX])
                continue
            a = agg[lid]  # a fused GroupNorm (+ SiLU): both paths are fp32 evaluations of the float64 values
            for got in (got_d, got_h):
                assert (a["lo"] <= got[HIST]).all() and (got[HIST] <= a["lo"] + a["unc"]).all()
                frac = got[NZ].astype(np.float64) * forwards
                assert (a["nzlo"] - 1e-6 <= frac).all() and (frac <= a["nzhi"] + 1e-6).all()
                top = np.stack(a["amax"]).max(axis=0)
                assert (np.abs(got[AMAX] - top) <= np.stack(a["rad"]).max(axis=0)).all()
    kinds = lambda recs: [(r["global_step"], r["layer_identifier"], r["original_metric_name"], r["metric_type"]) for r in recs]  # noqa: E731
    assert kinds(rd) == kinds(rh) and len(rd) == 2 * 4 * 11


def test_engine_shares_one_pass_among_the_trackers_of_a_point(cuda):
    """two registrations at one point and threshold share a pass; the old sink signature is still called with two arguments"""
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip import ops
    w = SDXLVAEWrapper("synthetic:1")
    w.to(cuda)
    eng = w.vae.engine
    norm1 = w.vae.encoder.down_blocks[0].resnets[0].norm1
    seen = {"a": [], "b": [], "old": []}
    hs = [eng.add_tracker(norm1, "output", lambda m, f, chanhist=None: seen["a"].append((m, f, chanhist)), metrics=[HIST]),
          eng.add_tracker(norm1, "output", lambda m, f, chanhist=None: seen["b"].append((m, f, chanhist)),
                          metrics=[NZ, "mean_activation"]),
          eng.add_tracker(norm1, "output", lambda m, f: seen["old"].append((m, f)), metrics=["std_activation"])]
    real, n = ops.chanhist, []
    ops.chanhist = lambda *a, **k: (n.append(1), real(*a, **k))[1]
    try:
        with torch.no_grad():
            w.vae.encode(vo.synthetic_pixels(1, 32, 1, 1).to(cuda))
    finally:
        ops.chanhist = real
        for h in hs:
            h.remove()
    assert len(n) == 1 and len(seen["a"]) == len(seen["b"]) == len(seen["old"]) == 1
    assert seen["a"][0][2] is seen["b"][0][2] and seen["a"][0][0] is None and seen["b"][0][0] is seen["old"][0][0]
    hist = seen["a"][0][2][0]
    assert hist.shape == (128, 48) and bool((hist.sum(dim=1) == 32 * 32).all())


# ---------------------------------------------------------------------------------------------------- CLI
def test_train_cli_with_the_channel_hist_config(cuda, tmp_path):
    """src/train.py with configs/experiment_synthetic_channel_hist.yaml: the CSV carries the new record kinds, and every
    histogram row sums to forwards x B*H*W"""
    import yaml
    src = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
    c = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_channel_hist.yaml")))
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
    # 10 training forwards and the 2 validation batches of the first epoch (16 samples) before the tracker fires at step 10
    forwards, n = 12, 8 * 32 * 32
    for lid, Cc in (("vae.encoder.down_blocks.0.resnets.0.norm1.output", 128), ("vae.encoder.down_blocks.0.resnets.0.conv1.input", 128),
                    ("vae.encoder.down_blocks.0.resnets.0.output", 128), ("vae.encoder.input", 3)):
        for k in ("histogram_shape", "histogram_row_total", "histogram_top_bin_count", "histogram_zero_bin_count", "histogram_median_bin",
                  "abs_max_overall_max", "abs_max_overall_mean", "abs_max_argmax_channel", "near_zero_overall_mean",
                  "near_zero_overall_max", "near_zero_dead_channels"):
            assert (lid, k) in val, (lid, k)
        assert val[(lid, "histogram_shape")] == f"({Cc}, 48)"
        assert int(float(val[(lid, "histogram_row_total")])) == forwards * n, (lid, val[(lid, "histogram_row_total")])
        assert int(float(val[(lid, "histogram_top_bin_count")])) == 0 and 0 <= int(float(val[(lid, "histogram_median_bin")])) < 48
        assert 0 <= int(float(val[(lid, "abs_max_argmax_channel")])) < Cc and float(val[(lid, "abs_max_overall_max")]) > 0
    assert ("vae.encoder.down_blocks.0.resnets.0.norm1.output", "per_channel_overall_mean") in val
    assert ("vae.decoder.conv_norm_out.input", "scalar") in val
