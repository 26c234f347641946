"""ops.chancov (csrc/chancov.hip): channel covariance and mean of y = XF(x) in one read, split-bf16 products of the values
centred on the tensor's first pixel row.

Every element of the device covariance is held to the float64 reference of tests/chancov_refs.py:
|cov_dev - cov_64| (N - 1) <= BAR sqrt(S_c S_c') with S_c = sum (y_c - K_c)^2 and BAR = conv_routes.BAR_WGRAD (3e-5), the mean
to 1e-6 (|mean| + sqrt(S_c / N)).  Then the exact properties (zeros of constant channels, bitwise symmetry and repeatability,
refusals before any launch), guarded memory, the engine (hook path against device path on the small synthetic VAE) and
src/train.py on the new config."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chancov_refs as R
from guarded import GuardedPool, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV, RHO, MAXR, RANK = ("channel_covariance_matrix", "channel_correlation_matrix", "max_abs_correlation_per_channel",
                        "effective_rank")
FOUR = [COV, RHO, MAXR, RANK]
T = 128  # vae_chancov_tile(), asserted below
CHANNELS = (1, 3, 4, 8, T - 1, T, T + 1, 2 * T + 1, 512)
# two rows; one k-group with a tail; chunks not dividing HW; several chunks per image; a whole tile of pixels
SHAPES = [(1, 1, 2), (1, 7, 13), (3, 7, 13), (3, 16, 16), (1, 32, 24)]
DTYPES = [torch.float32, torch.bfloat16]
WORST = {}


def _stats(B, ld, dev, seed):
    from vaehip.ops import Stats
    sc, sh = R.stats_rows(B, ld, seed)
    return Stats(None, None, sc.to(dev), sh.to(dev))


def _x(shape, seed):
    """the moments suite's generator, with a mean and a scale of its own per channel"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    Cc = shape[-1]
    return (torch.randn(shape, generator=g) * 1.3 + 0.4) * (torch.rand((Cc,), generator=g) + 0.5) + torch.randn((Cc,), generator=g)


def _check(got, x, st=None, xf=0, group=None):
    e, m = R.check(got, x, st.scale if st is not None else None, st.shift if st is not None else None, xf)
    if group:
        w = WORST.setdefault(group, [0.0, 0.0])
        w[0], w[1] = max(w[0], e), max(w[1], m)


def test_tile_is_the_one_the_sweep_sits_on(cuda):
    from vaehip.lib import lib
    assert lib.query("vae_chancov_tile") == T


# ---------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("xf", [0, 1, 2])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_against_float64(cuda, Cc, dt, xf, B, H, W):
    """The first two pixels of image 0 -- all there is in the two-row shape -- are placed where the transform's argument
    u = x scale + shift is 0.5 and 2.5 in every channel (y = 0.31 and 2.31 behind SiLU).  The criterion's reference evaluates XF
    in float64, the device in fp32 (about 2e-7 |y| per value, chanhist_refs.ref_transformed); on the scale sqrt(S_c S_c') that
    is invisible unless a channel's rows nearly coincide, which two random rows of some channel out of hundreds do: with
    random rows the case C = 128, fp32, GroupNorm + SiLU measured 3.3e-4 (a channel whose two y agree to 3e-4 of their size;
    8e-6 and 4e-6 at C = 127 and behind the affine alone), all of it the fp32 evaluation of y and none of it the Gram product:
    untransformed two-row cases measure 2e-7.  No fp32 evaluation of y can do better there, so the two rows are kept apart."""
    from vaehip import ops
    x = _x((B, H, W, Cc), Cc * 131 + B * 7 + H + xf)
    st = _stats(B, Cc, cuda, Cc + xf) if xf else None
    for pix, u in ((0, 0.5), (1, 2.5)):
        x[0, 0, pix] = (u - st.shift[0].cpu()) / st.scale[0].cpu() if xf else u
    x = x.to(cuda).to(dt)
    _check(ops.chancov(x, st, xf), x, st, xf, group=f"{str(dt)[6:]}_xf{xf}")


def test_worst_of_the_sweep(cuda):
    for k, (e, m) in sorted(WORST.items()):
        print(f"chancov sweep {k}: worst cov error {e:.3e} (bar {R.BAR:.0e}), worst mean error {m:.3e} (bar {R.MEAN_TOL:.0e})")
    assert all(e <= R.BAR and m <= R.MEAN_TOL for e, m in WORST.values())


@pytest.mark.parametrize("xf", [0, 1, 2])
@pytest.mark.parametrize("dt", DTYPES)
def test_channel_prefix_view(cuda, dt, xf):
    """the encoder's input: the 3-channel view x4[..., :3] of a 4-channel buffer, read in place; the pad channel must not leak"""
    from vaehip import ops
    x4 = _x((3, 7, 13, 4), 5).to(cuda).to(dt)
    x4[..., 3] = 1e6
    x = x4[..., :3]
    st = _stats(3, 4, cuda, 9) if xf else None
    got = ops.chancov(x, st, xf)
    assert got[0].shape == (3, 3) and float(got[0].abs().max()) < 1e3 and float(got[1].abs().max()) < 1e3
    _check(got, x, st, xf)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cc,B,H,W", [(T, 3, 16, 16), (4, 2, 16, 24), (3, 1, 7, 13), (2 * T + 1, 1, 7, 13)])
def test_constant_and_zero_channels_are_exactly_zero(cuda, Cc, B, H, W, dt):
    from vaehip import ops
    x = _x((B, H, W, Cc), 11 + Cc)
    x[..., 0] = 3.0
    x[..., Cc - 1] = 0.0
    x = x.to(cuda).to(dt)
    got = ops.chancov(x)
    _check(got, x)
    cov, mean = (t.cpu().numpy() for t in got)
    for c in (0, Cc - 1):
        assert (cov[c, :] == 0.0).all() and (cov[:, c] == 0.0).all()
    assert mean[0] == 3.0 and mean[Cc - 1] == 0.0
    assert (np.diag(cov)[1:Cc - 1] > 0).all()


@pytest.mark.parametrize("Cc,B,H,W", [(8, 3, 16, 16), (T + 1, 1, 32, 24)])
def test_means_a_thousand_sigma_away(cuda, Cc, B, H, W):
    """every channel's mean is 1000 sigma: values 1024 s + k s / 1024 with integer |k| of a few thousand are exact in fp32, and so
    is their difference from the first pixel row; unshifted, the split products lose the variance (3.7e-2 in the emulation)"""
    from vaehip import ops
    g = torch.Generator(device="cpu").manual_seed(Cc)
    k = torch.round(torch.randn((B, H, W, Cc), generator=g) * 1024.0)
    s = torch.pow(2.0, torch.randint(-3, 4, (Cc,), generator=g).float())
    sign = torch.where(torch.rand((Cc,), generator=g) < 0.5, -1.0, 1.0)
    x = ((1024.0 + k / 1024.0) * s * sign).to(cuda)
    assert torch.equal(x.double().cpu(), ((1024.0 + k.double() / 1024.0) * s.double() * sign.double()))
    sd, mu = x.double().std(dim=(0, 1, 2)), x.double().mean(dim=(0, 1, 2))
    assert bool((mu.abs() > 900 * sd).all())
    _check(ops.chancov(x), x)


# ---------------------------------------------------------------------------------------------------- exactness
def test_repeatable_and_symmetric(cuda):
    from vaehip import ops
    torch.manual_seed(6)
    for dt, xf, shape in ((torch.float32, 0, (3, 40, 56, 256)), (torch.bfloat16, 2, (3, 40, 56, 256)), (torch.float32, 0, (2, 9, 11, 3))):
        x = torch.randn(shape, device=cuda).to(dt)
        st = _stats(shape[0], shape[3], cuda, 1) if xf else None
        a = ops.chancov(x, st, xf)
        b = ops.chancov(x, st, xf)
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int64), v.view(torch.int64))
        assert torch.equal(a[0].view(torch.int64), a[0].t().contiguous().view(torch.int64))


def test_argument_errors_are_refused_before_any_launch(cuda):
    import ctypes
    from vaehip import ops
    from vaehip.lib import lib, VaeHipError
    B, H, W, Cc, nch = 2, 8, 8, 8, 2
    x = torch.randn((B, H, W, Cc), device=cuda)
    one = torch.ones((B, Cc), device=cuda)
    n = ctypes.c_int64(0)
    lib.call("vae_chancov_workspace", B, H * W, Cc, nch, ctypes.byref(n))
    ws = torch.full((n.value + 4,), -1.0, device=cuda)
    cov = torch.full((Cc, Cc), -1.0, device=cuda, dtype=torch.float64)
    mean = torch.full((Cc,), -1.0, device=cuda, dtype=torch.float64)
    p = ops._p

    def partial(xp=p(x), sc=None, sh=None, xf=0, B=B, HW=H * W, Cc=Cc, ld=Cc, nch=nch, wsp=p(ws)):
        lib.call("vae_chancov_partial", xp, 0, sc, sh, xf, B, HW, Cc, ld, nch, wsp, ops._stream())

    for kw, msg in [(dict(xp=None), "null args"), (dict(wsp=None), "null args"), (dict(ld=Cc - 1), "pixel stride"),
                    (dict(nch=H * W // 2 + 1), "empty chunk"), (dict(xf=1), "xf needs scale and shift"),
                    (dict(xf=2, sh=p(one)), "xf needs scale and shift"), (dict(wsp=ws.data_ptr() + 4), "unaligned workspace"),
                    (dict(B=1, HW=1, nch=1), "two rows"), (dict(B=32768, HW=65536), "2\\^31")]:
        with pytest.raises(VaeHipError, match="chancov_partial.*" + msg):
            partial(**kw)
    with pytest.raises(VaeHipError, match="chancov_final.*null args"):
        lib.call("vae_chancov_final", p(ws), B, H * W, Cc, nch, p(cov), None, ops._stream())
    with pytest.raises(VaeHipError, match="chancov_final.*unaligned workspace"):
        lib.call("vae_chancov_final", ws.data_ptr() + 4, B, H * W, Cc, nch, p(cov), p(mean), ops._stream())
    with pytest.raises(VaeHipError, match="chancov_final.*two rows"):
        lib.call("vae_chancov_final", p(ws), 1, 1, Cc, 1, p(cov), p(mean), ops._stream())
    torch.cuda.synchronize()
    # nothing was launched by any of them
    assert bool((ws == -1).all()) and bool((cov == -1).all()) and bool((mean == -1).all())
    with pytest.raises(ValueError, match="needs its stats"):
        ops.chancov(x, None, 2)
    with pytest.raises(ValueError, match="contiguous channels"):
        ops.chancov(x.permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match="two rows"):
        ops.chancov(torch.randn((1, 1, 1, 8), device=cuda))
    # and the same arguments, valid, run; the partial pass writes exactly the words the size query names
    partial()
    lib.call("vae_chancov_final", p(ws), B, H * W, Cc, nch, p(cov), p(mean), ops._stream())
    assert bool((ws[n.value:] == -1).all())
    _check((cov, mean), x)


@pytest.mark.parametrize("case", ["c1_2rows_f32", "c512_f32_affine", "c512_bf16_silu", "view3of4_f32", "view3of4_bf16_silu", "c257_f32"])
def test_guarded_memory(cuda, case):
    """the sweep's smallest and largest cases (and the prefix view, and a tile edge) with operands, workspace and results in
    guarded, poisoned blocks: no store outside a block, no unwritten result or workspace word, no operand changed, and the
    values are still right (a load outside an operand would have met NaN)"""
    from vaehip import ops
    from vaehip.ops import Stats
    pool = GuardedPool(cuda)
    if case == "c1_2rows_f32":
        x, st, xf = pool.put(_x((1, 1, 2, 1), 71), "x"), None, 0
    elif case.startswith("view3of4"):
        dt = torch.bfloat16 if "bf16" in case else torch.float32
        x4 = _x((2, 12, 20, 4), 70).to(dt)
        x4[..., 3] = 1e6
        x = pool.put(x4, "x4")[..., :3]
        xf = 2 if "silu" in case else 0
        st = Stats(None, None, *(pool.put(t, n) for t, n in zip(R.stats_rows(2, 4, 3), ("scale", "shift")))) if xf else None
    elif case == "c257_f32":
        x, st, xf = pool.put(_x((2, 12, 20, 257), 72), "x"), None, 0
    else:
        dt = torch.bfloat16 if "bf16" in case else torch.float32
        x = pool.put(_x((1, 32, 24, 512), 73).to(dt), "x")
        xf = 2 if "silu" in case else 1
        st = Stats(None, None, *(pool.put(t, n) for t, n in zip(R.stats_rows(1, 512, 4), ("scale", "shift"))))
    pool.snapshot()
    with guarded(pool, ops):
        got = ops.chancov(x, st, xf)
    torch.cuda.synchronize()
    assert len(pool.blocks) >= 4  # the operands, the workspace and two results
    assert pool.violations() == [] and pool.changed() == []
    assert pool.unwritten_report() == []
    for t in got:
        pool.block_of(t)  # the results are pool tensors
    _check(got, x, st, xf)


# ---------------------------------------------------------------------------------------------------- engine
POINTS = [("vae.encoder.down_blocks.0.resnets.0.norm1", "output"),   # GroupNorm affine, fused: no tensor exists
          ("vae.encoder.down_blocks.0.resnets.0.conv1", "input"),    # ... + SiLU
          ("vae.encoder.down_blocks.0.resnets.0", "output"),
          ("vae.encoder", "input")]
KEY_OF = {(1, 128): "vae.encoder.down_blocks.0.resnets.0.norm1.output", (2, 128): "vae.encoder.down_blocks.0.resnets.0.conv1.input",
          (0, 128): "vae.encoder.down_blocks.0.resnets.0.output", (0, 3): "vae.encoder.input"}
THR = 0.9


def _run(cuda, device_metrics, mixed_precision, record=None):
    """steps 1 and 2 of a small run; step 2 buffers two forwards (a train step and an eval step)"""
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from vaehip import ops
    from vaehip.trainer import HipTrainer
    cfg = {"enabled": True, "track_interval": 1, "device_metrics": device_metrics, "redundancy_threshold": THR,
           "target_layers": [{"name": n, "capture_point": p, "metrics": list(FOUR)} for n, p in POINTS]}
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), 7))
    w.to(cuda)
    tr = HipTrainer(w, lr=1e-4, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mixed_precision)
    mon = ActivityMonitor(w, cfg)
    real = ops.chancov
    calls = []
    if record is not None:
        def spy(x, stats=None, xf=0):
            out = real(x, stats, xf)
            calls.append((x.clone(), stats, xf, out))
            return out
        ops.chancov = spy
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
        ops.chancov = real
    torch.cuda.synchronize()
    recs = mon.export_all_processed_data_to_records()
    hooked = [n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks]
    layers = list(mon.device_layers)
    mon.remove_hooks()
    return logs, data, recs, hooked, layers


def _summary_bounds(cov, E):
    """what an elementwise covariance error of at most E can do to correlation_summary(cov), rigorously: with a_c = E_cc / v_c
    and m = sqrt((1 - a_c)(1 - a_c')), |rho' - rho| <= E_cc' / (sqrt(v_c v_c') m) + |rho| (1 / m - 1); the per-channel maximum
    moves by at most the largest such bound of its row; tr and ||.||_F^2 move by at most sum E_cc and 2 sum |cov| E + sum E^2,
    which brackets the participation ratio.  fp32 storage adds 2^-24 of the value."""
    from tracking.monitor import correlation_summary
    s = correlation_summary(cov, THR)
    v = np.diag(cov)
    a = np.diag(E) / v
    assert (v > 0).all() and a.max() < 0.5
    m = np.sqrt(np.outer(1 - a, 1 - a))
    drho = E / (np.sqrt(np.outer(v, v)) * m) + np.abs(s["correlation"]) * (1 / m - 1) + 2.0 ** -24
    np.fill_diagonal(drho, 0.0)
    dmax = drho.max(axis=1) + 2.0 ** -24
    tr, f2 = np.trace(cov), (cov * cov).sum()
    dtr, df2 = np.trace(E), 2 * (np.abs(cov) * E).sum() + (E * E).sum()
    rank = ((tr - dtr) ** 2 / (f2 + df2), (tr + dtr) ** 2 / (f2 - df2))
    return s, drho, dmax, rank


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_hook_path_against_device_path(cuda, mode):
    """both paths against the float64 covariance of the values the device pass read, averaged over the step's forwards: the
    covariance within the bar, the three derived metrics within the bar propagated through correlation_summary"""
    record = {}
    ld, dd, rd, hooked, layers = _run(cuda, True, mode, record)
    assert hooked == [] and sorted(layers) == sorted(KEY_OF.values())
    lh, dh, rh, hooked_h, layers_h = _run(cuda, False, mode)
    assert layers_h == [] and len(hooked_h) == 4
    for s, forwards in ((1, 1), (2, 2)):
        assert set(ld[s]) == set(lh[s]) and len(ld[s]) == 4 * 3  # step() returns the same keys from both paths
        assert list(dd[s]) == list(dh[s])
        calls = record[s]
        assert len(calls) == 4 * forwards  # one pass per capture point and forward
        agg = {}
        for x, st, xf, out in calls:
            lid = KEY_OF[(xf, x.shape[-1])]
            assert tuple(x.shape[:3]) == (2, 32, 32)
            _check(out, x, st, xf)  # every pass against its own reference
            r = R.ref(x, st.scale if st is not None else None, st.shift if st is not None else None, xf)
            a = agg.setdefault(lid, {"cov": 0.0, "E": 0.0})
            a["cov"] = a["cov"] + r["cov"] / forwards
            a["E"] = a["E"] + R.BAR * np.sqrt(np.outer(r["S"], r["S"])) / (r["n"] - 1) / forwards
        for lid in dd[s]:
            want, E = agg[lid]["cov"], agg[lid]["E"]
            summ, drho, dmax, rank = _summary_bounds(want, E)
            for path, got in (("device", dd[s][lid]), ("hook", dh[s][lid])):
                assert list(got) == FOUR
                assert got[COV].dtype == np.float64 and got[RHO].dtype == np.float32 and got[MAXR].dtype == np.float32
                e_cov = float((np.abs(got[COV] - want) / E).max())
                e_rho = float((np.abs(got[RHO] - summ["correlation"]) / np.where(drho > 0, drho, 1.0)).max())
                e_max = float((np.abs(got[MAXR] - summ["max_abs"]) / dmax).max())
                print(f"{mode} step {s} {lid} {path}: cov {e_cov:.3f}, rho {e_rho:.3f}, max|rho| {e_max:.3f} of the bound; "
                      f"rank {got[RANK]:.6f} in [{rank[0]:.6f}, {rank[1]:.6f}]")
                assert e_cov <= 1.0 and e_rho <= 1.0 and e_max <= 1.0
                assert np.array_equal(np.diag(got[RHO]), np.ones(len(want), dtype=np.float32))
                assert rank[0] <= got[RANK] <= rank[1]
    kinds = lambda recs: [(r["global_step"], r["layer_identifier"], r["original_metric_name"], r["metric_type"]) for r in recs]  # noqa: E731
    assert kinds(rd) == kinds(rh) and len(rd) == 2 * 4 * 12


def test_engine_shares_one_pass_among_the_trackers_of_a_point(cuda):
    """two registrations at one point share a pass; a sink that asked for no covariance is called without the keyword"""
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip import ops
    w = SDXLVAEWrapper("synthetic:1")
    w.to(cuda)
    eng = w.vae.engine
    norm1 = w.vae.encoder.down_blocks[0].resnets[0].norm1
    seen = {"a": [], "b": [], "old": []}
    hs = [eng.add_tracker(norm1, "output", lambda m, f, chancov=None: seen["a"].append((m, f, chancov)), metrics=[RANK]),
          eng.add_tracker(norm1, "output", lambda m, f, chancov=None, chanhist=None: seen["b"].append((m, f, chancov, chanhist)),
                          metrics=[COV, "mean_activation", "abs_max_activation_per_channel"]),
          eng.add_tracker(norm1, "output", lambda m, f: seen["old"].append((m, f)), metrics=["std_activation"])]
    real, n = ops.chancov, []
    ops.chancov = lambda *a, **k: (n.append(1), real(*a, **k))[1]
    try:
        with torch.no_grad():
            w.vae.encode(vo.synthetic_pixels(1, 32, 1, 1).to(cuda))
    finally:
        ops.chancov = real
        for h in hs:
            h.remove()
    assert len(n) == 1 and len(seen["a"]) == len(seen["b"]) == len(seen["old"]) == 1
    assert seen["a"][0][2] is seen["b"][0][2] and seen["a"][0][0] is None and seen["b"][0][0] is seen["old"][0][0]
    assert seen["b"][0][3] is not None
    cov, mean = seen["a"][0][2]
    assert cov.shape == (128, 128) and mean.shape == (128,) and cov.dtype == torch.float64


# ---------------------------------------------------------------------------------------------------- CLI
def test_train_cli_with_the_channel_corr_config(cuda, tmp_path):
    """src/train.py with configs/experiment_synthetic_channel_corr.yaml: the CSV carries the new record kinds"""
    import yaml
    src = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
    c = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_channel_corr.yaml")))
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
    val = {(row["layer_identifier"], row["original_metric_name"], row["metric_type"]): row["metric_value"] for row in rows}
    for lid, Cc in (("vae.encoder.down_blocks.0.resnets.0.norm1.output", 128), ("vae.encoder.down_blocks.0.resnets.0.conv1.input", 128),
                    ("vae.encoder.down_blocks.0.resnets.0.output", 128), ("vae.encoder.input", 3)):
        for m, k in [(COV, "covariance_shape"), (COV, "covariance_mean_abs_offdiag"), (COV, "covariance_max_abs_offdiag"),
                     (COV, "covariance_redundant_pairs"), (RHO, "correlation_shape"), (RHO, "correlation_mean_abs_offdiag"),
                     (RHO, "correlation_max_abs_offdiag"), (RHO, "correlation_redundant_pairs"),
                     (MAXR, "max_abs_correlation_overall_mean"), (MAXR, "max_abs_correlation_overall_max"),
                     (MAXR, "max_abs_correlation_redundant_channels"), (RANK, "scalar")]:
            assert (lid, m, k) in val, (lid, m, k)
        assert val[(lid, COV, "covariance_shape")] == val[(lid, RHO, "correlation_shape")] == f"({Cc}, {Cc})"
        assert 1.0 <= float(val[(lid, RANK, "scalar")]) <= Cc
        assert 0.0 < float(val[(lid, RHO, "correlation_max_abs_offdiag")]) <= 1.0 + 1e-6
        assert float(val[(lid, MAXR, "max_abs_correlation_overall_max")]) == pytest.approx(
            float(val[(lid, RHO, "correlation_max_abs_offdiag")]), abs=1e-6)
        assert int(float(val[(lid, COV, "covariance_redundant_pairs")])) == int(float(val[(lid, RHO, "correlation_redundant_pairs")]))
    assert ("vae.encoder.down_blocks.0.resnets.0.norm1.output", "mean_abs_activation_per_channel", "per_channel_overall_mean") in val
    assert ("vae.decoder.conv_norm_out.input", "mean_activation", "scalar") in val
