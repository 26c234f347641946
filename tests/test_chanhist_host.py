"""log2_histogram_per_channel / abs_max_activation_per_channel / near_zero_fraction_per_channel on the host: the hook path's
formulas (tracking.monitor.compute_metrics) against known answers and against tests/chanhist_refs.py, step() and the exported
records of a plain torch module on the CPU, the routing of the new config, and the library's workspace query and argument
refusals.  Nothing here touches a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import chanhist_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_channel_hist.yaml")
HIST, AMAX, NZ = "log2_histogram_per_channel", "abs_max_activation_per_channel", "near_zero_fraction_per_channel"
THREE = [HIST, AMAX, NZ]
FUSED = "mean_abs_activation_per_channel"


def _metrics(t, tau=1e-3):
    from tracking.monitor import compute_metrics
    out = compute_metrics(t, THREE, tau)
    assert list(out) == THREE
    assert out[HIST].dtype == np.int64 and out[AMAX].dtype == np.float32 and out[NZ].dtype == np.float32
    return out


# ------------------------------------------------------------------------------------------------ formulas
def test_bin_edge_known_answers():
    vals = R.edge_values()
    want = np.array([b for _, b in R.EDGES])
    assert len(vals) == 19 and set(want) == {0, 1, 31, 46, 47}
    # every value in a channel of its own: (B, C, H, W) = (1, n, 1, 1) for the hook path, NHWC (1, 1, 1, n) for the reference
    out = _metrics(vals.reshape(1, -1, 1, 1))
    hist, nz, amax = R.ref_exact(vals.reshape(1, 1, 1, -1))
    for h in (out[HIST], hist):
        assert h.shape == (len(vals), 48) and (h.sum(axis=1) == 1).all()
        assert (h.argmax(axis=1) == want).all(), (h.argmax(axis=1), want)
    a = np.abs(vals.numpy())
    for got in (out[AMAX], amax):
        assert np.array_equal(got.view(np.uint32)[~np.isnan(a)], a.view(np.uint32)[~np.isnan(a)])
        assert np.isnan(got[np.isnan(a)]).all() and np.isnan(a).sum() == 1
    near = (a < np.float32(1e-3)).astype(np.float32)  # zero, the denormal, 2^-30 and its neighbour; not NaN
    assert near.sum() == 8
    assert np.array_equal(out[NZ], near) and np.array_equal(nz, near.astype(np.int64))
    # all of them in ONE channel: a NaN makes the maximum NaN and is not near zero
    one = _metrics(vals.reshape(1, 1, -1, 1))
    assert one[HIST].shape == (1, 48) and np.array_equal(one[HIST][0], np.bincount(want, minlength=48))
    assert np.isnan(one[AMAX][0]) and one[NZ][0] == np.float32(8 / 19)
    fin = _metrics(vals[:-1].reshape(1, 1, -1, 1))
    assert math.isinf(fin[AMAX][0]) and _metrics(vals[:16].reshape(1, 1, -1, 1))[AMAX][0] == np.float32(65536.0)


@pytest.mark.parametrize("tau", [1e-3, 0.25, 3e-7])
def test_tau_edge(tau):
    vals = R.tau_edge_values(tau)  # below, at, above, and their negatives
    want = np.array([1, 0, 0, 1, 0, 0], dtype=np.float32)
    assert np.array_equal(_metrics(vals.reshape(1, -1, 1, 1), tau)[NZ], want)
    assert np.array_equal(R.ref_exact(vals.reshape(1, 1, 1, -1), tau)[1], want.astype(np.int64))
    assert _metrics(vals.reshape(1, 1, 2, 3), tau)[NZ][0] == np.float32(2 / 6)


def test_rows_sum_and_the_hook_formulas_match_the_reference():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 9, 5, 7), generator=g) * torch.logspace(-9, 5, 9).reshape(1, 9, 1, 1)  # NCHW, magnitudes over 14 decades
    x[0, 2] = 0.0   # a dead channel (one image of it)
    x[:, 4] = 3.0   # a constant channel
    out = _metrics(x)
    hist, nz, amax = R.ref_exact(x.permute(0, 2, 3, 1))
    assert (out[HIST].sum(axis=1) == 2 * 5 * 7).all()
    assert np.array_equal(out[HIST], hist) and np.array_equal(out[AMAX], amax)
    assert np.array_equal(out[NZ], (nz / 70.0).astype(np.float32))
    assert out[HIST][4, 32] == 70 and out[AMAX][4] == 3.0 and out[NZ][4] == 0.0 and out[HIST][2, 0] >= 35
    bf = _metrics(x.to(torch.bfloat16))  # a bf16 tensor is widened, not refused
    assert np.array_equal(bf[HIST], R.ref_exact(x.to(torch.bfloat16).permute(0, 2, 3, 1))[0])
    # [N, C] activations (a Linear's output) and a tensor without a channel axis
    assert _metrics(x[:, :, 0, 0])[HIST].shape == (9, 48) and _metrics(x[0, 0, 0])[HIST].shape == (1, 48)


def test_real_bins_agree_with_the_exponent_field():
    """the float64 binning the transformed-input bounds use is the bit-pattern binning on every fp32 number"""
    g = torch.Generator().manual_seed(5)
    v = (torch.randn(20000, generator=g) * torch.pow(2.0, torch.randint(-40, 24, (20000,), generator=g).float())).numpy()
    v = np.concatenate([v, np.array([x for x, _ in R.EDGES], dtype=np.float32)])
    assert np.array_equal(R.real_bin(np.abs(v.astype(np.float64))), R.bits_bin(v))
    # an element well inside a bin is certain, one within its radius of an edge is not
    y = np.array([[1.5, 2.0 - 1e-9, 1e-3 + 1e-12, -0.75]])
    bd = R.count_bounds(y, np.full_like(y, 1e-7), 1e-3)
    assert bd["uncertain"] == 2 and bd["hist_lo"].sum() == 3 and bd["hist_unc"][1, 31] == bd["hist_unc"][1, 32] == 1
    assert list(bd["nz_lo"]) == [0, 0, 0, 0] and list(bd["nz_unc"]) == [0, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ monitor, hook path
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 5, 1)
        self.act = torch.nn.ReLU()

    def forward(self, x):
        return self.act(self.conv(x))


def test_hook_path_end_to_end_on_a_plain_module():
    from tracking.monitor import ActivityMonitor, compute_metrics
    torch.manual_seed(0)
    net = _Net()
    tau = 0.05
    cfg = {"enabled": True, "track_interval": 1, "near_zero_threshold": tau, "device_metrics": True,  # no engine: hooks anyway
           "target_layers": [{"name": "act", "capture_point": "output", "metrics": THREE + [FUSED, "no_such_metric"]},
                             {"name": "conv", "capture_point": "input", "metrics": [NZ]}]}
    mon = ActivityMonitor(net, cfg)
    assert mon.device_layers == [] and mon.fused_layers == [] and len(mon.hooks) == 2
    xs = [torch.randn(2, 3, 4, 6), torch.randn(2, 3, 4, 6) * 40.0]
    xs[1][0, 0, 0, 0] = 1e6
    per = []
    with torch.no_grad():
        for x in xs:
            per.append(compute_metrics(net(x), THREE, tau))
    assert set(mon.hook_collected_buffer["act.output"]) == set(THREE + [FUSED])  # the unknown name is warned about, as before
    log = mon.step(1)
    data = mon.get_data_for_step(1)
    got = data["act.output"]
    assert list(got) == THREE + [FUSED]
    n = 2 * 4 * 6
    assert np.array_equal(got[HIST], per[0][HIST] + per[1][HIST]) and (got[HIST].sum(axis=1) == 2 * n).all()
    assert got[HIST].dtype == np.int64
    assert np.array_equal(got[AMAX], np.maximum(per[0][AMAX], per[1][AMAX]))
    assert np.array_equal(got[NZ], np.mean(np.stack([per[0][NZ], per[1][NZ]]), axis=0)) and got[NZ].max() >= 0.25  # ReLU zeros
    tin = compute_metrics(xs[0], [NZ], tau)[NZ], compute_metrics(xs[1], [NZ], tau)[NZ]
    assert np.array_equal(data["conv.input"][NZ], (tin[0] + tin[1]) / 2)
    base = "tracking/act.output/"
    assert set(log) == {base + HIST + "_top_bin_share", base + AMAX + "_overall_max", base + NZ + "_overall_mean",
                        base + NZ + "_overall_max", base + FUSED + "_overall_mean", base + FUSED + "_overall_std",
                        "tracking/conv.input/" + NZ + "_overall_mean", "tracking/conv.input/" + NZ + "_overall_max"}
    assert log[base + HIST + "_top_bin_share"] == float(got[HIST][:, 47].sum()) / (5 * 2 * n)
    assert log[base + AMAX + "_overall_max"] == got[AMAX].max() and log[base + NZ + "_overall_max"] == got[NZ].max()
    recs = [r for r in mon.export_all_processed_data_to_records() if r["layer_identifier"] == "act.output"]
    kinds = {(r["original_metric_name"], r["metric_type"]): r["metric_value"] for r in recs}
    assert kinds.pop((HIST, "histogram_row_total")) == 2 * n
    assert set(kinds) == {(HIST, "histogram_shape"), (HIST, "histogram_top_bin_count"), (HIST, "histogram_zero_bin_count"),
                          (HIST, "histogram_median_bin"), (AMAX, "abs_max_overall_max"), (AMAX, "abs_max_overall_mean"),
                          (AMAX, "abs_max_argmax_channel"), (NZ, "near_zero_overall_mean"), (NZ, "near_zero_overall_max"),
                          (NZ, "near_zero_dead_channels"), (FUSED, "per_channel_overall_mean"), (FUSED, "per_channel_overall_std"),
                          (FUSED, "per_channel_overall_min"), (FUSED, "per_channel_overall_max")}
    assert kinds[(HIST, "histogram_shape")] == "(5, 48)"
    assert kinds[(HIST, "histogram_zero_bin_count")] == int(got[HIST][:, 0].sum()) > 0
    assert kinds[(HIST, "histogram_top_bin_count")] == int(got[HIST][:, 47].sum())
    total = got[HIST].sum(axis=0)
    med = kinds[(HIST, "histogram_median_bin")]
    assert total[:med].sum() < (total.sum() + 1) // 2 <= total[:med + 1].sum()
    assert kinds[(AMAX, "abs_max_argmax_channel")] == int(got[AMAX].argmax())
    assert kinds[(NZ, "near_zero_dead_channels")] == int((got[NZ] >= 0.99).sum())
    mon.remove_hooks()


def test_old_metrics_and_unknown_names_behave_as_before():
    from tracking.monitor import KNOWN_METRICS, ActivityMonitor, compute_metrics
    assert KNOWN_METRICS[:4] == (FUSED, "full_activation_map", "mean_activation", "std_activation")
    assert set(KNOWN_METRICS[4:]) == set(THREE)
    x = torch.randn(2, 3, 4, 4)
    assert compute_metrics(x, ["no_such_metric"]) == {}
    old = compute_metrics(x, list(KNOWN_METRICS[:4]))
    assert list(old) == list(KNOWN_METRICS[:4]) and np.array_equal(old[FUSED], x.abs().mean(dim=(0, 2, 3)).numpy())
    net = _Net()
    mon = ActivityMonitor(net, {"enabled": True, "track_interval": 1,
                                "target_layers": [{"name": "act", "metrics": [FUSED, "mean_activation", "std_activation"]}]})
    with torch.no_grad():
        net(x)
    log = mon.step(1)
    base = "tracking/act.output/"
    assert set(log) == {base + FUSED + "_overall_mean", base + FUSED + "_overall_std", base + "mean_activation", base + "std_activation"}
    assert [r["metric_type"] for r in mon.export_all_processed_data_to_records()] == \
        ["per_channel_overall_mean", "per_channel_overall_std", "per_channel_overall_min", "per_channel_overall_max", "scalar", "scalar"]
    mon.remove_hooks()


# ------------------------------------------------------------------------------------------------ routing
def test_new_config_parses_and_routes_to_the_engine():
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from utils.config_utils import load_config
    from vaehip.engine import CHANHIST_METRICS, DEVICE_METRICS, MOMENT_METRICS
    assert set(CHANHIST_METRICS) == set(THREE) and set(THREE) <= set(DEVICE_METRICS) and not set(THREE) & set(MOMENT_METRICS)
    c = load_config(CFG)
    t = c["tracking"]
    assert t["device_metrics"] is True and float(t["near_zero_threshold"]) == 1e-3
    want = ["vae.encoder.down_blocks.0.resnets.0.norm1.output", "vae.encoder.down_blocks.0.resnets.0.conv1.input",
            "vae.encoder.down_blocks.0.resnets.0.output", "vae.encoder.input"]
    named = [f"{e['name']}.{e['capture_point']}" for e in t["target_layers"] if set(THREE) <= set(e["metrics"])]
    assert named == want
    w = SDXLVAEWrapper("synthetic:1")
    mon = ActivityMonitor(w, t)
    try:
        assert mon.near_zero_threshold == 1e-3
        assert mon.device_layers == want + ["vae.decoder.conv_norm_out.input"]
        assert sorted(n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks) == []
        eng = w.vae.engine
        tr = eng._mtrackers[id(w.vae.encoder)]["input"][0]
        assert tr.chanhist and not tr.moments and not tr.full_map and tr.tau == 1e-3
        both = eng._mtrackers[id(w.vae.encoder.down_blocks[0].resnets[0].norm1)]["output"][0]
        assert both.chanhist and both.moments
    finally:
        mon.remove_hooks()
    mon = ActivityMonitor(w, dict(t, device_metrics=False))  # the same targets on torch hooks
    try:
        assert mon.device_layers == [] and len(mon.fused_layers) == 3
    finally:
        mon.remove_hooks()


def test_wrapper_refuses_before_the_library_is_asked():
    from vaehip import ops
    assert ops.CHANHIST_BINS == 48
    with pytest.raises(ValueError, match="CUDA tensor"):  # CPU tensors: no fallback
        ops.chanhist(torch.zeros(1, 4, 4, 8))


# ------------------------------------------------------------------------------------------------ library, no GPU
def test_workspace_query_and_refusals_need_no_gpu():
    from vaehip.lib import lib, VaeHipError
    assert lib.query("vae_chanhist_bins") == 48
    n = C.c_int64(0)
    lib.call("vae_chanhist_workspace", 3, 16 * 16, 128, 4, C.byref(n))
    assert n.value == 3 * 4 * 128 * 50  # per (image, chunk, channel): 48 bins, the near-zero count, the largest |y| pattern
    lib.call("vae_chanhist_workspace", 1, 1, 1, 1, C.byref(n))
    assert n.value == 50
    with pytest.raises(VaeHipError, match="chanhist_workspace: bad args"):
        lib.call("vae_chanhist_workspace", 0, 16, 8, 1, C.byref(n))
    with pytest.raises(VaeHipError, match="null args"):
        lib.call("vae_chanhist_workspace", 1, 16, 8, 1, None)
    with pytest.raises(VaeHipError, match="empty chunk"):
        lib.call("vae_chanhist_workspace", 1, 10, 8, 7, C.byref(n))  # chunks of 2 pixels: the last two of 7 are empty
    with pytest.raises(VaeHipError, match="2\\^31"):
        lib.call("vae_chanhist_workspace", 32768, 65536, 8, 1, C.byref(n))
    lib.call("vae_chanhist_workspace", 32767, 65536, 8, 1, C.byref(n))
    assert n.value == 32767 * 8 * 50
    # the launch entry points refuse on the host, before any launch (the pointers are never followed)
    p, nan = C.c_void_p(4096), float("nan")

    def partial(x=p, sc=None, sh=None, xf=0, B=2, HW=64, Cc=8, ld=8, nch=2, tau=1e-3, ws=p):
        lib.call("vae_chanhist_partial", x, 0, sc, sh, xf, B, HW, Cc, ld, nch, tau, ws, None)

    for kw, msg in [(dict(x=None), "null args"), (dict(ws=None), "null args"), (dict(ld=7), "pixel stride ld=7 below C=8"),
                    (dict(nch=33, HW=64), "empty chunk"), (dict(xf=1), "xf needs scale and shift"),
                    (dict(xf=2, sc=p), "xf needs scale and shift"), (dict(xf=3, sc=p, sh=p), "xf=3"),
                    (dict(ws=C.c_void_p(4096 + 8)), "unaligned workspace"), (dict(tau=-1e-3), "negative or NaN"),
                    (dict(tau=nan), "negative or NaN"), (dict(B=32768, HW=65536), "2\\^31"), (dict(Cc=0), "bad args")]:
        with pytest.raises(VaeHipError, match="chanhist_partial.*" + msg):
            partial(**kw)
    i64 = C.c_void_p(8192)
    for args, msg in [((None, 2, 64, 8, 2, i64, i64, i64), "null args"), ((p, 2, 64, 8, 2, None, i64, i64), "null args"),
                      ((p, 2, 64, 8, 2, i64, None, i64), "null args"), ((p, 2, 64, 8, 2, i64, i64, None), "null args"),
                      ((C.c_void_p(4100), 2, 64, 8, 2, i64, i64, i64), "unaligned workspace"),
                      ((p, 2, 64, 8, 33, i64, i64, i64), "empty chunk"), ((p, 32768, 65536, 8, 1, i64, i64, i64), "2\\^31")]:
        with pytest.raises(VaeHipError, match="chanhist_final.*" + msg):
            lib.call("vae_chanhist_final", *args, None)
