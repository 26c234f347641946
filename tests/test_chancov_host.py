"""channel_covariance_matrix / channel_correlation_matrix / max_abs_correlation_per_channel / effective_rank on the host:
tracking.monitor.correlation_summary against numpy, the hook path (compute_metrics, step(), log keys, exported records) on a
plain torch module on the CPU, the routing of the new config, and the library's tile and workspace queries and argument
refusals.  Nothing here touches a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import chancov_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_channel_corr.yaml")
COV, RHO, MAXR, RANK = ("channel_covariance_matrix", "channel_correlation_matrix", "max_abs_correlation_per_channel",
                        "effective_rank")
FOUR = [COV, RHO, MAXR, RANK]
FUSED = "mean_abs_activation_per_channel"


def _data(n, Cc, seed):
    g = np.random.default_rng(seed)
    mix = g.standard_normal((Cc, Cc)) * 0.5 + np.eye(Cc)
    return g.standard_normal((n, Cc)) @ mix + g.standard_normal(Cc) * 3.0


# ------------------------------------------------------------------------------------------------ correlation_summary
@pytest.mark.parametrize("Cc", [2, 5, 33])
def test_summary_against_numpy(Cc):
    from tracking.monitor import correlation_summary
    y = _data(400, Cc, Cc)
    cov = np.cov(y, rowvar=False).reshape(Cc, Cc)
    s = correlation_summary(cov, 0.3)
    want = R.summary_ref(cov, 0.3)
    assert np.allclose(s["correlation"], np.corrcoef(y, rowvar=False), rtol=0, atol=1e-12)
    assert np.allclose(s["correlation"], want["rho"], rtol=0, atol=1e-14) and np.array_equal(np.diag(s["correlation"]), np.ones(Cc))
    assert np.allclose(s["max_abs"], want["max_abs"], rtol=0, atol=1e-14)
    assert abs(s["effective_rank"] - want["rank"]) <= 1e-12 * Cc and 1.0 <= s["effective_rank"] <= Cc
    assert s["redundant_pairs"] == want["pairs"] and s["redundant_channels"] == int((want["max_abs"] > 0.3).sum())
    off = np.abs(want["rho"])[~np.eye(Cc, dtype=bool)]
    assert abs(s["mean_abs_offdiag"] - off.mean()) <= 1e-14 and s["max_abs_offdiag"] == pytest.approx(off.max(), abs=1e-14)


def test_summary_with_a_dead_and_a_duplicated_channel():
    from tracking.monitor import correlation_summary
    y = _data(300, 5, 1)
    y[:, 1] = 7.0              # zero variance
    y[:, 4] = -2.0 * y[:, 0]   # a copy of channel 0, scaled: rho = -1
    cov = np.cov(y, rowvar=False)
    assert cov[1, 1] == 0.0
    s = correlation_summary(cov, 0.95)
    rho = s["correlation"]
    assert (rho[1, :] == 0).all() and (rho[:, 1] == 0).all()          # 0 wherever a variance is 0, the diagonal included
    assert np.array_equal(np.diag(rho), [1, 0, 1, 1, 1])
    assert abs(rho[0, 4] + 1.0) <= 1e-12 and abs(rho[4, 0] + 1.0) <= 1e-12
    live = [0, 2, 3, 4]
    assert np.allclose(rho[np.ix_(live, live)], np.corrcoef(y[:, live], rowvar=False), rtol=0, atol=1e-12)
    assert s["max_abs"][1] == 0.0 and abs(s["max_abs"][0] - 1.0) <= 1e-12 and abs(s["max_abs"][4] - 1.0) <= 1e-12
    assert s["redundant_pairs"] == 1 and s["redundant_channels"] == 2  # flagged at 0.95
    ev = np.linalg.eigvalsh(cov)
    assert abs(s["effective_rank"] - ev.sum() ** 2 / (ev ** 2).sum()) <= 1e-12
    assert s["effective_rank"] < 3.0 + 1e-9                               # five channels, three directions
    # a negative "variance" (round-off of a device covariance) counts as dead, too
    cov2 = cov.copy()
    cov2[1, 1] = -1e-30
    assert np.array_equal(correlation_summary(cov2)["correlation"], rho)


def test_summary_of_one_channel_and_of_nothing_alive():
    from tracking.monitor import correlation_summary
    s = correlation_summary(np.array([[2.5]]))
    assert s["correlation"].shape == (1, 1) and s["correlation"][0, 0] == 1.0
    assert s["max_abs"].tolist() == [0.0] and s["effective_rank"] == 1.0
    assert s["mean_abs_offdiag"] == 0.0 and s["max_abs_offdiag"] == 0.0 and s["redundant_pairs"] == 0
    z = correlation_summary(np.zeros((3, 3)))
    assert not z["correlation"].any() and z["effective_rank"] == 0.0 and z["max_abs"].tolist() == [0.0] * 3
    assert correlation_summary(2.5)["effective_rank"] == 1.0  # a 0-d covariance is one channel


def test_effective_rank_of_known_spectra():
    from tracking.monitor import correlation_summary
    assert correlation_summary(np.eye(6) * 3.0)["effective_rank"] == pytest.approx(6.0, abs=1e-12)
    u = np.ones((6, 1))
    assert correlation_summary(u @ u.T)["effective_rank"] == pytest.approx(1.0, abs=1e-12)
    assert correlation_summary(np.diag([1.0, 1.0, 0.0, 0.0]))["effective_rank"] == pytest.approx(2.0, abs=1e-12)


# ------------------------------------------------------------------------------------------------ the hook path
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 5, 3, padding=1)
        self.act = torch.nn.ReLU()

    def forward(self, x):
        return self.act(self.conv(x))


def _cov_of(t):
    """float64 covariance of an NCHW tensor's channels over batch and pixels, with numpy"""
    y = t.detach().double().numpy()
    y = np.moveaxis(y, 1, -1).reshape(-1, y.shape[1])
    return np.cov(y, rowvar=False).reshape(y.shape[1], y.shape[1])


def test_compute_metrics_buffers_the_float64_covariance():
    from tracking.monitor import channel_covariance, compute_metrics
    x = torch.randn(2, 5, 4, 6) * torch.arange(1, 6).reshape(1, 5, 1, 1) + 100.0
    out = compute_metrics(x, FOUR)
    assert list(out) == FOUR and all(out[k] is out[COV] for k in FOUR)  # one tensor, shared
    assert out[COV].dtype == torch.float64 and out[COV].shape == (5, 5)
    assert np.allclose(out[COV].numpy(), _cov_of(x), rtol=1e-12, atol=0)
    assert list(compute_metrics(x, [RANK, FUSED])) == [RANK, FUSED]
    assert channel_covariance(torch.randn(7, 1, 3)).shape == (1, 1) and channel_covariance(torch.randn(9)).shape == (1, 1)
    assert compute_metrics(x, ["no_such_metric"]) == {}


def test_hook_path_end_to_end_on_a_plain_module():
    from tracking.monitor import ActivityMonitor, _CovSum, correlation_summary
    torch.manual_seed(0)
    net = _Net()
    cfg = {"enabled": True, "track_interval": 1, "redundancy_threshold": 0.5, "device_metrics": True,  # no engine: hooks anyway
           "target_layers": [{"name": "act", "capture_point": "output", "metrics": [RHO, FUSED, COV, MAXR, RANK, "no_such_metric"]},
                             {"name": "conv", "capture_point": "input", "metrics": [RANK]}]}
    mon = ActivityMonitor(net, cfg)
    assert mon.device_layers == [] and mon.fused_layers == [] and len(mon.hooks) == 2 and mon.redundancy_threshold == 0.5
    xs = [torch.randn(2, 3, 4, 6), torch.randn(2, 3, 4, 6) * 4.0 + 1.0]
    covs = []
    with torch.no_grad():
        for x in xs:
            covs.append(_cov_of(net(x)))
    buf = mon.hook_collected_buffer["act.output"]
    assert list(buf) == [RHO, FUSED, COV, MAXR, RANK]
    # a running sum and a count, not a list: one shared accumulator however many forwards
    assert all(len(buf[k]) == 1 and isinstance(buf[k][0], _CovSum) and buf[k][0] is buf[COV][0] for k in FOUR)
    assert buf[COV][0].n == 2 and len(buf[FUSED]) == 2
    log = mon.step(1)
    data = mon.get_data_for_step(1)
    got = data["act.output"]
    assert list(got) == [RHO, FUSED, COV, MAXR, RANK]
    want = (covs[0] + covs[1]) / 2  # averaged over the two forwards
    assert got[COV].dtype == np.float64 and np.allclose(got[COV], want, rtol=1e-12, atol=1e-300)
    s = correlation_summary(got[COV], 0.5)
    assert got[RHO].dtype == np.float32 and np.array_equal(got[RHO], s["correlation"].astype(np.float32))
    assert got[MAXR].dtype == np.float32 and np.array_equal(got[MAXR], s["max_abs"].astype(np.float32))
    assert isinstance(got[RANK], float) and got[RANK] == s["effective_rank"] and 1.0 <= got[RANK] <= 5.0
    sin = correlation_summary((_cov_of(xs[0]) + _cov_of(xs[1])) / 2)
    assert data["conv.input"][RANK] == pytest.approx(sin["effective_rank"], rel=1e-12)
    base = "tracking/act.output/"
    assert set(log) == {base + RHO + "_mean_abs_offdiag", base + MAXR + "_overall_max", base + RANK,
                        base + FUSED + "_overall_mean", base + FUSED + "_overall_std", "tracking/conv.input/" + RANK}
    assert log[base + RHO + "_mean_abs_offdiag"] == pytest.approx(s["mean_abs_offdiag"], abs=1e-6)
    assert log[base + MAXR + "_overall_max"] == got[MAXR].max() and log[base + RANK] == got[RANK]
    recs = [r for r in mon.export_all_processed_data_to_records() if r["layer_identifier"] == "act.output"]
    kinds = {(r["original_metric_name"], r["metric_type"]): r["metric_value"] for r in recs}
    assert set(kinds) == {(COV, "covariance_shape"), (COV, "covariance_mean_abs_offdiag"), (COV, "covariance_max_abs_offdiag"),
                          (COV, "covariance_redundant_pairs"), (RHO, "correlation_shape"), (RHO, "correlation_mean_abs_offdiag"),
                          (RHO, "correlation_max_abs_offdiag"), (RHO, "correlation_redundant_pairs"),
                          (MAXR, "max_abs_correlation_overall_mean"), (MAXR, "max_abs_correlation_overall_max"),
                          (MAXR, "max_abs_correlation_redundant_channels"), (RANK, "scalar"),
                          (FUSED, "per_channel_overall_mean"), (FUSED, "per_channel_overall_std"),
                          (FUSED, "per_channel_overall_min"), (FUSED, "per_channel_overall_max")}
    assert kinds[(COV, "covariance_shape")] == kinds[(RHO, "correlation_shape")] == "(5, 5)"
    assert kinds[(COV, "covariance_redundant_pairs")] == kinds[(RHO, "correlation_redundant_pairs")] == s["redundant_pairs"]
    assert kinds[(RHO, "correlation_max_abs_offdiag")] == pytest.approx(s["max_abs_offdiag"], abs=1e-6)
    assert kinds[(COV, "covariance_mean_abs_offdiag")] == pytest.approx(s["cov_mean_abs_offdiag"], rel=1e-12)
    assert kinds[(COV, "covariance_max_abs_offdiag")] == pytest.approx(s["cov_max_abs_offdiag"], rel=1e-12)
    assert kinds[(MAXR, "max_abs_correlation_redundant_channels")] == int((got[MAXR] > 0.5).sum())
    assert kinds[(RANK, "scalar")] == got[RANK]
    # the buffer is empty again: the next step starts a new sum
    with torch.no_grad():
        net(xs[0])
    mon.step(2)
    assert np.allclose(mon.get_data_for_step(2)["act.output"][COV], covs[0], rtol=1e-12, atol=1e-300)
    mon.remove_hooks()


def test_known_metrics_are_unchanged():
    from tracking.monitor import CHANCOV_METRICS, KNOWN_METRICS
    assert KNOWN_METRICS == (FUSED, "full_activation_map", "mean_activation", "std_activation", "log2_histogram_per_channel",
                             "abs_max_activation_per_channel", "near_zero_fraction_per_channel")
    assert CHANCOV_METRICS == tuple(FOUR) and not set(CHANCOV_METRICS) & set(KNOWN_METRICS)


# ------------------------------------------------------------------------------------------------ routing
def test_new_config_parses_and_routes_to_the_engine():
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from utils.config_utils import load_config
    from vaehip.engine import CHANCOV_METRICS, CHANHIST_METRICS, DEVICE_METRICS, MOMENT_METRICS
    assert CHANCOV_METRICS == tuple(FOUR) and set(FOUR) <= set(DEVICE_METRICS)
    assert not set(FOUR) & (set(MOMENT_METRICS) | set(CHANHIST_METRICS))
    c = load_config(CFG)
    t = c["tracking"]
    assert t["device_metrics"] is True and float(t["redundancy_threshold"]) == 0.95
    want = ["vae.encoder.down_blocks.0.resnets.0.norm1.output", "vae.encoder.down_blocks.0.resnets.0.conv1.input",
            "vae.encoder.down_blocks.0.resnets.0.output", "vae.encoder.input"]
    named = [f"{e['name']}.{e['capture_point']}" for e in t["target_layers"] if set(FOUR) <= set(e["metrics"])]
    assert named == want
    w = SDXLVAEWrapper("synthetic:1")
    mon = ActivityMonitor(w, t)
    try:
        assert mon.redundancy_threshold == 0.95
        assert mon.device_layers == want + ["vae.decoder.conv_norm_out.input"]
        assert sorted(n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks) == []  # no torch hooks left
        eng = w.vae.engine
        tr = eng._mtrackers[id(w.vae.encoder)]["input"][0]
        assert tr.chancov and not tr.chanhist and not tr.moments and not tr.full_map
        both = eng._mtrackers[id(w.vae.encoder.down_blocks[0].resnets[0].norm1)]["output"][0]
        assert both.chancov and both.moments
    finally:
        mon.remove_hooks()
    mon = ActivityMonitor(w, dict(t, device_metrics=False))  # the same targets on torch hooks
    try:
        assert mon.device_layers == [] and len(mon.fused_layers) == 3
    finally:
        mon.remove_hooks()


def test_wrapper_refuses_before_the_library_is_asked():
    from vaehip import ops
    with pytest.raises(ValueError, match="CUDA tensor"):  # CPU tensors: no fallback
        ops.chancov(torch.zeros(1, 4, 4, 8))


def test_workspace_stays_within_64_mb_at_the_shipped_shapes():
    """the activations of the shipped model at the benchmark's and launch_shapes.py's batches (16 and 32 at 256 x 256): chunks
    x tile pairs fill the device, every chunk is non-empty and the workspace the library asks for stays within 64 MB"""
    from vaehip import ops
    from vaehip.lib import lib
    n = C.c_int64(0)
    for B in (1, 2, 16, 32):
        for HW, Cc in ((256 * 256, 3), (256 * 256, 128), (128 * 128, 128), (128 * 128, 256), (64 * 64, 256), (64 * 64, 512),
                       (32 * 32, 512), (32 * 32, 8), (32 * 32, 4)):
            nch = ops.chancov_chunks(B, HW, Cc)
            lib.call("vae_chancov_workspace", B, HW, Cc, nch, C.byref(n))  # refuses an empty chunk
            assert n.value * 4 <= ops.CHANCOV_WS_BYTES == 64 << 20, (B, HW, Cc, nch, n.value * 4)
            tiles = -(-Cc // 128)
            assert nch == 1 or B * nch * tiles * (tiles + 1) // 2 <= 1024
    assert ops.chancov_chunks(16, 256 * 256, 128) == 63 and ops.chancov_chunks(1, 2, 1) == 1 and ops.chancov_chunks(3, 91, 8) == 2


# ------------------------------------------------------------------------------------------------ library, no GPU
def test_tile_and_workspace_queries_and_refusals_need_no_gpu():
    from vaehip.lib import lib, VaeHipError
    T = lib.query("vae_chancov_tile")
    assert T == 128
    n = C.c_int64(0)
    lib.call("vae_chancov_workspace", 3, 16 * 16, T, 4, C.byref(n))
    assert n.value == 3 * 4 * (T * T + 2 * T) + T  # per (image, chunk): one fp32 tile and one float64 row; K once
    lib.call("vae_chancov_workspace", 1, 2, 1, 1, C.byref(n))
    assert n.value == T * T + 2 * T + T
    lib.call("vae_chancov_workspace", 2, 64, 2 * T + 1, 2, C.byref(n))  # three tiles: six pairs of the upper triangle
    assert n.value == 4 * (6 * T * T + 2 * 3 * T) + 3 * T
    with pytest.raises(VaeHipError, match="chancov_workspace: bad args"):
        lib.call("vae_chancov_workspace", 0, 16, 8, 1, C.byref(n))
    with pytest.raises(VaeHipError, match="null args"):
        lib.call("vae_chancov_workspace", 1, 16, 8, 1, None)
    with pytest.raises(VaeHipError, match="empty chunk"):
        lib.call("vae_chancov_workspace", 1, 10, 8, 7, C.byref(n))  # chunks of 2 pixels: the last two of 7 are empty
    with pytest.raises(VaeHipError, match="two rows"):
        lib.call("vae_chancov_workspace", 1, 1, 8, 1, C.byref(n))
    with pytest.raises(VaeHipError, match="2\\^31"):
        lib.call("vae_chancov_workspace", 32768, 65536, 8, 1, C.byref(n))
    # the launch entry points refuse on the host, before any launch (the pointers are never followed)
    p = C.c_void_p(4096)

    def partial(x=p, sc=None, sh=None, xf=0, B=2, HW=64, Cc=8, ld=8, nch=2, ws=p):
        lib.call("vae_chancov_partial", x, 0, sc, sh, xf, B, HW, Cc, ld, nch, ws, None)

    for kw, msg in [(dict(x=None), "null args"), (dict(ws=None), "null args"), (dict(ld=7), "pixel stride ld=7 below C=8"),
                    (dict(nch=33, HW=64), "empty chunk"), (dict(xf=1), "xf needs scale and shift"),
                    (dict(xf=2, sc=p), "xf needs scale and shift"), (dict(xf=3, sc=p, sh=p), "xf=3"),
                    (dict(ws=C.c_void_p(4096 + 8)), "unaligned workspace"), (dict(B=1, HW=1, nch=1), "two rows"),
                    (dict(B=32768, HW=65536), "2\\^31"), (dict(Cc=0), "bad args")]:
        with pytest.raises(VaeHipError, match="chancov_partial.*" + msg):
            partial(**kw)
    f64 = C.c_void_p(8192)
    for args, msg in [((None, 2, 64, 8, 2, f64, f64), "null args"), ((p, 2, 64, 8, 2, None, f64), "null args"),
                      ((p, 2, 64, 8, 2, f64, None), "null args"), ((C.c_void_p(4100), 2, 64, 8, 2, f64, f64), "unaligned workspace"),
                      ((p, 2, 64, 8, 33, f64, f64), "empty chunk"), ((p, 1, 1, 8, 1, f64, f64), "two rows"),
                      ((p, 32768, 65536, 8, 1, f64, f64), "2\\^31")]:
        with pytest.raises(VaeHipError, match="chancov_final.*" + msg):
            lib.call("vae_chancov_final", *args, None)
