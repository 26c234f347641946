"""The GroupNorm group dynamics and per-sample activity metrics without a GPU: the torch formulas (ops.changroup_metrics,
tracking.monitor.per_sample_sums / changroup_summary / compute_metrics) on hand-made cases and against the two-pass float64
reference of tests/changroup_refs.py, the monitor's hook path end to end (G and eps of a target, the refusals, aggregation over
forwards of different batch sizes, log keys, the records export), the new config's routing, ops.changroup_chunks and the
library's size query and refusals."""
import ctypes as C
import logging
import os

import numpy as np
import pytest
import torch

import changroup_refs as R
from changroup_refs import ACTIVE, DOM, FIVE, NRMS, SHARE, VARIATION

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_group_dynamics.yaml")
FUSED = "mean_abs_activation_per_channel"


def _sums(t):
    """NCHW tensor -> float64 [B, C, 3] with numpy"""
    y = t.detach().double().numpy()
    y = y.reshape(y.shape[0], y.shape[1], -1)
    return np.stack([y.sum(axis=2), (y * y).sum(axis=2), np.abs(y).sum(axis=2)], axis=2)


def _nhwc(t):
    """NCHW tensor -> float64 [B, HW, C] for the reference"""
    y = t.detach().double().numpy()
    return np.moveaxis(y.reshape(y.shape[0], y.shape[1], -1), 1, 2)


def _five(t, G, eps=1e-6, tau=1e-3):
    from tracking.monitor import changroup_summary, per_sample_sums
    from vaehip.ops import changroup_metrics
    chan, grp, S = changroup_metrics(per_sample_sums(t), t[0, 0].numel(), G, eps, tau)
    return changroup_summary(chan.numpy(), grp.numpy(), S)


# ------------------------------------------------------------------------------------------------ formulas
def test_per_sample_sums_against_numpy():
    from tracking.monitor import per_sample_sums
    x = torch.randn(3, 8, 5, 7) * 2.0 + 1000.0
    s = per_sample_sums(x)
    assert s.dtype == torch.float64 and s.shape == (3, 8, 3)
    assert np.allclose(s.numpy(), _sums(x), rtol=1e-14, atol=0)
    assert per_sample_sums(x.bfloat16()).dtype == torch.float64  # widened exactly, whatever the storage
    assert per_sample_sums(torch.randn(9)).shape == (1, 1, 3) and per_sample_sums(torch.randn(4, 6)).shape == (4, 6, 3)


@pytest.mark.parametrize("B,Cc,G,mean", [(3, 8, 2, 0.4), (1, 32, 32, 0.0), (2, 12, 3, 1000.0), (5, 64, 32, -3.0)])
def test_formulas_against_the_two_pass_reference(B, Cc, G, mean):
    x = R.draw((B, Cc, 6, 5), B * 100 + Cc) + mean
    x[:, 1] *= 30.0  # an outlier channel
    got = _five(x, G, eps=1e-6, tau=0.5)
    want = R.ref_metrics(_nhwc(x), G, 1e-6, 0.5)
    assert list(got) == FIVE
    for k in FIVE:
        assert got[k].dtype == np.float32 and got[k].shape == ((G,) if k == DOM else (Cc,))
        # the one-pass form loses log2((mean / sigma)^2) of float64's 53 bits: 20 at mean = 10^3 sigma
        assert np.allclose(got[k], want[k], rtol=1e-6, atol=1e-7), k


def test_shares_of_a_group_sum_to_one_per_sample():
    from tracking.monitor import per_sample_sums
    from vaehip.ops import changroup_metrics
    x = R.draw((4, 12, 5, 5), 3)
    chan, grp, S = changroup_metrics(per_sample_sums(x), 25, 3, 1e-6, 1e-3)
    assert S == 4 and chan.shape == (5, 12) and grp.shape == (3,) and chan.dtype == grp.dtype == torch.float64
    assert np.allclose(chan[0].reshape(3, 4).sum(dim=1).numpy(), 4.0, rtol=1e-12)  # sum over the samples of (1 per group)
    assert bool((grp >= 4.0 / 4 - 1e-12).all()) and bool((grp <= 4.0).all())   # the largest of cg = 4 shares is >= 1 / 4


def test_one_hot_group_and_a_constant_group():
    """group 0: channel 2 alternates +-1 around the group's mean 0, its three mates are 0: it owns the group.  Group 1 is constant
    in sample 0 (V = 0: shares 0, not NaN) and ordinary in sample 1"""
    x = torch.zeros(2, 8, 4, 4)
    x[:, 2] = torch.tensor([1.0, -1.0]).repeat(8).reshape(4, 4)
    x[0, 4:] = 0.75
    x[1, 4:] = R.draw((4, 4, 4), 9)
    from tracking.monitor import per_sample_sums
    from vaehip.ops import changroup_metrics
    chan, grp, S = changroup_metrics(per_sample_sums(x), 16, 2, 1e-6, 1e-3)
    share, nrms = chan[0].numpy() / 2, chan[1].numpy() / 2
    assert share[:4].tolist() == [0.0, 0.0, 1.0, 0.0] and grp[0].item() == 2.0
    assert nrms[:4].tolist() == pytest.approx([0.0, 0.0, np.sqrt(1.0 / (0.25 + 1e-6)), 0.0], rel=1e-12)
    assert np.isfinite(chan.numpy()).all() and np.isfinite(grp.numpy()).all()
    assert share[4:].sum() == pytest.approx(0.5, rel=1e-12)  # sample 0 gives 0 to every channel, sample 1 shares that sum to 1
    got = _five(x, 2)
    assert got[SHARE][2] == 1.0 and got[DOM][0] == 1.0 and got[ACTIVE].tolist() == [0, 0, 1, 0, 1, 1, 1, 1]


def test_a_single_sample():
    x = R.draw((1, 8, 3, 3), 4)
    got = _five(x, 4, tau=0.0)
    want = R.ref_metrics(_nhwc(x), 4, 1e-6, 0.0)
    for k in FIVE:
        assert np.allclose(got[k], want[k], rtol=1e-6, atol=1e-7), k
    assert (got[VARIATION] == 0.0).all() and (got[ACTIVE] == 1.0).all()  # one sample does not vary; tau 0: everything is active


def test_selective_against_fading_channel():
    """channel 0 is strongly active on 1 image of 16 and silent on the rest, channel 1 weakly active everywhere: the same mean |A|,
    which is all the batch average sees"""
    from tracking.monitor import compute_metrics
    x = torch.zeros(16, 2, 4, 4)
    x[5, 0] = 1.6
    x[:, 1] = 0.1
    assert compute_metrics(x, [FUSED])[FUSED].tolist() == pytest.approx([0.1, 0.1], rel=1e-6)
    got = _five(x, None, tau=1e-3)
    assert list(got) == FIVE and got[SHARE].tolist() == [0.0, 0.0] and got[DOM].shape == (0,)  # no group metric asked for
    assert got[ACTIVE].tolist() == [1.0 / 16, 1.0]
    assert got[VARIATION].tolist() == pytest.approx([np.sqrt(15.0), 0.0], rel=1e-6, abs=1e-7)


def test_nan_and_inf_stay_in_their_sample_and_group():
    from tracking.monitor import per_sample_sums
    from vaehip.ops import changroup_metrics
    x = R.draw((3, 8, 4, 4), 5)
    x[1, 5, 2, 2] = float("nan")
    x[2, 0, 0, 0] = float("inf")
    sums = per_sample_sums(x)
    for b in range(3):  # sample by sample: what each (b, group) gives
        chan, grp, S = changroup_metrics(sums[b:b + 1], 16, 2, 1e-6, 1e-3)
        bad_g = {0: None, 1: 1, 2: 0}[b]
        for g in range(2):
            ok = np.isfinite(chan[:2, 4 * g:4 * g + 4].numpy()).all() and np.isfinite(grp[g].item())
            assert ok == (g != bad_g), (b, g)
        bad_c = {0: None, 1: 5, 2: 0}[b]
        assert [c for c in range(8) if not np.isfinite(chan[2:4, c].numpy()).all()] == ([] if bad_c is None else [bad_c])


def test_compute_metrics_shares_one_result_and_summary_matches_the_refs_restatement():
    from tracking.monitor import CHANGROUP_METRICS, GROUP_METRICS, SAMPLE_METRICS, changroup_summary, compute_metrics
    assert CHANGROUP_METRICS == tuple(FIVE) and GROUP_METRICS == (SHARE, NRMS, DOM) and SAMPLE_METRICS == (ACTIVE, VARIATION)
    x = R.draw((3, 8, 4, 4), 6)
    out = compute_metrics(x, FIVE + [FUSED], 0.5, (4, 1e-5))
    assert list(out) == FIVE + [FUSED] and all(out[k] is out[SHARE] for k in FIVE)  # one tuple, shared
    chan, grp, S = out[SHARE]
    got = changroup_summary(chan.numpy(), grp.numpy(), S)
    mine = R.metrics_from_ops((chan, grp, S), 4)
    want = R.ref_metrics(_nhwc(x), 4, 1e-5, 0.5)
    for k in FIVE:
        assert np.array_equal(got[k], mine[k].astype(np.float32)), k
        assert np.allclose(got[k], want[k], rtol=1e-6, atol=1e-7), k
    assert list(compute_metrics(x, [ACTIVE], 0.5, (None, 1e-6))) == [ACTIVE]
    assert compute_metrics(x, [SHARE], 0.5, (3, 1e-6)) == {}  # 8 channels, 3 groups: logged, nothing served


def test_compute_metrics_logs_an_undivided_group_once_and_keeps_the_sample_metrics(caplog):
    from tracking import monitor as M
    x = R.draw((3, 8, 4, 4), 6)
    real, calls = M.per_sample_sums, []
    M.per_sample_sums = lambda t: (calls.append(1), real(t))[1]
    try:
        with caplog.at_level(logging.ERROR, logger="tracking.monitor"):
            out = M.compute_metrics(x, [SHARE, ACTIVE, NRMS, DOM, VARIATION, FUSED], 0.5, (3, 1e-6))
    finally:
        M.per_sample_sums = real
    errors = [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
    assert len(errors) == 1 and "8 channels do not divide into 3 groups" in errors[0] and len(calls) == 1  # once, not per name
    assert list(out) == [ACTIVE, VARIATION, FUSED] and out[ACTIVE] is out[VARIATION]
    got = M.changroup_summary(out[ACTIVE][0].numpy(), out[ACTIVE][1].numpy(), out[ACTIVE][2])
    want = R.ref_metrics(_nhwc(x), None, 1e-6, 0.5)
    assert np.allclose(got[ACTIVE], want[ACTIVE]) and np.allclose(got[VARIATION], want[VARIATION], rtol=1e-6, atol=1e-7)


def test_changroup_metrics_refuses_bad_arguments():
    from vaehip.ops import changroup_metrics
    s = torch.zeros((2, 8, 3), dtype=torch.float64)
    for args, msg in [((s.float(), 4, 2, 1e-6, 0.0), "float64"), ((s[:, :, :2], 4, 2, 1e-6, 0.0), "float64"),
                      ((s, 4, 3, 1e-6, 0.0), "do not divide"), ((s, 4, 0, 1e-6, 0.0), "do not divide"), ((s, 0, 2, 1e-6, 0.0), "HW")]:
        with pytest.raises(ValueError, match=msg):
            changroup_metrics(*args)


def test_known_metrics_are_unchanged():
    from tracking.monitor import CHANCOV_METRICS, CHANGROUP_METRICS, KNOWN_METRICS
    assert KNOWN_METRICS == (FUSED, "full_activation_map", "mean_activation", "std_activation", "log2_histogram_per_channel",
                             "abs_max_activation_per_channel", "near_zero_fraction_per_channel")
    assert not set(CHANGROUP_METRICS) & (set(KNOWN_METRICS) | set(CHANCOV_METRICS))


# ------------------------------------------------------------------------------------------------ monitor, hook path
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.norm = torch.nn.GroupNorm(2, 8, eps=1e-4)
        self.act = torch.nn.SiLU()

    def forward(self, x):
        return self.act(self.norm(self.conv(x)))


def test_hook_path_end_to_end_on_a_plain_module(caplog):
    from tracking.monitor import ActivityMonitor, _GroupSum
    torch.manual_seed(0)
    net = _Net()
    cfg = {"enabled": True, "track_interval": 1, "device_metrics": True, "near_zero_threshold": 0.3, "group_count": 4, "group_eps": 1e-3,
           "target_layers": [{"name": "norm", "capture_point": "input", "metrics": FIVE + [FUSED]},        # G, eps: the norm's own
                             {"name": "conv", "capture_point": "output", "metrics": [SHARE, VARIATION]},  # tracking.group_*
                             {"name": "act", "capture_point": "output", "metrics": [DOM, ACTIVE], "groups": 8},
                             {"name": "conv", "capture_point": "input", "metrics": [ACTIVE, VARIATION]},  # 3 channels: no G needed
                             {"name": "norm", "capture_point": "output", "metrics": [NRMS], "groups": 3},  # 8 % 3: refused
                             {"name": "conv", "capture_point": "input", "metrics": [SHARE, ACTIVE]}]}     # 3 % 4: refused
    with caplog.at_level(logging.ERROR, logger="tracking.monitor"):
        mon = ActivityMonitor(net, cfg)
    errors = [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
    assert len(errors) == 2 and "layer norm (output)" in errors[0] and NRMS in errors[0] and "layer conv (input)" in errors[1]
    assert len(mon.hooks) == 4 and mon.device_layers == []
    assert mon._groups == {"norm.input": (2, 1e-4), "conv.output": (4, 1e-3), "act.output": (8, 1e-3), "conv.input": (None, 1e-3)}
    xs = [torch.randn(2, 3, 4, 6), torch.randn(5, 3, 4, 6) * 4.0 + 1.0]  # two forwards of different batch sizes
    pre, outs = [], []
    with torch.no_grad():
        for x in xs:
            pre.append(net.conv(x))
            outs.append(net(x))
    buf = mon.hook_collected_buffer["norm.input"]
    assert list(buf) == FIVE + [FUSED]
    assert all(len(buf[k]) == 1 and isinstance(buf[k][0], _GroupSum) and buf[k][0] is buf[SHARE][0] for k in FIVE)
    assert buf[SHARE][0].samples == 7 and buf[SHARE][0].forwards == 2 and len(buf[FUSED]) == 2
    log = mon.step(1)
    data = mon.get_data_for_step(1)
    # every sample counts once, whatever forward it came in: the values of the concatenated batch
    allpre, allout, allx = torch.cat(pre), torch.cat(outs), torch.cat(xs)
    want = R.ref_metrics(_nhwc(allpre), 2, 1e-4, 0.3)
    got = data["norm.input"]
    assert list(got) == FIVE + [FUSED]
    for k in FIVE:
        assert got[k].dtype == np.float32 and np.allclose(got[k], want[k], rtol=1e-6, atol=1e-7), k
    want = R.ref_metrics(_nhwc(allpre), 4, 1e-3, 0.3)
    assert list(data["conv.output"]) == [SHARE, VARIATION]
    assert all(np.allclose(data["conv.output"][k], want[k], rtol=1e-6, atol=1e-7) for k in (SHARE, VARIATION))
    want = R.ref_metrics(_nhwc(allout), 8, 1e-3, 0.3)
    assert (data["act.output"][DOM] == 1.0).all() and data["act.output"][DOM].shape == (8,)  # cg = 1: every channel owns its group
    assert np.allclose(data["act.output"][ACTIVE], want[ACTIVE])
    want = R.ref_metrics(_nhwc(allx), None, 1e-3, 0.3)
    assert all(np.allclose(data["conv.input"][k], want[k], rtol=1e-6, atol=1e-7) for k in (ACTIVE, VARIATION))
    base = "tracking/norm.input/"
    mine = {k: v for k, v in log.items() if k.startswith(base) and FUSED not in k}
    assert set(mine) == {base + SHARE + "_squashed_channels", base + SHARE + "_overall_max", base + NRMS + "_overall_min",
                         base + DOM + "_overall_max", base + DOM + "_most_dominated_group", base + ACTIVE + "_overall_min",
                         base + VARIATION + "_overall_max"}
    assert mine[base + DOM + "_most_dominated_group"] == int(np.argmax(got[DOM]))
    assert mine[base + SHARE + "_squashed_channels"] == int((got[SHARE] < 0.1 / 4).sum())  # uniform share 1 / cg = 1 / 4
    recs = [r for r in mon.export_all_processed_data_to_records() if r["layer_identifier"] == "norm.input"]
    kinds = {(r["original_metric_name"], r["metric_type"]): r["metric_value"] for r in recs if r["original_metric_name"] != FUSED}
    names = {SHARE: "group_variance_share", NRMS: "normalized_rms", DOM: "group_dominance", ACTIVE: "active_sample_fraction",
             VARIATION: "sample_variation"}
    want_kinds = {(m, n + s) for m, n in names.items() for s in ("_overall_mean", "_overall_min", "_overall_max")}
    want_kinds |= {(SHARE, "group_variance_share_squashed_channels"), (DOM, "group_dominance_argmax_group"),
                   (ACTIVE, "active_sample_fraction_silent_channels")}
    assert set(kinds) == want_kinds
    assert kinds[(DOM, "group_dominance_argmax_group")] == int(np.argmax(got[DOM]))
    assert kinds[(SHARE, "group_variance_share_overall_max")] == float(got[SHARE].max())
    assert kinds[(ACTIVE, "active_sample_fraction_silent_channels")] == int((got[ACTIVE] == 0).sum())
    # the buffer is empty again: the next step starts new sums
    with torch.no_grad():
        net(xs[0])
    mon.step(2)
    want = R.ref_metrics(_nhwc(pre[0]), 2, 1e-4, 0.3)
    assert np.allclose(mon.get_data_for_step(2)["norm.input"][SHARE], want[SHARE], rtol=1e-6, atol=1e-7)
    mon.remove_hooks()


def test_a_plain_module_with_unknown_channels_is_dropped_at_its_first_forward_with_one_error(caplog):
    """registration cannot know the channels of a SiLU; the first forward finds 8 channels for 3 groups: the layer is dropped with
    one logged error (no exception, no traceback per forward), the other targets go on"""
    from tracking.monitor import ActivityMonitor
    net = _Net()
    cfg = {"enabled": True, "track_interval": 1, "group_count": 3,
           "target_layers": [{"name": "act", "capture_point": "output", "metrics": [SHARE, ACTIVE]},
                             {"name": "act", "capture_point": "input", "metrics": [ACTIVE]},
                             {"name": "norm", "capture_point": "input", "metrics": [DOM], "groups": 0},
                             {"name": "norm", "capture_point": "input", "metrics": [DOM], "groups": "8"},
                             {"name": "conv", "capture_point": "output", "metrics": [NRMS], "groups": True}]}
    with caplog.at_level(logging.ERROR, logger="tracking.monitor"):
        mon = ActivityMonitor(net, cfg)
        errors = [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
        assert len(errors) == 3 and all("groups must be a positive integer" in e for e in errors)
        assert "layer norm (input)" in errors[0] and "not 0" in errors[0] and "not '8'" in errors[1] and "layer conv (output)" in errors[2]
        assert len(mon.hooks) == 2 and mon._groups == {"act.output": (3, 1e-6), "act.input": (None, 1e-6)}
        caplog.clear()
        with torch.no_grad():
            for _ in range(3):
                net(torch.randn(2, 3, 4, 6))
        errors = [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
    assert len(errors) == 1 and "act.output" in errors[0] and "8 channels do not divide into 3" in errors[0]
    mon.step(1)
    data = mon.get_data_for_step(1)
    assert list(data) == ["act.input"] and list(data["act.input"]) == [ACTIVE]
    mon.remove_hooks()


def test_planted_outlier_squashes_its_group_mates_on_the_hook_path():
    """the mechanism the metrics exist for: one filter row times 100 in front of a GroupNorm"""
    from tracking.monitor import ActivityMonitor
    torch.manual_seed(1)
    net = _Net()
    cfg = {"enabled": True, "track_interval": 1, "target_layers": [{"name": "norm", "capture_point": "input", "metrics": [SHARE, NRMS, DOM]}]}
    mon = ActivityMonitor(net, cfg)
    x = torch.randn(4, 3, 8, 8)
    with torch.no_grad():
        net.conv.bias.zero_()
        net(x)
        mon.step(1)
        net.conv.weight[5] *= 100.0
        net(x)
        mon.step(2)
    a, b = mon.get_data_for_step(1)["norm.input"], mon.get_data_for_step(2)["norm.input"]
    assert b[SHARE][5] > 0.9 and b[DOM][1] > 0.9 and (b[NRMS][[4, 6, 7]] < 0.1 * a[NRMS][[4, 6, 7]]).all()
    assert np.array_equal(a[SHARE][:4], b[SHARE][:4]) and np.array_equal(a[NRMS][:4], b[NRMS][:4]) and a[DOM][0] == b[DOM][0]
    mon.remove_hooks()


# ------------------------------------------------------------------------------------------------ routing
def test_new_config_parses_and_routes_to_the_engine(caplog):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from utils.config_utils import load_config
    from vaehip.engine import CHANCOV_METRICS, CHANGROUP_METRICS, CHANHIST_METRICS, DEVICE_METRICS, MOMENT_METRICS, SERVED_METRICS
    assert CHANGROUP_METRICS == tuple(FIVE) and SERVED_METRICS == DEVICE_METRICS + tuple(FIVE)
    assert not set(FIVE) & (set(MOMENT_METRICS) | set(CHANHIST_METRICS) | set(CHANCOV_METRICS))
    c = load_config(CFG)
    t = c["tracking"]
    assert t["device_metrics"] is True and int(t["group_count"]) == 32 and float(t["group_eps"]) == 1e-6
    want = ["vae.decoder.conv_norm_out.input", "vae.decoder.up_blocks.0.resnets.0.norm1.input", "vae.decoder.up_blocks.1.resnets.0.conv1.output"]
    named = [f"{e['name']}.{e['capture_point']}" for e in t["target_layers"] if set(FIVE) <= set(e["metrics"])]
    assert named == want
    # the all-metrics run it extends is otherwise the same
    base = load_config(os.path.join(os.path.dirname(CFG), "experiment_synthetic_all_metrics.yaml"))
    strip = lambda e: dict(e, metrics=[m for m in e["metrics"] if m not in FIVE])  # noqa: E731
    assert [strip(e) for e in t["target_layers"] if strip(e)["metrics"]] == base["tracking"]["target_layers"]
    w = SDXLVAEWrapper("synthetic:1")
    mon = ActivityMonitor(w, t)
    try:
        assert set(want) <= set(mon.device_layers)
        assert sorted(n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks) == []  # no torch hooks left
        eng, dec = w.vae.engine, w.vae.decoder
        tr = eng._mtrackers[id(dec.up_blocks[0].resnets[0].norm1)]["input"][0]
        assert tr.changroup and not tr.chanhist and not tr.moments and not tr.full_map and not tr.chancov
        both = eng._mtrackers[id(dec.conv_norm_out)]["input"][0]
        assert both.changroup and both.moments
        norm = dec.up_blocks[0].resnets[0].norm1
        assert mon._groups["vae.decoder.up_blocks.0.resnets.0.norm1.input"] == (norm.num_groups, norm.eps)
        assert mon._groups["vae.decoder.up_blocks.1.resnets.0.conv1.output"] == (32, 1e-6)
    finally:
        mon.remove_hooks()
    # the 3-channel image, the 4-channel latent and the 8-channel moments do not divide into 32 groups: a group metric is
    # refused with a logged error that names the layer, the sample metrics are served
    ends = {"enabled": True, "track_interval": 1, "device_metrics": True, "target_layers": [
        {"name": "vae.encoder", "capture_point": "input", "metrics": [ACTIVE, VARIATION]},
        {"name": "vae.decoder.conv_out", "capture_point": "output", "metrics": [SHARE]},
        {"name": "vae.encoder.conv_out", "capture_point": "output", "metrics": [FUSED, DOM]},
        {"name": "vae.decoder.conv_in", "capture_point": "input", "metrics": [NRMS, ACTIVE]},
        {"name": "vae.encoder.conv_out", "capture_point": "output", "metrics": [SHARE], "groups": 4},
        # the inputs of composite engine modules: the image, the latent, and a mid block of 512 channels in 7 groups
        {"name": "vae.encoder", "capture_point": "input", "metrics": [SHARE]},
        {"name": "vae.decoder", "capture_point": "input", "metrics": [DOM, ACTIVE]},
        {"name": "vae.decoder.mid_block", "capture_point": "input", "metrics": [NRMS], "groups": 7},
        {"name": "vae.decoder.mid_block", "capture_point": "input", "metrics": [NRMS], "groups": 8}]}
    with caplog.at_level(logging.ERROR, logger="tracking.monitor"):
        mon = ActivityMonitor(w, ends)
    try:
        errors = [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
        refused = ("layer vae.decoder.conv_out (output)", "layer vae.encoder.conv_out (output)", "layer vae.decoder.conv_in (input)",
                   "layer vae.encoder (input)", "layer vae.decoder (input)", "layer vae.decoder.mid_block (input)")
        assert len(errors) == len(refused) and all(n in e for n, e in zip(refused, errors))
        assert "3 channels do not divide into 32" in errors[3] and "4 channels do not divide into 32" in errors[4]
        assert "channels do not divide into 7" in errors[5]
        assert mon.device_layers == ["vae.encoder.input", "vae.encoder.conv_out.output", "vae.decoder.mid_block.input"]
        assert mon._groups == {"vae.encoder.input": (None, 1e-6), "vae.encoder.conv_out.output": (4, 1e-6),
                               "vae.decoder.mid_block.input": (8, 1e-6)}
        # both ends of every module the engine serves are known at registration
        eng = w.vae.engine
        for name, m in w.named_modules():
            if eng.metric_trackable(m):
                assert eng._in_channels(m) > 0 and eng._out_channels(m) > 0, name
        assert eng._in_channels(w.vae.encoder) == 3 and eng._in_channels(w.vae.decoder) == 4
        assert eng._in_channels(w.vae.decoder.up_blocks[0].upsamplers[0]) == eng._out_channels(w.vae.decoder.up_blocks[0])
    finally:
        mon.remove_hooks()
    mon = ActivityMonitor(w, dict(t, device_metrics=False))  # the same targets on torch hooks
    try:
        assert not set(want) & set(mon.device_layers)
        assert len([n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks]) >= 3
    finally:
        mon.remove_hooks()


def test_wrapper_refuses_before_the_library_is_asked():
    from vaehip import ops
    with pytest.raises(ValueError, match="changroup: expected a 4-D NHWC fp32 / bf16 CUDA tensor"):  # CPU tensors: no fallback
        ops.changroup(torch.zeros(1, 4, 4, 8))


# ------------------------------------------------------------------------------------------------ chunks, library
def _shipped_shapes():
    """(batch, {(H * W, C)}) of tools/launch_shapes.py: every 4-D activation of the model it builds, at the batch and resolution
    it runs by default, read from the tool's own text and the model's own modules"""
    import re
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    src = open(os.path.join(ROOT, "tools", "launch_shapes.py")).read()
    batch = int(re.search(r'"--batch", type=int, default=(\d+)', src).group(1))
    res = int(re.search(r'"--res", type=int, default=(\d+)', src).group(1))
    vae = SDXLVAEWrapper(re.search(r'SDXLVAEWrapper\("([^"]+)"', src).group(1)).vae
    shapes = set()

    def conv(m, r_in, r_out):
        shapes.update({(r_in * r_in, m.in_channels), (r_out * r_out, m.out_channels)})

    def resnets(blk, r):
        for rn in blk.resnets:
            shapes.update({(r * r, rn.norm1.num_channels), (r * r, rn.norm2.num_channels)})

    enc, dec = vae.encoder, vae.decoder
    conv(enc.conv_in, res, res)
    for blk in enc.down_blocks:
        resnets(blk, res)
        if blk.downsamplers is not None:
            conv(blk.downsamplers[0].conv, res, res // 2)
            res //= 2
    resnets(enc.mid_block, res)
    conv(enc.conv_out, res, res)
    conv(vae.quant_conv, res, res)
    conv(vae.post_quant_conv, res, res)
    conv(dec.conv_in, res, res)
    resnets(dec.mid_block, res)
    for blk in dec.up_blocks:
        resnets(blk, res)
        if blk.upsamplers is not None:
            conv(blk.upsamplers[0].conv, 2 * res, 2 * res)
            res *= 2
    conv(dec.conv_out, res, res)
    return batch, sorted(shapes)


def _chanhist_words(B, HW, Cc):
    """what ops.chanhist allocates: its chunk rule (vaehip/ops.py) times 50 words per (image, chunk, channel)"""
    units, tile = (Cc // 4, 32) if Cc % 4 == 0 else (Cc, 128)
    pr = max(1, 256 // min(tile, units))
    tiles = (units + tile - 1) // tile
    nch = max(1, min(1024 // max(B * tiles, 1), HW // (16 * pr)))
    per = (HW + nch - 1) // nch
    nch = (HW + per - 1) // per
    from vaehip.lib import lib
    n = C.c_int64(0)
    lib.call("vae_chanhist_workspace", B, HW, Cc, nch, C.byref(n))
    return n.value


def test_chunks_are_non_empty_and_the_workspace_stays_below_the_histogram_pass():
    """every activation shape of the shipped model as tools/launch_shapes.py runs it (its batch, 32, and resolution, 256), at the
    benchmark's batch 16 and at 1 and 2 as well, and a sweep of small shapes: every chunk non-empty (the library refuses an empty
    one), the workspace in bytes at or below what ops.chanhist allocates for the same tensor"""
    from vaehip import ops
    from vaehip.lib import lib
    n = C.c_int64(0)
    batch, shipped = _shipped_shapes()
    assert batch == 32 and {(256 * 256, 3), (256 * 256, 128), (128 * 128, 256), (64 * 64, 512), (32 * 32, 512), (32 * 32, 8),
                            (32 * 32, 4)} <= set(shipped)
    for B in sorted({1, 2, 16, batch}):
        for HW, Cc in shipped:
            nch = ops.changroup_chunks(B, HW, Cc)
            lib.call("vae_changroup_workspace", B, HW, Cc, nch, C.byref(n))
            assert n.value == B * nch * Cc * 3
            assert n.value * 8 <= _chanhist_words(B, HW, Cc) * 4, (B, HW, Cc, nch)
            tiles = -(-(Cc // 4 if Cc % 4 == 0 else Cc) // (64 if Cc % 4 == 0 else 256))
            assert nch == 1 or B * nch * tiles <= 1024
    for B in (1, 3):
        for HW in (1, 2, 15, 16, 17, 35, 255, 256, 257, 1023, 4097):
            for Cc in (1, 3, 4, 8, 32, 64, 132, 260, 512, 1028):
                nch = ops.changroup_chunks(B, HW, Cc)
                per = -(-HW // nch)
                assert 1 <= nch <= HW and (nch - 1) * per < HW, (B, HW, Cc, nch)
                assert nch == R.chunks(B, HW, Cc)  # the references' restatement
                lib.call("vae_changroup_workspace", B, HW, Cc, nch, C.byref(n))
    assert ops.changroup_chunks(16, 256 * 256, 128) == 64 and ops.changroup_chunks(1, 1, 3) == 1


def test_the_derived_share_bound_is_small_where_fp32_accumulators_would_fail():
    """the references' own condition, on the CPU: at mean = 10^3 sigma the bound from float64 chains is far below 1 % of the
    uniform share; the same chains with u = 2^-24 would give a bound above it"""
    from tracking.monitor import per_sample_sums
    from vaehip import ops
    x = torch.randn(2, 33, 31, 32) + 1000.0
    sums, rad = R.ref_sums(x)
    b = R.metric_bounds(sums, rad, 33 * 31, 8, 1e-6, 1e-3)
    # the chains the radii are derived from are those of the op's own chunk rule, and the op's arithmetic on float64 sums of the
    # same tensor stays inside the bounds
    nch = ops.changroup_chunks(2, 33 * 31, 32)
    assert nch == R.chunks(2, 33 * 31, 32) and (R.chain_depth(2, 33 * 31, 32) == -(-(-(-33 * 31 // nch)) // 32) + 32 + nch).all()
    mine = R.metrics_from_ops(ops.changroup_metrics(per_sample_sums(x.permute(0, 3, 1, 2)), 33 * 31, 8, 1e-6, 1e-3), 8)
    R.assert_within(mine, b)
    assert R.assert_share_bound_small(b, 32, 8) < 1e-7
    b32 = R.metric_bounds(sums, rad * 2.0 ** 29, 33 * 31, 8, 1e-6, 1e-3)
    with pytest.raises(AssertionError):
        R.assert_share_bound_small(b32, 32, 8)
    want = R.ref_metrics(R.values(x)[0], 8, 1e-6, 1e-3)
    R.assert_within(R.summarise(*R.per_sample(R.values(x)[0], 8, 1e-6), 1e-3), b, want)


def test_workspace_query_and_refusals_need_no_gpu():
    from vaehip.lib import lib, VaeHipError
    n = C.c_int64(0)
    lib.call("vae_changroup_workspace", 3, 16 * 16, 130, 4, C.byref(n))
    assert n.value == 3 * 4 * 130 * 3
    with pytest.raises(VaeHipError, match="changroup_workspace: bad args"):
        lib.call("vae_changroup_workspace", 0, 16, 8, 1, C.byref(n))
    with pytest.raises(VaeHipError, match="null args"):
        lib.call("vae_changroup_workspace", 1, 16, 8, 1, None)
    with pytest.raises(VaeHipError, match="empty chunk"):
        lib.call("vae_changroup_workspace", 1, 10, 8, 7, C.byref(n))  # chunks of 2 pixels: the last two of 7 are empty
    with pytest.raises(VaeHipError, match="2\\^31"):
        lib.call("vae_changroup_workspace", 32768, 65536, 8, 1, C.byref(n))
    # the launch entry points refuse on the host, before any launch (the pointers are never followed)
    p = C.c_void_p(4096)

    def partial(x=p, sc=None, sh=None, xf=0, B=2, HW=64, Cc=8, ld=8, nch=2, ws=p):
        lib.call("vae_changroup_partial", x, 0, sc, sh, xf, B, HW, Cc, ld, nch, ws, None)

    for kw, msg in [(dict(x=None), "null args"), (dict(ws=None), "null args"), (dict(ld=7), "pixel stride ld=7 below C=8"),
                    (dict(nch=33, HW=64), "empty chunk"), (dict(xf=1), "xf needs scale and shift"),
                    (dict(xf=2, sc=p), "xf needs scale and shift"), (dict(xf=3, sc=p, sh=p), "xf=3"),
                    (dict(ws=C.c_void_p(4096 + 8)), "unaligned workspace"), (dict(B=32768, HW=65536), "2\\^31"),
                    (dict(Cc=0), "bad args")]:
        with pytest.raises(VaeHipError, match="changroup_partial.*" + msg):
            partial(**kw)
    f64 = C.c_void_p(8192)
    for args, msg in [((None, 2, 64, 8, 2, f64), "null args"), ((p, 2, 64, 8, 2, None), "null args"),
                      ((C.c_void_p(4104), 2, 64, 8, 2, f64), "unaligned workspace"), ((p, 2, 64, 8, 33, f64), "empty chunk"),
                      ((p, 32768, 65536, 8, 1, f64), "2\\^31")]:
        with pytest.raises(VaeHipError, match="changroup_final.*" + msg):
            lib.call("vae_changroup_final", *args, None)
