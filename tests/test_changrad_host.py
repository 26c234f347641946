"""The gradient metrics of the capture point `output_grad` on the host: the hook path's formulas
(tracking.monitor.compute_grad_metrics) against tests/changrad_refs.py, the hook path end to end on a plain torch module on the
CPU (two backward passes, step(), log keys, record kinds), the routing of engine modules and of the new config, and the
library's workspace query, chunk rule and argument refusals.  Nothing here touches a device."""
import ctypes as C
import logging
import os

import numpy as np
import pytest
import torch

import changrad_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_channel_grad.yaml")
MEAN, AMAX, GAIN, SAL = ("mean_abs_gradient_per_channel", "abs_max_gradient_per_channel", "gain_gradient_per_channel",
                         "taylor_saliency_per_channel")
FOUR = [MEAN, AMAX, GAIN, SAL]
FUSED = "mean_abs_activation_per_channel"


# ------------------------------------------------------------------------------------------------ formulas
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 7, 13, 5), (2, 4, 4, 8)])
def test_compute_grad_metrics_against_the_float64_reference(shape, dt):
    from tracking.monitor import compute_grad_metrics
    a, g = (t.to(dt) for t in R.draw(shape, 3 + shape[-1]))
    sums, amax = compute_grad_metrics(a.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2))  # the hook sees NCHW
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (3, shape[-1]) and amax.dtype == torch.float32
    r = R.ref(a.float() if dt != torch.float64 else a, g.float() if dt != torch.float64 else g)
    if dt != torch.float64:  # the same float64 sums of the same exact products, in another order
        assert np.allclose(sums.numpy(), r["sums"], rtol=1e-12, atol=0)
        assert R.same_bits(amax.numpy(), r["absmax"])
        R.check(sums, amax, a, g, per=1)  # and so inside the tightest kernel bound
    else:
        assert np.allclose(sums.numpy(), r["sums"], rtol=1e-6, atol=1e-9)


def test_known_answers():
    from tracking.monitor import compute_grad_metrics
    # two images, two channels, two pixels: channel 0 flips its sign between the images, channel 1 gets no gradient
    a = torch.tensor([[[1.0, 2.0], [5.0, 5.0]], [[1.0, 2.0], [7.0, 7.0]]])        # [B, C, P]
    g = torch.tensor([[[0.5, -0.25], [0.0, 0.0]], [[-0.5, 0.25], [0.0, -0.0]]])
    sums, amax = compute_grad_metrics(a, g)
    assert sums[:, 0].tolist() == [0.375, 0.0, 0.0] and amax.tolist() == [0.5, 0.0]  # P = [0.5 - 0.5, ...] = 0 per image
    sums, amax = compute_grad_metrics(a, g.abs())
    assert sums[:, 0].tolist() == [0.375, 2.0, 1.0] and sums[:, 1].tolist() == [0.0, 0.0, 0.0]
    sums, _ = compute_grad_metrics(a, g.abs() * torch.tensor([1.0, -1.0]).view(2, 1, 1))   # P = [1, -1]: gain 0, saliency 1
    assert sums[:, 0].tolist() == [0.375, 0.0, 1.0]
    # NaN and inf stay in their channel; a tensor without a channel axis is one channel of one image
    g2 = g.clone()
    g2[0, 1, 0] = float("nan")
    g2[1, 0, 1] = float("-inf")
    _, amax = compute_grad_metrics(a, g2)
    assert np.isposinf(amax[0].item()) and np.isnan(amax[1].item())
    sums, amax = compute_grad_metrics(torch.tensor([1.0, -2.0, 3.0]), torch.tensor([0.5, 0.5, -1.0]))
    assert sums[:, 0].tolist() == [2.0 / 3.0, -3.5, 3.5] and amax.tolist() == [1.0]
    with pytest.raises(ValueError, match="differ"):
        compute_grad_metrics(a, g[:, :1])


# ------------------------------------------------------------------------------------------------ the hook path end to end
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.conv = torch.nn.Conv2d(3, 6, 3, padding=1)
        self.act = torch.nn.Tanh()
        self.head = torch.nn.Conv2d(6, 2, 1)

    def forward(self, x):
        return self.head(self.act(self.conv(x)))


def test_hook_path_two_backward_passes_step_and_records():
    from tracking.monitor import ActivityMonitor
    net = _Net()
    mon = ActivityMonitor(net, {"enabled": True, "track_interval": 1, "zero_gradient_threshold": 1e-3, "target_layers": [
        {"name": "act", "capture_point": "output_grad", "metrics": list(FOUR)},
        {"name": "act", "capture_point": "output", "metrics": [FUSED]},
        {"name": "conv", "capture_point": "output_grad"}]})  # no metrics: all four
    assert mon.device_layers == [] and len(mon.hooks) == 3
    kept = {}

    def keep(m, i, out):
        if out.requires_grad:
            out.retain_grad()
            kept.setdefault("out", []).append(out)
    net.act.register_forward_hook(keep)
    xs = [torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(s)) for s in (1, 2)]
    for i, x in enumerate(xs):
        (net(x).square().sum() * (0.5 if i else 1.0)).backward()  # (the factor: a micro-batch of an accumulated update)
    with torch.no_grad():
        net(xs[0])  # an eval forward buffers nothing for output_grad
    buf = mon.hook_collected_buffer
    assert {k: len(v) for k, v in buf["act.output_grad"].items()} == dict.fromkeys(FOUR, 2)
    assert list(buf["conv.output_grad"]) == FOUR and len(buf["act.output"][FUSED]) == 3
    log = mon.step(1)
    data = mon.get_data_for_step(1)
    assert not mon.hook_collected_buffer
    # each pass against the float64 reference of the output and gradient autograd kept (NCHW -> NHWC), then step()'s rule
    refs = [R.ref(o.detach().permute(0, 2, 3, 1), o.grad.permute(0, 2, 3, 1)) for o in kept["out"][:2]]
    got = data["act.output_grad"]
    assert list(got) == FOUR and all(got[m].dtype == np.float32 and got[m].shape == (6,) for m in FOUR)
    for m, row in ((MEAN, 0), (GAIN, 1), (SAL, 2)):
        want = np.mean(np.stack([r["sums"][row].astype(np.float32) for r in refs]), axis=0)  # unweighted mean over the passes
        assert np.allclose(got[m], want, rtol=1e-6, atol=0), m
    assert np.array_equal(got[AMAX], np.max(np.stack([r["absmax"] for r in refs]), axis=0))
    assert (got[SAL] >= np.abs(got[GAIN]) / 2 - 1e-6).all() and (got[AMAX] >= got[MEAN]).all()
    base = "tracking/act.output_grad/"
    want_keys = {base + MEAN + "_overall_mean", base + MEAN + "_overall_max", base + SAL + "_overall_mean", base + SAL + "_overall_max",
                 base + AMAX + "_overall_max", base + GAIN + "_overall_mean"}
    assert {k for k in log if k.startswith(base)} == want_keys
    assert log[base + AMAX + "_overall_max"] == got[AMAX].max() and log[base + GAIN + "_overall_mean"] == got[GAIN].mean()
    assert len([k for k in log if k.startswith("tracking/conv.output_grad/")]) == 6
    recs = [r for r in mon.export_all_processed_data_to_records() if r["layer_identifier"] == "act.output_grad"]
    kinds = {(r["original_metric_name"], r["metric_type"]): r["metric_value"] for r in recs}
    want_kinds = [(m, m[:-len("_per_channel")] + k) for m in FOUR for k in ("_overall_mean", "_overall_min", "_overall_max")]
    want_kinds += [(MEAN, "mean_abs_gradient_zero_channels"), (SAL, "taylor_saliency_argmax_channel")]
    assert sorted(kinds) == sorted(want_kinds)
    assert kinds[(SAL, "taylor_saliency_argmax_channel")] == int(got[SAL].argmax())
    assert kinds[(MEAN, "mean_abs_gradient_zero_channels")] == int((got[MEAN] <= 1e-3).sum())
    assert kinds[(GAIN, "gain_gradient_overall_min")] == float(got[GAIN].min())
    # a NaN gradient: the maximum stays NaN through step()
    x = xs[0]
    out = net(x)
    (out.sum() * float("nan")).backward()
    net(x).sum().backward()
    mon.step(2)
    assert np.isnan(mon.get_data_for_step(2)["act.output_grad"][AMAX]).all()
    # remove_hooks() removes the forward hook and silences a tensor hook already placed
    y = net(x)
    mon.remove_hooks()
    y.sum().backward()
    net(x).sum().backward()
    assert not any(k.endswith(".output_grad") for k in mon.hook_collected_buffer) and mon.hooks == []
    assert len(net.act._forward_hooks) == 1 and not net.conv._forward_hooks  # the test's own


def test_zero_gradient_threshold_default_counts_exact_zeros():
    from tracking.monitor import ActivityMonitor
    net = _Net()
    mon = ActivityMonitor(net, {"enabled": True, "track_interval": 1,
                                "target_layers": [{"name": "act", "capture_point": "output_grad", "metrics": [MEAN]}]})
    assert mon.zero_gradient_threshold == 0.0
    with torch.no_grad():
        net.head.weight[:, 4] = 0.0  # channel 4 of act's output reaches nothing
    net(torch.randn(2, 3, 4, 4)).sum().backward()
    mon.step(1)
    recs = {r["metric_type"]: r["metric_value"] for r in mon.export_all_processed_data_to_records()}
    assert recs["mean_abs_gradient_zero_channels"] == 1 and recs["mean_abs_gradient_overall_min"] == 0.0
    mon.remove_hooks()


def test_existing_metric_tuples_are_unchanged():
    from tracking import monitor as M
    from vaehip import engine as E
    assert M.KNOWN_METRICS == (FUSED, "full_activation_map", "mean_activation", "std_activation", "log2_histogram_per_channel",
                               "abs_max_activation_per_channel", "near_zero_fraction_per_channel")
    assert M.CHANCOV_METRICS == E.CHANCOV_METRICS == ("channel_covariance_matrix", "channel_correlation_matrix",
                                                      "max_abs_correlation_per_channel", "effective_rank")
    assert E.DEVICE_METRICS == E.MOMENT_METRICS + E.CHANHIST_METRICS + E.CHANCOV_METRICS + ("full_activation_map",)
    assert M.CHANGRAD_METRICS == E.CHANGRAD_METRICS == tuple(FOUR)
    assert not set(FOUR) & set(M.KNOWN_METRICS + M.CHANCOV_METRICS + E.DEVICE_METRICS)


# ------------------------------------------------------------------------------------------------ routing
def test_engine_targets_route_to_gradient_trackers(caplog):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    w = SDXLVAEWrapper("synthetic:1")
    eng = w.vae.engine
    res = "vae.decoder.up_blocks.1.resnets.0"
    good = [res, res + ".conv1", "vae.decoder.up_blocks.1.upsamplers.0", "vae.decoder", "vae.quant_conv", "vae.encoder.mid_block"]
    targets = [{"name": n, "capture_point": "output_grad", "metrics": list(FOUR)} for n in good]
    targets += [{"name": res + ".norm1", "capture_point": "output_grad", "metrics": [MEAN]},          # a GroupNorm: refused
                {"name": res, "capture_point": "output", "metrics": [GAIN]},                          # a gradient metric on output
                {"name": res, "capture_point": "input", "metrics": [FUSED, SAL]},                     # ... on input
                {"name": res, "capture_point": "output_grad", "metrics": [FUSED]},                    # a forward metric on output_grad
                {"name": res, "capture_point": "output_grad", "metrics": [MEAN, "no_such_metric"]},
                {"name": res, "capture_point": "output_gradient", "metrics": [MEAN]}]                 # unknown capture point
    for device_metrics in (False, True):  # no torch hook could serve them: routed to the engine either way
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            mon = ActivityMonitor(w, {"enabled": True, "track_interval": 1, "device_metrics": device_metrics, "target_layers": targets})
        try:
            assert mon.device_layers == [n + ".output_grad" for n in good] and mon.fused_layers == []
            assert sorted(n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks) == []
            assert sum(len(d["output_grad"]) for d in eng._gtrackers.values()) == len(good)
            errors = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
            assert len(errors) == 5 and sum("never materialised" in e for e in errors) == 1
            assert sum("need capture_point 'output_grad'" in e for e in errors) == 2
            assert sum("serves" in e and "Skipping" in e for e in errors) == 2
            assert any("Unknown capture_point 'output_gradient'" in r.getMessage() for r in caplog.records)
        finally:
            mon.remove_hooks()
        assert not any(d.get("output_grad") for d in eng._gtrackers.values()) and mon.device_layers == []
    with pytest.raises(ValueError, match="GroupNorm output is never materialised"):
        eng.add_grad_tracker(w.vae.decoder.conv_norm_out, lambda s, m: None, [MEAN])
    with pytest.raises(ValueError, match="gradient trackers serve"):
        eng.add_grad_tracker(w.vae.decoder, lambda s, m: None, [FUSED])
    with pytest.raises(ValueError, match="no 4-D capture point"):
        eng.add_grad_tracker(w.vae.decoder.mid_block.attentions[0].to_q, lambda s, m: None, [MEAN])
    with pytest.raises(ValueError, match="device trackers serve"):  # add_tracker is what it was
        eng.add_tracker(w.vae.decoder, "output", lambda *a: None, metrics=[MEAN])


def test_new_config_parses_and_routes():
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from utils.config_utils import load_config
    c = load_config(CFG)
    t = c["tracking"]
    assert float(t["zero_gradient_threshold"]) == 0.0
    grad = [e["name"] for e in t["target_layers"] if e["capture_point"] == "output_grad"]
    assert grad == ["vae.decoder.up_blocks.1.resnets.0", "vae.decoder.up_blocks.1.resnets.0.conv1",
                    "vae.decoder.up_blocks.1.upsamplers.0", "vae.decoder", "vae.quant_conv"]
    assert all(e["metrics"] == FOUR for e in t["target_layers"] if e["capture_point"] == "output_grad")
    fwd = [e["name"] for e in t["target_layers"] if e["capture_point"] == "output"]
    assert set(grad) <= set(fwd)  # a forward metric next to each of them
    w = SDXLVAEWrapper("synthetic:1")
    mon = ActivityMonitor(w, t)
    try:
        assert [lid for lid in mon.device_layers if lid.endswith(".output_grad")] == [n + ".output_grad" for n in grad]
        assert sorted(n for n, m in w.named_modules() if m._forward_hooks or m._forward_pre_hooks) == []
    finally:
        mon.remove_hooks()


# ------------------------------------------------------------------------------------------------ library, no GPU
def test_wrapper_refuses_before_the_library_is_asked():
    from vaehip import ops
    with pytest.raises(ValueError, match="CUDA tensors"):  # CPU tensors: no fallback
        ops.changrad(torch.zeros(1, 4, 4, 8), torch.zeros(1, 4, 4, 8))


@pytest.mark.parametrize("Cc", [1, 3, 4, 8, 128, 256, 257, 512, 1024])
def test_chunk_rule_and_workspace_query(Cc):
    from vaehip import ops
    from vaehip.lib import lib
    n = C.c_int64(0)
    for B, HW in [(1, 1), (1, 91), (3, 91), (3, 256), (1, 768), (2, 1024), (16, 65536), (32, 65536), (1, 1 << 20), (64, 17)]:
        nch = ops.changrad_chunks(B, HW, Cc)
        per = (HW + nch - 1) // nch
        assert nch >= 1 and (nch - 1) * per < HW <= nch * per  # every chunk non-empty, together they cover the image
        tiles = (Cc + 255) // 256
        pr = max(1, 256 // min(64, Cc // 4)) if Cc % 4 == 0 else max(1, 256 // min(256, Cc))  # pixel rows of a workgroup
        # workgroups near the target, never above it by choice, and no chunk below 16 pixels per pixel row unless it is the only one
        lim = max(1, min(ops._GN_TARGET // (B * tiles), HW // (16 * pr)))
        assert lim / 2 < nch <= lim and (nch == 1 or per >= 16 * pr)
        lib.call("vae_changrad_workspace", B, HW, Cc, nch, C.byref(n))  # the library accepts what the rule gives
        assert n.value == B * nch * Cc * 3  # per (channel, image, chunk): sum |g|, sum a g, the largest |g| pattern


def test_workspace_query_and_refusals_need_no_gpu():
    from vaehip.lib import lib, VaeHipError
    n = C.c_int64(0)
    with pytest.raises(VaeHipError, match="changrad_workspace: bad args"):
        lib.call("vae_changrad_workspace", 0, 16, 8, 1, C.byref(n))
    with pytest.raises(VaeHipError, match="null args"):
        lib.call("vae_changrad_workspace", 1, 16, 8, 1, None)
    with pytest.raises(VaeHipError, match="empty chunk"):
        lib.call("vae_changrad_workspace", 1, 10, 8, 7, C.byref(n))  # chunks of 2 pixels: the last two of 7 are empty
    with pytest.raises(VaeHipError, match="2\\^31"):
        lib.call("vae_changrad_workspace", 32768, 65536, 8, 1, C.byref(n))
    lib.call("vae_changrad_workspace", 32767, 65536, 8, 1, C.byref(n))
    assert n.value == 32767 * 8 * 3
    # the launch entry points refuse on the host, before any launch (the pointers are never followed)
    p = C.c_void_p(4096)

    def partial(a=p, g=p, lda=8, ldg=8, B=2, HW=64, Cc=8, nch=2, ws=p):
        lib.call("vae_changrad_partial", a, 0, lda, g, 1, ldg, B, HW, Cc, nch, ws, None)

    for kw, msg in [(dict(a=None), "null args"), (dict(g=None), "null args"), (dict(ws=None), "null args"),
                    (dict(lda=7), "pixel stride lda=7 or ldg=8 below C=8"), (dict(ldg=7), "pixel stride lda=8 or ldg=7 below C=8"),
                    (dict(nch=33, HW=64), "empty chunk"), (dict(ws=C.c_void_p(4096 + 8)), "unaligned workspace"),
                    (dict(B=32768, HW=65536), "2\\^31"), (dict(Cc=0), "bad args")]:
        with pytest.raises(VaeHipError, match="changrad_partial.*" + msg):
            partial(**kw)
    out = C.c_void_p(8192)
    for args, msg in [((None, 2, 64, 8, 2, out, out), "null args"), ((p, 2, 64, 8, 2, None, out), "null args"),
                      ((p, 2, 64, 8, 2, out, None), "null args"), ((C.c_void_p(4100), 2, 64, 8, 2, out, out), "unaligned workspace"),
                      ((p, 2, 64, 8, 33, out, out), "empty chunk"), ((p, 32768, 65536, 8, 1, out, out), "2\\^31")]:
        with pytest.raises(VaeHipError, match="changrad_final.*" + msg):
            lib.call("vae_changrad_final", *args, None)
