"""tracking.device_metrics on the host: the key parses, the default routes exactly as before, and with the key set an engine
target with a 4-D capture point and any subset of the four metrics is device-served (no torch hook)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_all_metrics.yaml")
FUSED = "mean_abs_activation_per_channel"


@pytest.fixture(scope="module")
def wrapper():
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    return SDXLVAEWrapper("synthetic:1")


def _hooked(model):
    return sorted(n for n, m in model.named_modules() if m._forward_hooks or m._forward_pre_hooks)


def _targets():
    return [{"name": "vae.encoder.conv_in", "capture_point": "output", "metrics": [FUSED]},
            {"name": "vae.encoder.down_blocks.0.resnets.0.norm1", "capture_point": "output",
             "metrics": [FUSED, "full_activation_map"]},
            {"name": "vae.encoder", "capture_point": "input", "metrics": ["mean_activation", "std_activation"]},
            {"name": "vae.decoder.mid_block.attentions.0.to_q", "capture_point": "output", "metrics": ["mean_activation"]}]


def test_config_key_parses():
    from utils.config_utils import load_config
    c = load_config(CFG)
    assert c["tracking"]["device_metrics"] is True
    metrics = {(t["name"], t["capture_point"]): t["metrics"] for t in c["tracking"]["target_layers"]}
    assert metrics[("vae.encoder.down_blocks.0.resnets.0.norm1", "input")] == ["full_activation_map"]
    assert metrics[("vae.decoder.conv_norm_out", "input")] == ["mean_activation", "std_activation"]


def test_default_routes_as_before(wrapper):
    from tracking.monitor import ActivityMonitor
    for extra in ({}, {"device_metrics": False}):
        mon = ActivityMonitor(wrapper, {"enabled": True, "target_layers": _targets(), **extra})
        try:
            assert mon.fused_layers == ["vae.encoder.conv_in.output"]
            assert mon.device_layers == []
            assert _hooked(wrapper) == ["vae.decoder.mid_block.attentions.0.to_q", "vae.encoder",
                                        "vae.encoder.down_blocks.0.resnets.0.norm1"]
        finally:
            mon.remove_hooks()
    assert _hooked(wrapper) == []


def test_device_metrics_route_to_the_engine(wrapper):
    from tracking.monitor import ActivityMonitor
    mon = ActivityMonitor(wrapper, {"enabled": True, "device_metrics": True, "target_layers": _targets()})
    try:
        assert mon.fused_layers == ["vae.encoder.conv_in.output"]
        assert mon.device_layers == ["vae.encoder.down_blocks.0.resnets.0.norm1.output", "vae.encoder.input"]
        assert _hooked(wrapper) == ["vae.decoder.mid_block.attentions.0.to_q"]  # a Linear capture point stays on hooks
        eng = wrapper.vae.engine
        norm1 = wrapper.vae.encoder.down_blocks[0].resnets[0].norm1
        assert len(eng._mtrackers[id(norm1)]["output"]) == 1
    finally:
        mon.remove_hooks()
    assert _hooked(wrapper) == []
    assert all(not lst for d in wrapper.vae.engine._mtrackers.values() for lst in d.values())


def test_engine_refuses_what_it_cannot_serve(wrapper):
    eng = wrapper.vae.engine
    with pytest.raises(ValueError):
        eng.add_tracker(wrapper.vae.decoder.mid_block.attentions[0].to_q, "output", lambda m, f: None, metrics=["mean_activation"])
    with pytest.raises(ValueError):
        eng.add_tracker(wrapper.vae.encoder, "input", lambda m, f: None, metrics=["histogram"])
