"""Activation penalties without a GPU: the closed-form gradients of tests/actreg_refs.py against torch.autograd of the
definitions in float64, the spec and YAML validation, the chunk planner and the host-side refusals of the C ABI, registration
refusals on a CPU-built engine, and the input conditions of the engine-against-oracle test of tests/test_actreg_gpu.py,
checked on the float64 oracle alone."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import actreg_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- definitions
@pytest.mark.parametrize("channels", [None, (0, 3), (2,)])
@pytest.mark.parametrize("kind,thr,weight", [("ceiling", 0.5, 1.0), ("ceiling", 0.25, 3.0), ("floor", 0.3, 10.0), ("floor", 0.9, 0.5)])
def test_gradient_formulas_are_autograd_of_the_definitions(kind, thr, weight, channels):
    a, _ = R.draw((2, 5, 7, 6), 3)
    a[0, 0, 0, 1] = 0.0  # sign(0) = 0
    if kind == "floor":
        a[..., 2] *= 0.05  # under either floor, as channel 0 is
    a = a.double().requires_grad_(True)
    P = R.penalty(a, kind, thr, weight, channels)
    (0.5 * P).backward()  # grad_scale 0.5
    k, psi = R.grad_formula(a.detach().numpy(), kind, thr, weight, channels, grad_scale=0.5)
    want = k * psi
    assert np.abs(a.grad.numpy() - want).max() <= 1e-15 * max(np.abs(want).max(), 1e-30)
    assert np.abs(want).max() > 0
    if channels is not None:
        off = [c for c in range(6) if c not in channels]
        assert (a.grad.numpy()[..., off] == 0).all()
    # the reference of the statistics pass states the same value and coefficient (the fp32 thresholds here are exact or 1e-8 off)
    r = R.stats_ref(a.detach().float(), kind, thr, weight, channels, grad_scale=0.5)
    a32 = a.detach().float().double()
    assert abs(r["pen"].sum() - float(R.penalty(a32, kind, thr, weight, channels).detach())) <= 1e-6 * float(P.detach()) + 1e-12
    k32, _ = R.grad_formula(a32.numpy(), kind, thr, weight, channels, grad_scale=0.5)
    assert np.abs(r["coef"] - k32).max() <= 1e-6 * np.abs(k32).max()


def test_channel_dim_of_the_definition():
    a = torch.randn(2, 6, 5, 7, dtype=torch.float64)  # NCHW, as an oracle hook sees it
    for kind in R.KINDS:
        assert float(R.penalty(a, kind, 0.4, 2.0, (1, 2), channel_dim=1)) == float(R.penalty(a.permute(0, 2, 3, 1), kind, 0.4, 2.0, (1, 2)))


# ---------------------------------------------------------------------------------------------------- spec and YAML
def test_spec_validation_messages():
    from vaehip.actreg import ActivationPenalty, from_mapping
    s = ActivationPenalty("ceiling", 1, 2, [3, 1])
    assert (s.kind, s.threshold, s.weight, s.channels, s.kind_id) == ("ceiling", 1.0, 2.0, (3, 1), 0)
    assert ActivationPenalty("floor", 0.3).weight == 1.0 and ActivationPenalty("floor", 0.3).kind_id == 1
    with pytest.raises(Exception):
        s.weight = 3.0  # frozen
    for args, msg in [(("roof", 0.5, 1.0), "kind 'roof': expected one of ceiling, floor"),
                      (("ceiling", 0.0, 1.0), "threshold=0.0: must be > 0"), (("ceiling", -1.0, 1.0), "must be > 0"),
                      (("ceiling", float("inf"), 1.0), "threshold=inf: expected a finite number"),
                      (("ceiling", float("nan"), 1.0), "expected a finite number"), (("ceiling", "0.5", 1.0), "expected a finite number"),
                      (("ceiling", True, 1.0), "expected a finite number"),
                      (("floor", 0.3, -0.1), "weight=-0.1: must be >= 0"), (("floor", 0.3, float("inf")), "weight=inf: expected a finite number"),
                      (("floor", 0.3, 1.0, [1, 1]), "listed twice"), (("floor", 0.3, 1.0, [-1]), "negative"),
                      (("floor", 0.3, 1.0, [0.5]), "list of ints"), (("floor", 0.3, 1.0, []), "non-empty"),
                      (("floor", 0.3, 1.0, 3), "list of channel indices"), (("floor", 0.3, 1.0, [True]), "list of ints")]:
        with pytest.raises(ValueError, match=msg):
            ActivationPenalty(*args)
    assert ActivationPenalty("floor", 0.3, 0.0).weight == 0.0  # weight 0 is allowed
    with pytest.raises(ValueError, match=r"\[8\] out of range for a module with 8 output channels"):
        ActivationPenalty("floor", 0.3, 1.0, [0, 8]).check_channels(8)
    ActivationPenalty("floor", 0.3, 1.0, [0, 7]).check_channels(8)
    assert from_mapping({"kind": "floor", "threshold": 0.3, "channels": [0, 3]}) == ActivationPenalty("floor", 0.3, 1.0, (0, 3))
    with pytest.raises(ValueError, match="unknown keys \\['wieght'\\]"):
        from_mapping({"kind": "floor", "threshold": 0.3, "wieght": 2})
    with pytest.raises(ValueError, match="`threshold` is missing"):
        from_mapping({"kind": "floor"})


def test_yaml_section_parses_and_names_a_bad_entry():
    import yaml
    from train import activation_penalty_settings
    from vaehip.actreg import ActivationPenalty
    cfg = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_activation_penalty.yaml")))
    got = activation_penalty_settings(cfg)
    assert got == [("vae.decoder.up_blocks.1.resnets.0", ActivationPenalty("ceiling", 0.5, 1.0)),
                   ("vae.quant_conv", ActivationPenalty("floor", 0.3, 10.0, (0, 3)))]
    # ... with an output_grad tracker on a penalised layer
    tracked = {e["name"] for e in cfg["tracking"]["target_layers"] if e["capture_point"] == "output_grad"}
    assert {n for n, _ in got} <= tracked
    assert activation_penalty_settings({}) == [] and activation_penalty_settings({"activation_penalty": {"enabled": False, "targets": 3}}) == []
    assert activation_penalty_settings({"activation_penalty": {"enabled": True, "targets": [
        {"name": "vae.quant_conv", "kind": "floor", "threshold": "3e-1"}]}}) == [("vae.quant_conv", ActivationPenalty("floor", 0.3))]

    def bad(targets, msg):
        with pytest.raises(ValueError, match=msg):
            activation_penalty_settings({"activation_penalty": {"enabled": True, "targets": targets}})
    bad(None, "expected a non-empty list")
    bad([], "expected a non-empty list")
    bad(["vae.quant_conv"], r"targets\[0\]='vae.quant_conv': expected a mapping")
    bad([{"kind": "floor", "threshold": 0.3}], r"targets\[0\]: `name` is missing")
    ok = {"name": "vae.quant_conv", "kind": "floor", "threshold": 0.3}
    bad([ok, {"name": "vae.decoder", "kind": "lid", "threshold": 1}], r"targets\[1\] \(vae.decoder\): activation penalty kind 'lid'")
    bad([ok, {"name": "vae.decoder", "kind": "ceiling", "threshold": -1}], r"targets\[1\] \(vae.decoder\): threshold=-1.0: must be > 0")
    bad([{"name": "vae.decoder", "kind": "ceiling", "threshold": "high"}], r"\(vae.decoder\): threshold='high': expected a number")
    bad([{"name": "vae.decoder", "kind": "ceiling"}], r"\(vae.decoder\): `threshold` is missing")
    bad([dict(ok, channels=[0, 0])], r"targets\[0\] \(vae.quant_conv\): channels=\[0, 0\]: a channel is listed twice")
    bad([dict(ok, wait=2)], r"unknown keys \['wait'\]")


# ---------------------------------------------------------------------------------------------------- planner and C ABI
@pytest.mark.parametrize("Cc", [1, 3, 4, 8, 128, 256, 260, 512, 1024])
def test_chunk_rule_and_workspace_query(Cc):
    from vaehip import ops
    from vaehip.lib import lib
    for B, HW in [(1, 1), (1, 35), (2, 256), (3, 1023), (16, 65536), (32, 65536), (1, 1 << 20), (64, 17)]:
        nch = ops.actreg_chunks(B, HW, Cc)
        per = (HW + nch - 1) // nch
        assert nch >= 1 and (nch - 1) * per < HW <= nch * per  # every chunk non-empty, together they cover the image
        tiles = (Cc + 255) // 256
        pr = max(1, 256 // min(64, Cc // 4)) if Cc % 4 == 0 else max(1, 256 // min(256, Cc))  # pixel rows of a workgroup
        # workgroups near the target, never above it by choice, and no chunk below 16 pixels per pixel row unless it is the only one
        lim = max(1, min(ops._GN_TARGET // (B * tiles), HW // (16 * pr)))
        assert lim / 2 < nch <= lim and (nch == 1 or per >= 16 * pr)
        n = C.c_int64(0)
        lib.call("vae_actreg_workspace", B, HW, Cc, nch, C.byref(n))  # the library accepts the plan
        assert n.value == B * nch * Cc * 3


def test_refusals_need_no_gpu():
    """every entry point refuses on the host, before any launch (the pointers are never followed)"""
    from vaehip.lib import lib, VaeHipError
    n = C.c_int64(0)
    for args, msg in [((0, 64, 8, 1), "bad args"), ((2, 64, 0, 1), "bad args"), ((1, 10, 8, 7), "empty chunk"),
                      ((32768, 65536, 8, 1), "2\\^31")]:
        with pytest.raises(VaeHipError, match="actreg_workspace.*" + msg):
            lib.call("vae_actreg_workspace", *args, C.byref(n))
    with pytest.raises(VaeHipError, match="actreg_workspace: null args"):
        lib.call("vae_actreg_workspace", 1, 64, 8, 1, None)
    p = C.c_void_p(4096)

    def partial(a=p, lda=8, B=2, HW=64, Cc=8, nch=2, thr=0.5, ws=p):
        lib.call("vae_actreg_partial", a, 0, lda, B, HW, Cc, nch, thr, ws, None)

    for kw, msg in [(dict(a=None), "null args"), (dict(ws=None), "null args"), (dict(lda=7), "pixel stride lda=7 below C=8"),
                    (dict(nch=33), "empty chunk"), (dict(ws=C.c_void_p(4100)), "unaligned workspace"), (dict(thr=0.0), "threshold"),
                    (dict(thr=-1.0), "threshold"), (dict(thr=float("nan")), "threshold"), (dict(thr=float("inf")), "threshold"),
                    (dict(B=32768, HW=65536), "2\\^31"), (dict(Cc=0), "bad args")]:
        with pytest.raises(VaeHipError, match="actreg_partial.*" + msg):
            partial(**kw)

    def final(ws=p, B=2, HW=64, Cc=8, nch=2, kind=0, thr=0.5, weight=1.0, mask=None, gs=1.0, sums=p, pen=p, coef=p):
        lib.call("vae_actreg_final", ws, B, HW, Cc, nch, kind, thr, weight, mask, gs, sums, pen, coef, None)

    for kw, msg in [(dict(ws=None), "null args"), (dict(sums=None), "null args"), (dict(pen=None), "null args"), (dict(coef=None), "null args"),
                    (dict(kind=2), "kind=2"), (dict(kind=-1), "kind=-1"), (dict(thr=0.0), "threshold"), (dict(thr=float("nan")), "threshold"),
                    (dict(weight=-1.0), "weight"), (dict(weight=float("inf")), "weight"), (dict(weight=float("nan")), "weight"),
                    (dict(gs=float("nan")), "grad_scale"), (dict(gs=float("inf")), "grad_scale"),
                    (dict(ws=C.c_void_p(4100)), "unaligned workspace"), (dict(nch=33), "empty chunk")]:
        with pytest.raises(VaeHipError, match="actreg_final.*" + msg):
            final(**kw)

    def inject(a=p, lda=8, g=p, ldg=8, coef=p, rows=128, Cc=8, kind=0, thr=0.5, out=C.c_void_p(8192)):
        lib.call("vae_actreg_inject", a, 0, lda, g, 1, ldg, coef, rows, Cc, kind, thr, out, None)

    for kw, msg in [(dict(a=None), "null args"), (dict(g=None), "null args"), (dict(coef=None), "null args"), (dict(out=None), "null args"),
                    (dict(rows=0), "bad args"), (dict(rows=1 << 31), "bad args"), (dict(Cc=0), "bad args"), (dict(kind=3), "kind=3"),
                    (dict(thr=-0.5), "threshold"), (dict(thr=float("nan")), "threshold"), (dict(lda=7), "pixel stride"),
                    (dict(ldg=7), "pixel stride"), (dict(out=p), "out of place")]:
        with pytest.raises(VaeHipError, match="actreg_inject.*" + msg):
            inject(**kw)


def test_wrappers_refuse_before_the_library_is_asked():
    from vaehip import ops
    a = torch.zeros(2, 4, 4, 8)
    with pytest.raises(ValueError, match="kind 'lid' is not one of"):
        ops.actreg_stats(a, "lid", 0.5, 1.0)
    with pytest.raises(ValueError, match="threshold 0.0 is not a finite number > 0"):
        ops.actreg_stats(a, "floor", 0.0, 1.0)
    with pytest.raises(ValueError, match="actreg_stats: a: expected a 4-D NHWC fp32 / bf16 CUDA tensor"):
        ops.actreg_stats(a, "floor", 0.3, 1.0)
    with pytest.raises(ValueError, match="actreg_inject: a: expected a 4-D NHWC fp32 / bf16 CUDA tensor"):
        ops.actreg_inject(a, a, "floor", 0.3, torch.zeros(8))
    with pytest.raises(ValueError, match="kind"):
        ops.actreg_inject(a, a, "", 0.3, torch.zeros(8))


# ---------------------------------------------------------------------------------------------------- registration
def test_registration_refusals_on_a_cpu_engine():
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.actreg import ActivationPenalty
    from vaehip.trainer import HipTrainer
    w = SDXLVAEWrapper("synthetic:1")
    eng = w.vae.engine
    spec = ActivationPenalty("ceiling", 0.5)
    res = w.vae.decoder.up_blocks[1].resnets[0]
    with pytest.raises(ValueError, match="HipGroupNorm: the GroupNorm output is never materialised"):
        eng.add_activation_penalty(res.norm1, spec)
    with pytest.raises(ValueError, match="HipLinear: no 4-D capture point"):
        eng.add_activation_penalty(w.vae.decoder.mid_block.attentions[0].to_q, spec)
    with pytest.raises(ValueError, match="HipSiLU: no 4-D capture point"):
        eng.add_activation_penalty(res.nonlinearity, spec)
    with pytest.raises(TypeError, match="expected a vaehip.actreg.ActivationPenalty, got dict"):
        eng.add_activation_penalty(res, {"kind": "ceiling"})
    with pytest.raises(ValueError, match=r"\[8\] out of range for a module with 8 output channels"):
        eng.add_activation_penalty(w.vae.quant_conv, ActivationPenalty("floor", 0.3, 1.0, [8]))
    with pytest.raises(ValueError, match=r"\[3\] out of range for a module with 3 output channels"):
        eng.add_activation_penalty(w.vae.decoder, ActivationPenalty("floor", 0.3, 1.0, [3]))
    assert not eng._penalties
    # every kind of module add_grad_tracker accepts, with its output width
    for mod in (res, res.conv2, w.vae.quant_conv, w.vae.decoder.mid_block, w.vae.decoder.mid_block.attentions[0], w.vae.decoder.up_blocks[1],
                w.vae.decoder.up_blocks[1].upsamplers[0], w.vae.encoder.down_blocks[0].downsamplers[0], w.vae.encoder, w.vae.decoder):
        h = eng.add_activation_penalty(mod, spec)
        assert h.spec is spec and h.last is None and h.channels == eng._out_channels(mod)
        h.remove()
        h.remove()  # twice is harmless
    assert eng._out_channels(w.vae.decoder) == 3 and eng._out_channels(w.vae.encoder) == 8 and eng._out_channels(w.vae.quant_conv) == 8
    assert not eng._penalties
    # the trainer resolves names as tracking.target_layers names resolve, and names the entry it refuses
    for entries, msg in [([("vae.decoder.up_blocks.9", spec)], r"activation_penalties\[0\] \('vae.decoder.up_blocks.9'\): .*does not have a layer named"),
                         ([("vae.quant_conv", spec), ("vae.decoder.conv_norm_out", spec)],
                          r"activation_penalties\[1\] \('vae.decoder.conv_norm_out'\): HipGroupNorm"),
                         ([("vae.quant_conv", ActivationPenalty("floor", 0.3, 1.0, [9]))], r"\('vae.quant_conv'\): .*out of range"),
                         ([("vae.quant_conv", "floor")], r"\('vae.quant_conv'\): activation penalty: expected a vaehip.actreg")]:
        with pytest.raises(ValueError, match=msg):
            HipTrainer(w, activation_penalties=entries)
        assert not eng._penalties  # a refused list leaves nothing registered
    tr = HipTrainer(w, activation_penalties=[("vae.quant_conv", spec), ("decoder.mid_block", ActivationPenalty("floor", 0.3))])
    assert [n for n, _ in tr.activation_penalties] == ["vae.quant_conv", "decoder.mid_block"]
    assert tr.activation_penalties[1][1].module is w.vae.decoder.mid_block and len(eng._penalties) == 2


# ---------------------------------------------------------------------------------------------------- the oracle's inputs
@pytest.fixture(scope="module")
def oracle_runs():
    return R.oracle_pass(R.ENGINE_TARGETS), R.oracle_pass([])


def test_input_conditions_of_the_engine_test_hold_on_the_oracle(oracle_runs):
    """what makes the engine-against-oracle comparison of tests/test_actreg_gpu.py a test: every penalty is active, none is
    saturated, and together they move the gradient"""
    on, off = oracle_runs
    for n in R.CEILING_TARGETS:
        share, _, C_ = on["stats"][n]
        print(f"{n}: {100 * share:.1f} % of the elements over 0.5, penalty {on['terms'][n]:.4e}")
        assert 0.05 <= share <= 0.95, (n, share)
    for n in R.FLOOR_TARGETS:
        _, under, C_ = on["stats"][n]
        print(f"{n}: {under} of {C_} channels under 0.3, penalty {on['terms'][n]:.4e}")
        assert 1 <= under < C_, (n, under, C_)
    assert all(v > 0 for v in on["terms"].values()) and abs(sum(on["terms"].values()) - on["penalty"]) <= 1e-12 * on["penalty"]
    assert off["penalty"] == 0.0 and abs(on["total"] - off["total"] - on["penalty"]) <= 1e-12 * on["total"]
    num = sum(float(((on["grads"][k] - off["grads"][k]) ** 2).sum()) for k in off["grads"])
    den = sum(float((off["grads"][k] ** 2).sum()) for k in off["grads"])
    rel = (num / den) ** 0.5
    print(f"relative gradient change {rel:.3f}")
    assert rel >= 0.1, rel
