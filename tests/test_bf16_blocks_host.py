"""The criterion of tests/test_bf16_blocks_gpu.py has power and is not too tight, shown from the reference alone (no GPU).

Not too tight: every small case of tests/bf16_refs.py is evaluated a second time with every product accumulated in fp32 in
torch's CPU order on the same rounded operands -- a correct engine with another summation order -- and the float64 reference,
continued from that evaluation's stored values, accepts every stage and every element.

Power: each single mistake of MUTANTS (one rounding point of the reference switched off or moved) is applied to such an
evaluation; the true reference must find a stage that violates the criterion by at least 2x.  A mutant that is not rejected by
that margin is named in UNDETECTED; where a regime has no such rounding point (fp32 storage rounds no conv output), the mutant's
record must be bit-identical to the unmutated one (NOT_THERE), which is asserted, not assumed.

Arms: the engine's own block runs without a GPU (the library answers every dispatch query, nothing is launched), and the kernel
names of its launches must be the ones the case pins -- the tile counts and divisibility rules of an arm are the library's, not a
copy of them -- and the sequence of its ops-level calls must be the reference's wiring."""
import math

import pytest
import torch
import torch.nn.functional as F

import bf16_refs as br


@pytest.fixture(scope="module")
def vae():
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    w = SDXLVAEWrapper("synthetic:5")
    restore = br.contrast(w.vae)
    yield w.vae
    restore()


def _ops():
    from vaehip import ops
    return ops


def _setup(case, vae):
    ops = _ops()
    P, _ = br.params_of(case, vae)
    x_pre, x, dout = br.inputs_of(case, vae, ops)
    return br.cfg_of(case, vae, ops), P, x_pre, x, dout


def _stand_in(case, vae, **kw):
    cfg, P, x_pre, x, dout = _setup(case, vae)
    E = br.Ev(acc=torch.float32, **kw)
    br.reference(E, case, cfg, P, x_pre, x, dout)
    return E.record


def _judge(case, vae, record):
    cfg, P, x_pre, x, dout = _setup(case, vae)
    E = br.Ev(forced=record)
    br.reference(E, case, cfg, P, x_pre, x, dout)
    return br.worst(E.stages)


# ---------------------------------------------------------------------------------------------------- the pieces
def test_r16_is_torch_bfloat16_and_ulp_is_the_spacing():
    t = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3
    assert torch.equal(br.r16(t), t.bfloat16()) and torch.equal(br.r16(t.double()), t.bfloat16())
    for v, u in ((1.0, 2.0 ** -7), (1.5, 2.0 ** -7), (2.0, 2.0 ** -6), (0.75, 2.0 ** -8), (-3.0, 2.0 ** -6), (0.0, 2.0 ** -133), (1e-40, 2.0 ** -133)):
        assert float(br.ulp_bf16(torch.tensor(v))) == u, v
    # the spacing of bf16 around a value IS ulp_bf16: the next representable number is one ulp away
    b = torch.tensor([1.0, 2.5, 100.0]).bfloat16()
    nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - b.double()), br.ulp_bf16(b.double()))


def test_criterion_accepts_one_rounding_and_rejects_two():
    v = torch.randn(50000, generator=torch.Generator().manual_seed(1)).double()
    once = br.Stage("s", "op", v, br.r16(v), "bf16", 0.0, None)
    assert br.ratio(once) <= 1.0
    off = br.Stage("s", "op", v, (br.r16(v).view(torch.int16) + 1).view(torch.bfloat16), "bf16", 0.0, None)
    assert br.ratio(off) >= 2.0 - 2.0 ** -7
    img = br.Stage("i", "op", None, br.r16(v), "image", 0.0, v.float())
    assert br.ratio(img) == 0.0 and br.ratio(img._replace(got=br.r16(v.flip(0)))) == math.inf


def test_phase_kernels_are_the_upsampled_convolution():
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(2, 5, 4, 6, generator=g).double(), torch.randn(7, 5, 3, 3, generator=g).double()
    a = br.phase_conv_nchw(x, br.phase_weights(w))
    b = br.conv_nchw(x, w, "c3up")
    assert float((a - b).abs().max()) < 1e-12


def test_groupnorm_restatement_is_autograd_in_float64():
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(2, 4, 6, 64, generator=g) * 1.3 + 0.2, torch.randn(2, 4, 6, 64, generator=g)
    ga, be, add = 1 + 0.3 * torch.randn(64, generator=g), 0.2 * torch.randn(64, generator=g), torch.randn(2, 4, 6, 64, generator=g)
    E = br.Ev()
    st = E.gn_stats("st", x, ga, be)
    a = E.gn_apply_bf16("a", x, st, br.XF_AFFINE_SILU)
    dx, _, dga, dbe = E.gn_bwd("n", x, dy, st, ga, be, True, add, True, False)
    xr, gr, br_ = (t.double().requires_grad_(True) for t in (x, ga, be))
    y = F.silu(F.group_norm(xr.permute(0, 3, 1, 2), 32, gr, br_, br.EPS)).permute(0, 2, 3, 1)
    y.backward(dy.double())
    rel = lambda p, q: float((p.double() - q).abs().max() / q.abs().max())  # noqa: E731
    assert rel(dx, xr.grad + add.double()) < 1e-5 and rel(dga, gr.grad) < 1e-5 and rel(dbe, br_.grad) < 1e-5
    assert br.ratio(br.Stage("a", "", y.detach(), a, "bf16", br.BAR_GN_APPLY, None)) <= 1.0


# ---------------------------------------------------------------------------------------------------- arms
@pytest.mark.parametrize("case", br.CASES, ids=[c.id for c in br.CASES])
def test_case_takes_its_arm_and_the_references_wiring(case, vae):
    from vaehip.lib import lib
    ops = _ops()
    names, seq = br.dry_run(case, vae, ops, lib)
    assert names == case.names, (case.id, names)
    cfg = br.cfg_of(case, vae, ops)
    if case.block == "resnet":
        halo = "flat" not in case.arm
        assert (cfg.img1, cfg.img2, cfg.gimg1, cfg.gimg2) == (halo,) * 4, cfg
    if case.small:
        want = [e["op"] for e in _stand_in(case, vae) if e["op"] != "fused"]
        assert seq == want, (case.id, seq, want)


def test_every_issue_arm_has_its_case():
    by = br.BY_ID
    wide = lambda c: sum(n.startswith("conv3_wide_bf16") for n in c.names)  # noqa: E731
    assert wide(by["resnet-wide-128"]) == 3 and by["resnet-wide-128"].names[1].startswith("conv3_tile_bf16")
    assert wide(by["resnet-wide-256"]) == 4 and wide(by["up-13"]) == 8 and wide(by["up-7"]) == 1 and wide(by["up-halo"]) == 0
    assert by["up-halo-f32store"].names.count("conv3_tile_bf16_kernel<false,false,0,false>") == 4
    regimes = {(c.act16, c.after_conv3, c.live_in) for c in br.CASES if c.block == "resnet"}
    assert {a for a, _, _ in regimes} == {True, False} and {b for _, b, _ in regimes} == {True, False} and {l for _, _, l in regimes} == {True, False}
    assert {c.block for c in br.CASES} >= {"resnet", "up", "down", "tail", "conv"}
    for c in br.CASES:   # the wide cases keep the tile count their arm needs: B (H / 8) (W / 32) ceil(C / 128) >= 192
        if "wide" in c.id or c.id == "up-13":
            B, H, W = c.shape
            assert B * (H // 8) * (W // 32) * (2 if ("256" in c.id or c.block == "up") else 1) >= 192, c.id


# ---------------------------------------------------------------------------------------------------- not too tight
SMALL = [c for c in br.CASES if c.small]


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_fp32_sums_in_another_order_pass_everywhere(case, vae):
    ratios = _judge(case, vae, _stand_in(case, vae))
    over = {k: v for k, v in ratios.items() if v > 1.0}
    print(case.id, "worst", max(ratios.items(), key=lambda kv: kv[1]))
    assert not over, over


# ---------------------------------------------------------------------------------------------------- power
A, B_ = "resnet-halo-128", "resnet-halo-128-256"
MUTANTS = {   # name: (number in the issue, Ev keyword arguments, case, what the mistake is)
    "conv_reads_unrounded_activation": (1, dict(off={"act"}), A, "conv forward reads the unrounded activation"),
    "conv_reads_unrounded_weights": (2, dict(off={"weight"}), A, "conv reads unrounded weights"),
    "wgrad_reads_fp32_activation": (3, dict(off={"wgrad_act"}), A, "wgrad reads the fp32 transformed tensor instead of the image"),
    "h_rounded_before_bias": (4, dict(moved={"out_store": "bias_late"}), A, "h rounded before the bias is added"),
    "residual_after_rounding": (5, dict(moved={"out_store": "res_late"}), A, "the residual added after the rounding"),
    "stats_of_unrounded_h": (6, dict(off={"stats_stored"}), A, "norm2's statistics from the unrounded h"),
    "g2_unrounded_into_gn_bwd": (7, dict(off={"dgrad_store"}), A, "conv2's input gradient kept unrounded into the GroupNorm backward"),
    "gradient_rounded_twice": (8, dict(moved={"gnbwd_store": "twice"}), A, "rounded, added to the residual-path gradient, rounded again"),
    "dh_as_fp32_into_conv1": (9, dict(off={"dh_operand"}), A, "dL/dh handed to conv1 as fp32 where the engine hands over the image"),
    "stale_gradient_image": (10, dict(moved={"grad_image": "stale"}), A, "the image of dout of the other sample"),
    "shortcut_reads_fp32_x": (11, dict(off={"x_store"}), B_, "the shortcut reads fp32 x where the engine reads the stored / rounded x"),
    "phase_weights_per_tap": (12, dict(moved={"phase_weights": "per_tap"}), "up-halo", "phase weights rounded tap by tap"),
}
# a mutant the true reference does not reject by 2x: {(name, regime): why the arithmetic cannot tell the two apart}.  At most 2.
UNDETECTED = {}
# the regime has no such rounding point: the mutant changes nothing there (its record is asserted bit-identical)
NOT_THERE = {
    ("h_rounded_before_bias", "f32store"): "fp32 storage rounds no conv output",
    ("residual_after_rounding", "f32store"): "fp32 storage rounds no conv output",
    ("stats_of_unrounded_h", "f32store"): "h is stored as fp32: the statistics of the stored tensor are those of the unrounded one",
    ("phase_weights_per_tap", "act16"): "with bf16 storage the small upsampler runs no phase convolution forward or in its dgrad (the phases "
                                        "need 192 wide tiles there: up-13, which the GPU module runs)",
}


def _same(r0, r1):
    return len(r0) == len(r1) and all(a["op"] == b["op"] and all(torch.equal(p, q) for p, q in zip(a["out"], b["out"])) for a, b in zip(r0, r1))


@pytest.mark.parametrize("regime", ["act16", "f32store"])
@pytest.mark.parametrize("name", list(MUTANTS))
def test_single_mistake_is_rejected(name, regime, vae):
    _, kw, cid, what = MUTANTS[name]
    case = br.BY_ID[cid if regime == "act16" else cid + "-f32store"]
    rec = _stand_in(case, vae, **kw)
    if (name, regime) in NOT_THERE:
        assert _same(rec, _stand_in(case, vae)), (name, regime, "the mutant does change something here: it belongs in MUTANTS' verdicts")
        return
    assert not _same(rec, _stand_in(case, vae)), (name, regime, "the mutant changes nothing")
    ratios = _judge(case, vae, rec)
    stage, w = max(ratios.items(), key=lambda kv: kv[1])
    print(f"{name} [{regime}]: worst violation {w:.3g}x at {stage}")
    if (name, regime) in UNDETECTED:
        assert w < 2.0, (name, regime, "is rejected now: take it out of UNDETECTED")
    else:
        assert w >= 2.0, (name, regime, what, stage, w)


def test_undetected_table_is_short_and_names_real_mutants():
    assert len(UNDETECTED) <= 2
    assert all(n in MUTANTS and r in ("act16", "f32store") and why for (n, r), why in {**UNDETECTED, **NOT_THERE}.items())
    assert sorted(m[0] for m in MUTANTS.values()) == list(range(1, 13))
