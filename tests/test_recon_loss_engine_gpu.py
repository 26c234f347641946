"""The reconstruction losses of vaehip.losses in the fused step (Engine.forward_backward(recon_loss=...), HipTrainer, train.py)
on the synthetic model of tests/test_engine_gpu.py at R = 32, B = 2: the default spec is the step as it was, bit for bit; Huber +
SSIM against the CPU oracle with the loss written in torch here; L1 in fp32 and bf16 mode through its seed; train.py on the
shipped config."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import yaml

import recon_loss_refs as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, B = 32, 2
DELTA, WEIGHT, KLW = 0.5, 0.2, 1e-4
# the project's convention (tests/test_engine_gpu.py GRAD_TOL): 2x the worst per-tensor gradient error MEASURED on MI355X for
# this case (profiles/recon_loss_measured.json: 4.2e-5, on decoder.mid_block.attentions.0.to_q.bias; the MSE case at this shape
# measures 2.5e-5), itself held to <= 1e-4
GRAD_TOL_HUBER_SSIM = 8.4e-5


def _record(key, value):
    """measured figures of this run -> the JSON file named by VAEHIP_MEASURED_JSON, when set (copied into profiles/ when
    tolerances are set)"""
    path = os.environ.get("VAEHIP_MEASURED_JSON")
    if not path:
        return
    try:
        d = json.load(open(path))
    except Exception:
        d = {}
    d[key] = value
    json.dump(d, open(path, "w"), indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def pair(cuda):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    o = vo.OracleWrapper(seed=42)
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(o.vae.state_dict())
    w.to(cuda)
    return o, w


@pytest.fixture(scope="module")
def batch():
    import vae_oracle as vo
    return vo.synthetic_pixels(B, R, 42), vo.synthetic_eps(B, R, 42)


def _oracle_step(o, x, eps, kind, delta, weight, klw):
    """the oracle's forward in fp32, the loss in float64 torch from its reconstruction (recon_loss_refs), backward into the
    oracle's fp32 parameters"""
    for p in o.parameters():
        p.grad = None
    out = o(x, sample_posterior=True, eps=eps)
    rec = out["reconstruction"].double()
    pixel = rr.pixel_term(rec - x.double(), kind, delta)
    ssim = rr.ssim_map(rr.to_unit(rec), rr.to_unit(x.double())).mean() if weight > 0 else None
    recl = pixel + weight * (1.0 - ssim) if weight > 0 else pixel
    kl = out["latent_dist"].kl().mean()
    total = recl + klw * kl.double()
    total.backward()
    with torch.no_grad():
        return out, {"pixel": float(pixel), "ssim": float(ssim) if weight > 0 else float("nan"), "rec": float(recl),
                     "kl": float(kl), "total": float(total)}


def _close(got, want, tol=1e-4):
    return abs(float(got) - want) <= tol * abs(want)


def test_default_spec_is_the_step_as_it_was(pair, batch):
    from vaehip.losses import ReconLoss
    _, w = pair
    x, eps = batch[0].cuda(), batch[1].cuda()
    eng = w.vae.engine
    base = eng.forward_backward(x, eps, KLW)
    g0, s0 = w.vae.arena.grad.clone(), base["scalars"].clone()
    for spec in (ReconLoss(), None):
        res = eng.forward_backward(x, eps, KLW, recon_loss=spec)
        assert torch.equal(res["scalars"], s0) and torch.equal(w.vae.arena.grad, g0)
        assert res["loss_terms"] is None
    ev = eng.forward_eval(x, eps, True, KLW, recon_loss=ReconLoss())
    assert torch.equal(ev["scalars"], eng.forward_eval(x, eps, True, KLW)["scalars"])


def test_huber_ssim_matches_oracle(pair, batch):
    from vaehip.losses import ReconLoss
    o, w = pair
    x, eps = batch
    out, ref = _oracle_step(o, x, eps, "huber", DELTA, WEIGHT, KLW)
    small = float(((out["reconstruction"].detach() - x).abs() <= DELTA).float().mean())
    print(f"{100 * small:.1f} % of the oracle's residuals are within delta")
    assert 0.25 <= small <= 0.75   # both branches of the Huber term carry at least a quarter of the elements
    spec = ReconLoss("huber", DELTA, WEIGHT)
    res = w.vae.engine.forward_backward(x.cuda(), eps.cuda(), KLW, recon_loss=spec)
    sc, terms = res["scalars"].cpu(), res["loss_terms"].cpu()
    print(f"scalars {sc.tolist()} terms {terms.tolist()} against {ref}")
    assert _close(sc[0], ref["rec"]) and _close(sc[1], ref["kl"]) and _close(sc[2], ref["total"])
    assert _close(terms[0], ref["pixel"]) and _close(terms[1], ref["ssim"])
    # every gradient tensor, as tests/test_engine_gpu.py holds the MSE step: relative to the tensor's own largest gradient;
    # tensors whose reference gradient is below 1e-5 of the model's largest entry are held to that global scale
    worst, worst_name, worst_small, worst_small_name = 0.0, None, 0.0, None
    oparams = dict(o.vae.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in o.vae.parameters())
    for name, p in w.vae.named_parameters():
        want = oparams[name].grad.double()
        err = float((p.grad.detach().double().cpu() - want).abs().max())
        rmax = float(want.abs().max())
        if rmax < 1e-5 * gmax:
            if err / gmax > worst_small:
                worst_small, worst_small_name = err / gmax, name
        elif err / rmax > worst:
            worst, worst_name = err / rmax, name
    print(f"huber + ssim R={R} B={B}: worst grad rel err {worst:.3e} ({worst_name}), near-zero tensors {worst_small:.3e}")
    _record("engine_huber_ssim_grad_worst", {"R": R, "B": B, "rel_to_own_max": worst, "tensor": worst_name,
                                             "near_zero_rel_to_global_max": worst_small, "near_zero_tensor": worst_small_name})
    assert GRAD_TOL_HUBER_SSIM <= 1e-4
    assert worst <= GRAD_TOL_HUBER_SSIM, (worst_name, worst)
    assert worst_small <= 1e-6, (worst_small_name, worst_small)
    gn_ref = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in o.vae.parameters()))
    gn = torch.sqrt((w.vae.arena.grad.double() ** 2).sum()).cpu()
    assert abs(gn - gn_ref) / gn_ref < 1e-4
    # evaluation forward: the same terms without a seed
    ev = w.vae.engine.forward_eval(x.cuda(), eps.cuda(), True, KLW, recon_loss=spec)
    assert torch.equal(ev["scalars"], res["scalars"]) and torch.equal(ev["loss_terms"], res["loss_terms"])


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_l1_seed_in_both_precision_modes(pair, batch, mode):
    """the seed against the references evaluated on the engine's OWN returned reconstruction (per-tensor gradients are not held
    to the oracle for l1: a reconstruction that differs in the fifth digit flips sign(d) near zero)"""
    from vaehip.losses import ReconLoss
    o, w = pair
    x, eps = batch
    tgt = x.permute(0, 2, 3, 1).contiguous()
    eng = w.vae.engine
    eng.set_precision(mode)
    try:
        res = eng.forward_backward(x.cuda(), eps.cuda(), KLW, recon_loss=ReconLoss("l1"), grad_scale=0.5)
        rec, seed = res["reconstruction"].float().cpu(), res["drecon"].cpu()
        assert rec.shape == tgt.shape and seed.shape == tgt.shape and seed.dtype == torch.float32
        assert torch.equal(seed, rr.pixel_seed_fp32(rec, tgt, "l1", 1.0, 0.5))
        own = rr.reference(rec, tgt, "l1", 1.0, 0.0, 0.5)
        assert rr.seed_ok(seed, own) and _close(res["scalars"][0].cpu(), own["pixel"], 2e-7)
        assert bool(torch.isfinite(w.vae.arena.grad).all()) and float(w.vae.arena.grad.abs().max()) > 0
        if mode == "no":
            _, ref = _oracle_step(o, x, eps, "l1", 1.0, 0.0, KLW)
            assert _close(res["scalars"][0].cpu(), ref["rec"]) and _close(res["scalars"][2].cpu(), ref["total"])
        # with the SSIM term on top: the combined seed inside its float64 bar (NHWC tensors, as the engine holds them)
        res = eng.forward_backward(x.cuda(), eps.cuda(), KLW, recon_loss=ReconLoss("l1", 1.0, WEIGHT), grad_scale=0.5)
        rec = res["reconstruction"].float().cpu()
        own = rr.reference(rec.permute(0, 3, 1, 2), x, "l1", 1.0, WEIGHT, 0.5)
        ex = rr.seed_excess(res["drecon"].cpu().permute(0, 3, 1, 2), own)
        print(f"mode {mode}: l1 + ssim seed error / bound {ex:.3f}")
        assert ex <= 1.0
        assert _close(res["loss_terms"][1].cpu(), own["ssim"], 2e-7) and _close(res["scalars"][0].cpu(), own["rec"], 2e-7)
    finally:
        eng.set_precision("no")


def test_train_cli_on_the_shipped_config(cuda, tmp_path):
    """train.py on configs/experiment_synthetic_l1_ssim.yaml, cut to two optimizer updates of two micro-batches each"""
    src = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
    c = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_l1_ssim.yaml")))
    c["output_dir"] = str(tmp_path)
    c["data"].update(dataset_name="synthetic:16", resolution=32, batch_size=4, validation_max_samples=4, validation_batch_size=4)
    c["training"].update(num_train_epochs=1, gradient_accumulation_steps=2, validation_epochs=1)
    c["logging"]["log_interval"] = 1
    cpath = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(c, open(cpath, "w"))
    r = subprocess.run([sys.executable, os.path.join(src, "train.py"), "--config_path", cpath], env=dict(os.environ, PYTHONPATH=src),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in open(tmp_path / c["run_name"] / "metrics.jsonl")]
    steps = [l for l in lines if "train_loss_step" in l]
    assert len(steps) == 2, lines
    for l in steps:
        assert math.isfinite(l["train/pixel_loss"]) and l["train/pixel_loss"] > 0 and math.isfinite(l["train/ssim"]), l
    assert any("validation/avg_reconstruction_loss" in l for l in lines)
