"""The reconstruction-loss references and bars themselves (tests/recon_loss_refs.py), without a GPU: the closed-form SSIM
gradient the kernels implement equals float64 autograd, the bars accept what a correct implementation may differ by (fp32
roundings at the places the kernels have them, sums in another order) and reject each single mistake an implementation could
make; and the configuration keys of train.py."""
import os

import pytest
import torch
import yaml

import recon_loss_refs as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 3, 12, 37), (1, 3, 24, 20)]
VARIANTS = ["noisy", "flat", "range"]
DELTA, WEIGHT, SCALE = 0.5, 0.2, 0.25
_CACHE = {}


def _case(shape, variant, kind="huber"):
    key = (shape, variant, kind)
    if key not in _CACHE:
        p, t = rr.ssim_inputs(shape, variant)
        _CACHE[key] = (p, t, rr.reference(p, t, kind, DELTA, WEIGHT, SCALE))
    return _CACHE[key]


def _seed_with(p, t, ref, ssim_grad):
    """the seed a kernel pair would leave: exact pixel part + one fp32 rounding of the SSIM part, added in fp32"""
    pix = rr.pixel_seed_fp32(p, t, "huber", DELTA, SCALE)
    return pix + (-SCALE * WEIGHT * ssim_grad).float()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_closed_form_equals_autograd(shape, variant):
    p, t, ref = _case(shape, variant)
    want = ref["seed_ssim"] / (-SCALE * WEIGHT)
    got = rr.ssim_grad_closed_form(p, t)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"{shape} {variant}: closed form against autograd {err:.2e} of the gradient's max")
    assert err <= 1e-10


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bars_accept_a_correct_implementation(shape, variant):
    """the kernels' arithmetic emulated on the CPU: fp32 coefficient and product, the SSIM part from the closed form (another
    summation order than autograd's) rounded once, an fp32 sum; loss sums accumulated in fp32-stored chunks in reverse order"""
    p, t, ref = _case(shape, variant)
    got = _seed_with(p, t, ref, rr.ssim_grad_closed_form(p, t))
    print(f"{shape} {variant}: seed error / bound {rr.seed_excess(got, ref):.3f}")
    assert rr.seed_ok(got, ref)
    d = (p - t).double().flatten()
    terms = torch.where(d.abs() <= DELTA, 0.5 * d * d, DELTA * (d.abs() - 0.5 * DELTA))
    chunks = [c.flip(0).sum() for c in terms.split(97)]
    pixel = float((torch.stack(chunks[::-1]).sum() / d.numel()).float())
    assert rr.loss_ok(pixel, ref["pixel"])
    s = rr.ssim_map(rr.to_unit(p.double()), rr.to_unit(t.double()))
    per_image = torch.stack([im.flatten().flip(0).sum() for im in s]) / s[0].numel()
    assert rr.index_ok(per_image, rr.ssim_index(p, t))
    rec = float((torch.tensor(pixel, dtype=torch.float64) + WEIGHT * (1 - per_image.mean())).float())
    assert rr.loss_ok(rec, ref["rec"])


MISTAKES = {
    "fp32_window_statistics": ("flat", dict(stats_dtype=torch.float32)),
    "clamped_u": ("range", dict(clamp=True)),
    "missing_half": ("noisy", dict(half=1.0)),
    "same_padded_positions": ("noisy", dict(same_pad=True)),
}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bars_reject_ssim_mistakes(shape, mistake):
    variant, kw = MISTAKES[mistake]
    p, t, ref = _case(shape, variant)
    wrong = rr.ssim_grad_closed_form(p, t, **kw)
    want = ref["seed_ssim"] / (-SCALE * WEIGHT)
    print(f"{shape} {mistake}: off by {float((wrong - want).abs().max() / want.abs().max()):.2e} of the gradient's max, "
          f"seed error / bound {rr.seed_excess(_seed_with(p, t, ref, wrong), ref):.3g}")
    assert not rr.seed_ok(_seed_with(p, t, ref, wrong), ref)


def test_bars_reject_a_clamped_or_same_padded_index():
    p, t = rr.ssim_inputs(SHAPES[0], "range")
    ref = rr.ssim_index(p, t)
    clamped = rr.ssim_map(rr.to_unit(p.double()).clamp(0, 1), rr.to_unit(t.double()).clamp(0, 1))
    assert not rr.index_ok(clamped.reshape(clamped.shape[0], -1).mean(1), ref)
    padded = rr.ssim_map(rr.to_unit(p.double()), rr.to_unit(t.double()), same_pad=True)
    assert not rr.index_ok(padded.reshape(padded.shape[0], -1).mean(1), ref)


@pytest.mark.parametrize("n", [3, 257])
def test_bars_reject_pixel_mistakes(n):
    r, x = rr.pixel_inputs(n)
    d = r - x
    assert bool((d == 0).any()) and bool((d.abs() == DELTA).any())
    for kind in rr.KINDS:
        good = rr.pixel_seed_fp32(r, x, kind, DELTA, SCALE)
        ref = rr.reference(r, x, kind, DELTA, 0.0, SCALE)
        assert rr.seed_ok(good, ref), kind           # the fp32 expression is itself inside the float64 bar
        assert not torch.equal(rr.pixel_seed_fp32(r, x, kind, DELTA, 1.0), good)   # a seed that forgets grad_scale
        assert not rr.seed_ok(rr.pixel_seed_fp32(r, x, kind, DELTA, 1.0), ref)
    assert not torch.equal(rr.pixel_seed_fp32(r, x, "l1", DELTA, SCALE, sign0=1.0), rr.pixel_seed_fp32(r, x, "l1", DELTA, SCALE))
    if n > 3:  # elements beyond the forced 0 / +delta / -delta, on which the two branches agree
        assert not torch.equal(rr.pixel_seed_fp32(r, x, "huber", DELTA, SCALE, swap=True), rr.pixel_seed_fp32(r, x, "huber", DELTA, SCALE))
    # at |d| == delta the branches meet: taking the other one there is no mistake, in the value or in the gradient
    at = d.abs() == DELTA
    assert torch.equal(rr.pixel_seed_fp32(r, x, "huber", DELTA, SCALE, swap=True)[at], rr.pixel_seed_fp32(r, x, "huber", DELTA, SCALE)[at])


def test_seed_bar_rejects_a_forgotten_grad_scale_with_ssim():
    p, t, ref = _case(SHAPES[0], "noisy")
    unscaled = rr.reference(p, t, "huber", DELTA, WEIGHT, 1.0)["seed"]
    assert not rr.seed_ok(unscaled, ref)


# ---------------------------------------------------------------------------------------------------------- configuration
def test_spec_validation():
    from vaehip.losses import ReconLoss, as_spec
    assert ReconLoss() == ReconLoss("mse", 1.0, 0.0) and ReconLoss().is_default and as_spec(None).is_default
    assert not ReconLoss("l1").is_default and not ReconLoss(ssim_weight=0.1).is_default
    assert [ReconLoss(k).kind_id for k in ("mse", "l1", "huber")] == [0, 1, 2]
    for bad in (dict(kind="lpips"), dict(huber_delta=0.0), dict(huber_delta=-1.0), dict(ssim_weight=-0.1),
                dict(ssim_weight=float("nan")), dict(huber_delta=float("inf")), dict(huber_delta="1")):
        with pytest.raises(ValueError):
            ReconLoss(**bad)
    with pytest.raises(TypeError):
        as_spec("l1")


def test_config_parsing():
    import train
    from vaehip.losses import ReconLoss
    assert train.recon_loss_settings({}) == ReconLoss() and train.recon_loss_settings({}).is_default
    assert train.recon_loss_settings({"reconstruction_loss": "mse", "ssim_weight": 0, "huber_delta": 0.3}).is_default
    got = train.recon_loss_settings({"reconstruction_loss": "huber", "huber_delta": "5e-1", "ssim_weight": 0.2}, 64)
    assert got == ReconLoss("huber", 0.5, 0.2)
    assert train.recon_loss_settings({"reconstruction_loss": "l1"}, 8) == ReconLoss("l1")   # no SSIM term: any resolution
    for cfg, res, match in [({"reconstruction_loss": "lpips"}, 64, "reconstruction_loss"),
                            ({"reconstruction_loss": None}, 64, "reconstruction_loss"),
                            ({"reconstruction_loss": "huber", "huber_delta": 0}, 64, "huber_delta"),
                            ({"huber_delta": "small"}, 64, "huber_delta"),
                            ({"ssim_weight": -1}, 64, "ssim_weight"),
                            ({"ssim_weight": True}, 64, "ssim_weight"),
                            ({"ssim_weight": 0.1}, 10, "resolution")]:
        with pytest.raises(ValueError, match=match):
            train.recon_loss_settings(cfg, res)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_l1_ssim.yaml")))
    spec = train.recon_loss_settings(cfg["training"], cfg["data"]["resolution"])
    assert spec.kind == "l1" and spec.ssim_weight > 0 and not spec.is_default
