"""vae_adamw_ema (csrc/elementwise.hip) and what is built on it: the optimizer's weight average, HipTrainer.ema_weights(),
and save_state / load_state.

Two properties carry everything: (1) with the average on, p, m, v -- and so the whole trajectory -- are bit for bit what
vae_adamw gives; (2) the average is, step by step, the float64 recursion of tests/ema_refs.py over the kernel's own weights,
within 4 * 2^-24 * max(|e|, |p'|) per step (derived there from the two roundings of e' = fmaf(omd, p' - e, e))."""
import functools
import gc

import pytest
import torch

import ema_refs as er
import streaming_refs as sr

pytestmark = pytest.mark.gpu

HYPER = (1e-3, 0.9, 0.999, 1e-8, 1e-2)   # lr, betas, eps, weight decay of the kernel cases
SIZES = [1, 3, 4, 5, 1024, 1027, sr.ADAM_GRID_N]


# ---------------------------------------------------------------------------------------------------- the kernel
@functools.lru_cache(maxsize=2)
def _state(n):
    """p, m, v, g as tests/test_streaming_edges_gpu.py::test_adamw_and_sqnorm_sizes builds them, and an average 1 % off the
    weights; CPU tensors, shared between the cases of one size: read, never written"""
    gen = torch.Generator().manual_seed(n)
    p = sr.adam_params(n, seed=n)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 1e-2
    g = torch.randn(n, generator=gen) * 3.0
    e = p + 0.01 * torch.randn(n, generator=gen) * p.abs()
    return p, m, v, g, e


def _sqnorm(ops, gd):
    return ops.sqnorm(gd, torch.full((1,), float("nan"), device=gd.device), torch.full((2048,), float("nan"), device=gd.device))


def _worst(got, ref64, bound):
    """largest |got - ref| / bound over the elements (a zero bound allows a zero error only)"""
    err = (got.double() - ref64).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


@pytest.mark.parametrize("max_norm", [1.0, 0.0])
@pytest.mark.parametrize("d", [0.0, 2 / 11, 0.9999])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_ema_sizes_and_edges(cuda, n, d, max_norm):
    """no float4 at all, exactly one, one and a tail, whole float4s, more float4s than the capped grid has threads; the copying
    first update, an early decay and the capped one; with the clip coefficient and without a norm pointer"""
    from vaehip import ops
    p0, m0, v0, g, e0 = _state(n)
    gd = g.cuda()
    sq = _sqnorm(ops, gd) if max_norm > 0 else None
    p, m, v, e = (t.cuda() for t in (p0, m0, v0, e0))
    ops.adamw_ema(p, gd, m, v, e, sq, max_norm, *HYPER, 2, d)
    pr, mr, vr = (t.cuda() for t in (p0, m0, v0))
    ops.adamw(pr, gd, mr, vr, sq, max_norm, *HYPER, 2)
    torch.cuda.synchronize()
    assert torch.equal(gd, g.cuda())
    for name, got, want in (("p", p, pr), ("m", m, mr), ("v", v, vr)):
        assert torch.equal(got, want), (name, n, d, max_norm)
    assert not torch.equal(p, p0.cuda())   # (the step did move the weights)
    worst = _worst(e, er.ema_ref64(e0.cuda(), p, d), er.step_bound(e0.cuda(), p))
    print(f"adamw_ema n={n} d={d} max_norm={max_norm}: worst |e' - ref| / bound = {worst:.3f}")
    assert worst <= 1.0
    if d == 0:
        assert torch.equal(e, p)


def test_adamw_ema_five_steps_with_the_schedule(cuda):
    """streaming_refs.ADAM_STEPS (lr = 0 first, gradients of scale 3 and 1e-5) with d_t of the schedule: the final average
    against the float64 recursion over the kernel's own weights, within the sum of the five per-step bounds"""
    from vaehip import ops
    n = sr.ADAM_N
    p = sr.adam_params(n).cuda()
    m, v = torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    e = (sr.adam_params(n, seed=4) * 1.5).cuda()   # anything: the first update must overwrite it
    e64 = e.double()
    bound = torch.zeros(n, device=cuda, dtype=torch.float64)
    for step, (lr, gs) in enumerate(sr.ADAM_STEPS, start=1):
        d = er.decay_schedule(step)
        gd = sr.adam_grad(n, gs, 100 + step).cuda()
        ops.adamw_ema(p, gd, m, v, e, _sqnorm(ops, gd), 1.0, lr, *sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"], step, d)
        if step > 1:
            bound += er.step_bound(e64, p)
        e64 = er.ema_ref64(e64, p, d)
        if step == 1:
            assert torch.equal(e, p)
    worst = _worst(e, e64, bound)
    print(f"adamw_ema five steps: worst |e - ref| / (sum of the per-step bounds) = {worst:.3f}")
    assert worst <= 1.0
    assert float((e - p).abs().max()) > 0   # an average, not a copy


def test_adamw_ema_refusals(cuda):
    """argument checks: each returns VAE_EINVAL before any launch (the state is untouched)"""
    from vaehip import ops
    from vaehip.lib import VaeHipError
    n = 1024
    p0, m0, v0, g, e0 = _state(n)
    p, m, v, gd = (t.cuda() for t in (p0, m0, v0, g))
    room = torch.zeros(n + 4, device=cuda)
    room[1:n + 1] = e0.cuda()
    cases = (("unaligned", room[1:n + 1], 0.5), ("overlaps", p, 0.5), ("overlaps", m[: n], 0.5), ("outside", e0.cuda(), 1.0),
             ("outside", e0.cuda(), -0.25))
    for what, e, d in cases:
        keep = e.clone()
        with pytest.raises(VaeHipError, match=what):
            ops.adamw_ema(p, gd, m, v, e, None, 0.0, *HYPER, 2, d)
        torch.cuda.synchronize()
        assert torch.equal(e, keep), what
        for name, got, want in (("p", p, p0), ("m", m, m0), ("v", v, v0)):
            assert torch.equal(got.cpu(), want), (what, name)
    with pytest.raises(VaeHipError, match="bad args"):
        ops.adamw_ema(p, gd, m, v, None, None, 0.0, *HYPER, 2, 0.5)


def test_guarded_adamw_ema(cuda):
    """n = 1027 in guarded, poisoned memory (tests/guarded.py), as test_guarded_gpu.py::test_guarded_sqnorm_adamw: p, m, v, e
    in place, g read-only, no store outside a tensor, no poisoned element in a result"""
    from test_guarded_gpu import INPLACE, _check
    n = 1027
    p, m, v, g, e = _state(n)
    operands = dict(p=p.clone(), g=g.clone(), m=m.clone(), v=v.clone(), e=e.clone(), out=torch.zeros(1))

    def fn(ops, t):
        ops.sqnorm(t["g"], t["out"])
        ops.adamw_ema(t["p"], t["g"], t["m"], t["v"], t["e"], t["out"], 1.0, *HYPER, 2, 0.9999)
        return [t["out"], t["p"], t["m"], t["v"], t["e"]]

    _check("sqnorm + adamw_ema", operands, fn, inplace=INPLACE["adamw"] + ("e", "out"))


# ---------------------------------------------------------------------------------------------------- optimizer and trainer
R, B, UPDATES = 32, 2, 4
TRAINER = dict(lr=1e-3, kl_weight=1e-3, lr_warmup_steps=1, max_train_steps=10)   # lr = 0 on the first update, as in train.py


def _inputs(s, cuda):
    import vae_oracle as vo
    return vo.synthetic_pixels(B, R, 42, s).to(cuda), vo.synthetic_eps(B, R, 42, s).to(cuda)


def _build(cuda, **kw):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.trainer import HipTrainer
    w = SDXLVAEWrapper("synthetic:1")
    w.to(cuda)
    return w, HipTrainer(w, **TRAINER, **kw)


def _snapshot(tr, res):
    o = tr.optimizer
    return dict(flat=tr.vae.arena.flat.clone(), m=o.exp_avg.clone(), v=o.exp_avg_sq.clone(), scalars=res["scalars"].clone(),
                ema=None if o.ema is None else o.ema.clone(), step=tr.global_step, lr=tr.lr_scheduler.get_last_lr())


def _run(cuda, first, last, tr, accum=1):
    """updates first..last (1-based) on the fixed inputs; with accum = 2 every update takes micro-batches 2u-1 and 2u"""
    out = []
    for u in range(first, last + 1):
        for k in range(accum):
            res = tr.train_step(*_inputs(accum * (u - 1) + k + 1, cuda))
        out.append(_snapshot(tr, res))
    return out


def _same(a, b, keys=("flat", "m", "v", "scalars")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


def _average_follows_the_recursion(start, snaps):
    prev = start
    for t, s in enumerate(snaps, start=1):
        d = er.decay_schedule(t, 0.9999)
        worst = _worst(s["ema"], er.ema_ref64(prev, s["flat"], d), er.step_bound(prev, s["flat"]))
        print(f"trainer update {t} (d = {d:.4f}): worst |ema - ref| / bound = {worst:.3f}")
        assert worst <= 1.0, t
        if t == 1:
            assert torch.equal(s["ema"], s["flat"])
        prev = s["ema"]
    assert float((snaps[-1]["ema"] - snaps[-1]["flat"]).abs().max()) > 0


@pytest.fixture(scope="module")
def straight(cuda):
    """four updates at R = 32, B = 2 with the average on and with it off, same inputs -> (snapshots on, snapshots off,
    the average before the first update, the trainer with the average: left as it is after update 4)"""
    w, tr = _build(cuda, use_ema=True)
    start = tr.optimizer._ensure().flat.clone()
    assert torch.equal(tr.optimizer.ema, start) and tr.optimizer.ema.data_ptr() != tr.vae.arena.flat.data_ptr()
    on = _run(cuda, 1, UPDATES, tr)
    _, tr_off = _build(cuda)
    off = _run(cuda, 1, UPDATES, tr_off)
    assert tr_off.optimizer.ema is None
    del tr_off
    return on, off, start, tr


def test_the_average_never_changes_the_trajectory(straight):
    on, off, _, _ = straight
    for a, b in zip(on, off):
        _same(a, b)
        assert a["lr"] == b["lr"] and a["step"] == b["step"]
    assert not torch.equal(on[-1]["flat"], on[0]["flat"])


def test_the_trainers_average_follows_the_recursion(straight):
    on, _, start, _ = straight
    _average_follows_the_recursion(start, on)


def test_bf16_mode_averages_the_fp32_masters(cuda):
    _, tr = _build(cuda, use_ema=True, mixed_precision="bf16")
    start = tr.optimizer._ensure().flat.clone()
    on = _run(cuda, 1, UPDATES, tr)
    del tr
    _, tr_off = _build(cuda, mixed_precision="bf16")
    off = _run(cuda, 1, UPDATES, tr_off)
    for a, b in zip(on, off):
        _same(a, b)
    assert on[-1]["ema"].dtype == torch.float32
    _average_follows_the_recursion(start, on)


def test_the_average_moves_on_real_updates_only(cuda):
    """gradient_accumulation_steps = 2 over four micro-batches: the average changes on calls 2 and 4"""
    _, tr = _build(cuda, use_ema=True, gradient_accumulation_steps=2)
    prev = tr.optimizer._ensure().flat.clone() + 1.0   # (differs from the start: call 2's copy of the weights is a change)
    tr.optimizer.ema.copy_(prev)
    for call in range(1, 5):
        tr.train_step(*_inputs(call, cuda))
        now = tr.optimizer.ema.clone()
        if call % 2:
            assert not tr.sync_gradients and torch.equal(now, prev), call
        else:
            assert tr.sync_gradients and not torch.equal(now, prev), call
        prev = now
    assert tr.global_step == 2 and tr.optimizer.step_count == 2
    # flush() is a real update too: one pending micro-batch, then the average moves
    tr.train_step(*_inputs(5, cuda))
    assert torch.equal(tr.optimizer.ema, prev) and tr.pending_micro_batches == 1
    tr.flush()
    assert tr.global_step == 3 and not torch.equal(tr.optimizer.ema, prev)


def test_ema_weights_exchanges_and_restores(straight, cuda, tmp_path):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    on, _, _, tr = straight
    flat, ema = tr.vae.arena.flat.clone(), tr.optimizer.ema.clone()
    x, _ = _inputs(9, cuda)
    tr.wrapper.eval()
    raw = tr.eval_step(x)["scalars"].clone()
    with tr.ema_weights():
        assert torch.equal(tr.vae.arena.flat, ema) and torch.equal(tr.optimizer.ema, flat)
        avg = tr.eval_step(x)["scalars"].clone()
        tr.vae.save_pretrained(str(tmp_path / "vae_ema"))
        sd = {k: v.clone() for k, v in tr.wrapper.state_dict().items()}
    tr.wrapper.train()
    assert torch.equal(tr.vae.arena.flat, flat) and torch.equal(tr.optimizer.ema, ema)
    assert torch.equal(tr.eval_step(x)["scalars"], raw) and not torch.equal(avg, raw)
    w2 = SDXLVAEWrapper(str(tmp_path / "vae_ema"), device=cuda)
    assert torch.equal(w2.vae.arena.flat, ema)
    assert all(torch.equal(v, sd["vae." + k]) for k, v in w2.vae.state_dict().items())
    with pytest.raises(RuntimeError, match="use_ema"):   # (a trainer without an average has nothing to exchange)
        with type(tr)(w2, **TRAINER).ema_weights():
            pass


@pytest.mark.parametrize("accum", [1, 2])
def test_resume_is_exact(cuda, tmp_path, accum):
    """A: four updates straight.  B: two (accum = 2: and one more micro-batch, so a gradient sum is pending), save_state,
    everything dropped, a new wrapper and trainer, load_state, the rest.  Same weights, moments, average, scalars, counters."""
    import train
    kw = dict(use_ema=True, gradient_accumulation_steps=accum)
    _, a = _build(cuda, **kw)
    ref = _run(cuda, 1, UPDATES, a, accum)
    del a
    w, b = _build(cuda, **kw)
    _run(cuda, 1, 2, b, accum)
    if accum == 2:
        b.train_step(*_inputs(5, cuda))
        assert b.pending_micro_batches == 1
    train.save_state(str(tmp_path), w, b)
    del w, b
    gc.collect()
    w, b = _build(cuda, **kw)
    with torch.no_grad():   # nothing of the new objects' own state may survive the load
        b.vae.arena.flat.mul_(0.5)
    assert train.load_state(str(tmp_path), w, b) == 2
    assert b.global_step == 2 and b.optimizer.step_count == 2 and b.pending_micro_batches == accum - 1
    if accum == 2:
        res = b.train_step(*_inputs(6, cuda))
        assert b.sync_gradients
        got = [_snapshot(b, res)] + _run(cuda, 4, 4, b, accum)
    else:
        got = _run(cuda, 3, 4, b, accum)
    for want, have in zip(ref[2:], got):
        _same(want, have, ("flat", "m", "v", "ema", "scalars"))
        assert want["step"] == have["step"] and want["lr"] == have["lr"]
    assert b.global_step == UPDATES
