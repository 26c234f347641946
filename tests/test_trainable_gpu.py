"""Frozen parameters on the GPU: the two *_ranges entry points in guarded, NaN-poisoned memory, and the engine / trainer with
`decoder`, `encoder` and GroupNorm-only trainable sets in the scenario of tests/golden/e2e_r32.json."""
import bisect
import json
import os
import types

import pytest
import torch

import streaming_refs as sr
from guarded import GuardedPool

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SETS = ("decoder", "encoder", "norms")


# ------------------------------------------------------------------------------------------------- kernel level
def _range_cases(C):
    many, b = [], 0
    for i in range(130):  # 8 .. 520 elements, not all multiples of 4, separated by frozen gaps of 8 (starts stay on multiples of 8)
        n = min(520, 8 + 4 * i + i % 3)
        many.append((b, b + n))
        b = (b + n + 7) // 8 * 8 + 8
    cases = {f"one_{n}": ([(0, n)], n) for n in (1, 3, 8, 1027)}
    cases.update({"chunk": ([(0, C)], C + 8), "chunk_plus_4": ([(0, C + 4)], C + 12), "two_chunks_less_1": ([(0, 2 * C - 1)], 2 * C + 7),
                  "8_24_alone": ([(8, 24)], 40), "0_8_and_8_24": ([(0, 8), (8, 24)], 32), "130_ranges": (many, b + 16),
                  "ends_at_the_last_element": ([(0, 8), (16, 16 + C + 5)], 16 + C + 5)})
    return cases


def _bits(t):
    return t.view(torch.int32)


@pytest.fixture(scope="module")
def chunk(cuda):
    from vaehip.lib import lib
    return lib.query("vae_dead_scan_chunk")


@pytest.mark.parametrize("case", list(_range_cases(32768)))
def test_ranges_kernels_in_guarded_memory(cuda, chunk, case):
    """g is NaN outside the ranges, p / m / v / e hold canaries there; the workspace and the result start as NaN.  Inside:
    bitwise vae_adamw(_ema) on a compact copy with the same norm tensor; outside: not a bit changed; no guard byte touched."""
    from vaehip import ops
    from vaehip.trainable import RangeTable
    ranges, n = _range_cases(chunk)[case]
    gen = torch.Generator().manual_seed(len(case) * 131 + n)
    inside = torch.zeros(n, dtype=torch.bool)
    for b, e in ranges:
        inside[b:e] = True
    host = dict(p=sr.adam_params(n, seed=n), g=torch.randn(n, generator=gen) * 3.0, m=torch.randn(n, generator=gen) * 0.1,
                v=torch.rand(n, generator=gen) * 1e-2, e=sr.adam_params(n, seed=n + 1))
    host["g"][~inside] = float("nan")
    pool = GuardedPool(cuda)
    tab = RangeTable(ranges, cuda, n)
    tab.seg_off, tab.seg_chunk0 = pool.put(tab.seg_off, "seg_off"), pool.put(tab.seg_chunk0, "seg_chunk0")
    tab.ws = pool.alloc(tab.nchunk, label="ws")          # poisoned: every chunk must write its partial
    g = pool.put(host["g"], "g")
    out, out2 = pool.alloc(1, label="out"), pool.alloc(1, label="out2")
    ops.sqnorm_ranges(g, tab, out)
    assert pool.unwritten(tab.ws) == 0
    ops.sqnorm_ranges(g, tab, out2)
    assert torch.equal(_bits(out), _bits(out2))           # bitwise repeatable
    gin = host["g"][inside]
    ref = sr.sqnorm_ref64(gin)
    cpu = abs(float((gin * gin).sum()) - ref) / ref
    sr.check("sqnorm_ranges", case, abs(float(out.item()) - ref) / ref, sr.bar(4, cpu, 1e-6), cpu)
    idx = inside.to(cuda)
    for ema, max_norm, decay in ((False, 1.0, 0.0), (False, 0.0, 0.0), (True, 1.0, 0.9), (True, 0.0, 0.0)):
        t = {k: pool.put(host[k], k) for k in ("p", "m", "v") + (("e",) if ema else ())}
        c = {k: host[k][inside].to(cuda) for k in t}       # the compact copy, for the whole-buffer kernel
        hp = (out, max_norm, 1e-3, *sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"], 2)
        ops.adamw_ranges(t["p"], g, t["m"], t["v"], t.get("e"), tab, *hp, decay)
        if ema:
            ops.adamw_ema(c["p"], gin.to(cuda), c["m"], c["v"], c["e"], *hp, decay)
        else:
            ops.adamw(c["p"], gin.to(cuda), c["m"], c["v"], *hp)
        for k in t:
            assert torch.equal(_bits(t[k][idx]), _bits(c[k])), (case, ema, max_norm, k, "inside the ranges")
            assert torch.equal(_bits(t[k][~idx]), _bits(host[k][~inside].to(cuda))), (case, ema, max_norm, k, "outside the ranges")
            assert not torch.isnan(t[k][idx]).any()
        assert not torch.equal(t["p"][idx], host["p"][inside].to(cuda))   # the update happened
    assert torch.equal(_bits(g), _bits(host["g"].to(cuda)))
    assert pool.violations() == []


def test_ranges_entry_points_refuse_bad_arguments(cuda, chunk):
    from vaehip import ops
    from vaehip.lib import VaeHipError
    from vaehip.trainable import RangeTable
    n = 64
    tab = RangeTable([(0, 8), (16, 40)], cuda, n)
    p, g, m, v, e = (torch.ones(n + 4, device=cuda) * k for k in (1.0, 2.0, 0.0, 0.0, 1.0))
    out = torch.zeros(1, device=cuda)
    hp = (out, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1)

    def variant(**kw):
        d = dict(seg_off=tab.seg_off, seg_chunk0=tab.seg_chunk0, nseg=tab.nseg, nchunk=tab.nchunk, ws=tab.ws)
        d.update(kw)
        return types.SimpleNamespace(**d)
    bad_tables = [variant(seg_off=None), variant(seg_chunk0=None), variant(nseg=0), variant(nchunk=tab.nseg - 1)]
    for t in bad_tables:
        with pytest.raises(VaeHipError, match="bad args"):
            ops.sqnorm_ranges(g, t, out)
        with pytest.raises(VaeHipError, match="bad args"):
            ops.adamw_ranges(p, g, m, v, None, t, *hp)
    with pytest.raises(VaeHipError, match="bad args"):
        ops.sqnorm_ranges(g, variant(ws=None), out)
    with pytest.raises(VaeHipError, match="unaligned"):
        ops.sqnorm_ranges(g[1:], tab, out)
    for k in range(5):  # each base pointer off by one float in turn
        a = [p, g, m, v, e]
        a[k] = a[k][1:]
        with pytest.raises(VaeHipError, match="unaligned"):
            ops.adamw_ranges(*a, tab, *hp, 0.5)
    for decay in (1.0, -0.1, float("nan")):
        with pytest.raises(VaeHipError, match="ema_decay"):
            ops.adamw_ranges(p, g, m, v, e, tab, *hp, decay)
    for alias in (p, g, m, v):
        with pytest.raises(VaeHipError, match="overlaps"):
            ops.adamw_ranges(p, g, m, v, alias, tab, *hp, 0.5)
    with pytest.raises(VaeHipError, match="clipping needs sqnorm"):
        ops.adamw_ranges(p, g, m, v, None, tab, None, 1.0, *hp[2:])
    torch.cuda.synchronize()
    # nothing was launched
    assert float(out) == 0.0 and bool((p == 1).all()) and bool((m == 0).all()) and bool((v == 0).all()) and bool((e == 1).all())
    with pytest.raises(ValueError, match="range table"):
        RangeTable([(2, 8)], cuda, n)


# ------------------------------------------------------------------------------------------------- engine and trainer
def _golden():
    return json.load(open(os.path.join(G, "e2e_r32.json")))


def _value(vae, which):
    if which == "norms":
        return [n for n, m in vae.named_modules() if isinstance(m, torch.nn.GroupNorm)]
    return which


def _wrapper(cuda):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), 42))
    return w.to(cuda)


def _batch(B, R, step, cuda):
    import vae_oracle as vo
    return vo.synthetic_pixels(B, R, 42, step).to(cuda), vo.synthetic_eps(B, R, 42, step).to(cuda)


# the frozen GroupNorm scale that is nudged before the run (so that a stray weight decay or Adam step on it would show)
NUDGED = {"decoder": "encoder.down_blocks.0.resnets.0.norm1.weight", "encoder": "decoder.up_blocks.1.resnets.0.norm1.weight",
          "norms": None}


def _inside(arena, device):
    mask = torch.zeros(arena.total, dtype=torch.bool, device=device)
    for b, e in arena.trainable_ranges():
        mask[b:e] = True
    return mask


def _compare_grads(vae, full_grad, full, res, what):
    a = vae.arena
    for k in ("scalars", "reconstruction", "moments"):
        assert torch.equal(res[k], full[k]), (what, k)
    n_tr = 0
    for name, p, o, n in a.entries:
        if p.requires_grad:
            n_tr += 1
            assert p.grad is not None and p.grad.data_ptr() == a.grad.data_ptr() + 4 * o, (what, name)
            assert torch.equal(_bits(a.grad[o:o + n]), _bits(full_grad[o:o + n])), (what, name)
        else:
            assert p.grad is None, (what, name)
    assert n_tr > 0


@pytest.fixture(scope="module")
def full(cuda):
    """one wrapper and its full backward (every parameter trainable) on the scenario's first batch: the reference of the
    gradient tests, computed once"""
    g = _golden()
    w = _wrapper(cuda)
    x, eps = _batch(g["B"], g["R"], 1, cuda)
    res = w.vae.engine.forward_backward(x, eps, g["kl_weight"])
    return g, w, x, eps, {k: v.clone() for k, v in res.items() if v is not None}, w.vae.arena.grad.clone()


@pytest.mark.parametrize("which", SETS + ("encoder.mid_block", "decoder.up_blocks.3"))
def test_trainable_gradients_are_those_of_the_full_backward(full, which):
    from vaehip.trainable import apply_trainable
    g, w, x, eps, ref, ref_grad = full
    vae = w.vae
    try:
        apply_trainable(vae, _value(vae, which) if which in SETS else [which])
        vae.arena.grad.fill_(float("nan"))  # whatever a frozen stretch holds afterwards, nothing below reads it
        res = vae.engine.forward_backward(x, eps, g["kl_weight"])
        _compare_grads(vae, ref_grad, ref, res, which)
    finally:
        vae.requires_grad_(True)


def test_trainable_gradients_bf16_decoder(cuda):
    from vaehip.trainable import apply_trainable
    g = _golden()
    w = _wrapper(cuda)
    vae = w.vae
    vae.engine.set_precision("bf16")
    x, eps = _batch(2, 64, 1, cuda)
    res = vae.engine.forward_backward(x, eps, g["kl_weight"])
    ref, ref_grad = {k: v.clone() for k, v in res.items() if v is not None}, vae.arena.grad.clone()
    apply_trainable(vae, "decoder")
    vae.arena.grad.fill_(float("nan"))
    _compare_grads(vae, ref_grad, ref, vae.engine.forward_backward(x, eps, g["kl_weight"]), "bf16 decoder")


class _Spy:
    """wraps the backward launch sites of vaehip.ops and books every call on the parameter it belongs to"""

    def __init__(self, monkeypatch, vae):
        from vaehip import ops
        a = vae.arena
        self.offs = [o for _, _p, o, _n in a.entries]
        self.names = [n for n, _p, _o, _n in a.entries]
        self.req = {n: p.requires_grad for n, p, _o, _n in a.entries}
        self.flat, self.grad = a.flat, a.grad
        self.calls = {k: [] for k in ("wgrad", "dgrad", "gn_bwd")}
        self.count = {k: 0 for k in ("sample_kl_bwd", "attn_bwd", "gemm")}

        def owner(t, base):
            off = (t.data_ptr() - base.data_ptr()) // 4
            assert 0 <= off < base.numel(), "not a view of the arena"
            return self.names[bisect.bisect_right(self.offs, off) - 1]

        def book(name, key, who):
            real = getattr(ops, name)

            def f(*args, **kw):
                if key in self.calls:
                    self.calls[key].append(who(args))
                else:
                    self.count[key] += 1
                return real(*args, **kw)
            monkeypatch.setattr(ops, name, f)
        book("conv_wgrad", "wgrad", lambda args: owner(args[3], self.grad))      # wgrad_out: a view of the gradient arena
        book("conv_dgrad", "dgrad", lambda args: owner(args[1], self.flat))      # the weight
        book("gn_bwd", "gn_bwd", lambda args: owner(args[3], self.flat))         # gamma
        book("sample_kl_bwd", "sample_kl_bwd", None)
        book("attn_bwd", "attn_bwd", None)
        for name in ("gemm_nt", "gemm_nn", "gemm_tn"):                           # the materialised attention, forward and backward
            book(name, "gemm", None)

    def backward_owners(self):
        return self.calls["wgrad"] + self.calls["dgrad"] + self.calls["gn_bwd"]


# gemm calls of one materialised attention block: 2 in the forward (scores, context), 4 in the backward (dP, dv, dq, dk); the model has one per mid block
GEMM_FWD, GEMM_BWD = 2, 4


@pytest.mark.parametrize("which", SETS + ("encoder.mid_block", "decoder.up_blocks.3"))
def test_launch_spy(full, monkeypatch, which):
    from vaehip.trainable import apply_trainable
    g, w, x, eps, _ref, _grad = full
    vae = w.vae
    try:
        apply_trainable(vae, _value(vae, which) if which in SETS else [which])
        spy = _Spy(monkeypatch, vae)
        vae.engine.forward_backward(x, eps, g["kl_weight"])
        monkeypatch.undo()
        own = spy.backward_owners()
        assert spy.count["attn_bwd"] == 0  # R = 32: the materialised attention
        # no weight gradient for a layer whose weight and bias are both frozen
        for n in spy.calls["wgrad"]:
            stem = n.rsplit(".", 1)[0]
            assert spy.req[stem + ".weight"] or spy.req.get(stem + ".bias", False), n
        # ... and one for every trainable convolution / linear layer
        want = {n for n, r in spy.req.items() if r and n.endswith(".weight") and "norm" not in n.rsplit(".", 2)[-2]}
        assert want <= set(spy.calls["wgrad"]), sorted(want - set(spy.calls["wgrad"]))[:5]
        enc = [n for n in own if n.startswith("encoder.") or n.startswith("quant_conv.")]
        if which in ("decoder", "decoder.up_blocks.3"):
            assert enc == [] and spy.count["sample_kl_bwd"] == 0
        else:
            assert spy.count["sample_kl_bwd"] == 1
        if which == "decoder":
            assert "post_quant_conv.weight" in spy.calls["wgrad"] and "post_quant_conv.weight" not in spy.calls["dgrad"]
            assert spy.count["gemm"] == 2 * GEMM_FWD + GEMM_BWD
        if which == "decoder.up_blocks.3":
            # nothing before decoder.up_blocks.3.resnets.0 has a backward: not the mid block's attention, not up_blocks.0-2
            assert all(n.startswith("decoder.up_blocks.3.") or n.startswith("decoder.conv_norm_out") or n.startswith("decoder.conv_out")
                       for n in own), [n for n in own if not n.startswith("decoder.up_blocks.3.")][:5]
            assert spy.count["gemm"] == 2 * GEMM_FWD
        if which == "encoder.mid_block":
            assert [n for n in own if n.startswith("encoder.down_blocks.") or n.startswith("encoder.conv_in.")] == []
            assert any(n.startswith("encoder.mid_block.") for n in spy.calls["wgrad"])
            assert any(n.startswith("decoder.") for n in spy.calls["dgrad"]) and not any(n.startswith("decoder.") for n in spy.calls["wgrad"])
            assert spy.count["gemm"] == 2 * (GEMM_FWD + GEMM_BWD)
        if which == "encoder":
            assert "encoder.conv_in.weight" in spy.calls["wgrad"] and "encoder.conv_in.weight" not in spy.calls["dgrad"]
        if which == "norms":  # every GroupNorm's backward runs (it is what gives it its gradient), no weight gradient at all
            assert spy.calls["wgrad"] == []
            assert set(spy.calls["gn_bwd"]) == {n for n, r in spy.req.items() if r and n.endswith(".weight")}
            assert "encoder.conv_in.weight" not in spy.calls["dgrad"]
    finally:
        monkeypatch.undo()
        vae.requires_grad_(True)


# -- the four-step run of each set: measured once, judged by the step test and the trajectory test
_RUNS = {}
SAMPLE_EDGE, SAMPLE_STRIDE = 1 << 16, 61


def _sample(ranges, device):
    """the elements on which the float64 AdamW reference is evaluated: the update is elementwise given the norm, and the
    float64 reference of 49 M elements on the CPU takes seconds per step, so a range contributes its first and last 65536
    elements (where chunk and vector boundaries lie) and every 61st in between; the GroupNorm ranges are taken whole"""
    idx = []
    for b, e in ranges:
        if e - b <= 4 * SAMPLE_EDGE:
            idx.append(torch.arange(b, e, device=device))
        else:
            idx += [torch.arange(b, b + SAMPLE_EDGE, device=device), torch.arange(b + SAMPLE_EDGE, e - SAMPLE_EDGE, SAMPLE_STRIDE, device=device),
                    torch.arange(e - SAMPLE_EDGE, e, device=device)]
    return torch.cat(idx)


def _run(which, cuda):
    if which in _RUNS:
        return _RUNS[which]
    from vaehip.trainer import HipTrainer
    g = _golden()
    w = _wrapper(cuda)
    vae = w.vae
    if NUDGED[which]:
        with torch.no_grad():
            dict(vae.named_parameters())[NUDGED[which]].mul_(1.05)
    tr = HipTrainer(w, lr=g["lr"], lr_warmup_steps=g["warmup"], max_train_steps=g["max_steps"], kl_weight=g["kl_weight"],
                    max_grad_norm=1.0, trainable=_value(vae, which))
    a, opt = vae.arena, tr.optimizer
    inside = _inside(a, cuda)
    pick = _sample(a.trainable_ranges(), cuda)
    steps = []
    for s in range(1, 5):
        lr = opt.param_groups[0]["lr"]
        x, eps = _batch(g["B"], g["R"], s, cuda)
        prev = a.flat.clone()
        m0 = opt.exp_avg.clone() if opt.exp_avg is not None else torch.zeros_like(prev)
        v0 = opt.exp_avg_sq.clone() if opt.exp_avg_sq is not None else torch.zeros_like(prev)
        res = tr.train_step(x, eps)
        sc = res["scalars"].cpu().tolist()
        grad = a.grad
        sq64 = float((grad[inside].double() ** 2).sum())
        rec = {"rec": sc[0], "kl": sc[1], "total": sc[2], "grad_norm": opt.grad_norm().item(), "lr": lr, "sq64": sq64,
               "frozen_unchanged": torch.equal(_bits(a.flat[~inside]), _bits(prev[~inside])),
               "frozen_moments_zero": bool((opt.exp_avg[~inside] == 0).all()) and bool((opt.exp_avg_sq[~inside] == 0).all()),
               "frozen_grad_none": all((p.grad is None) != p.requires_grad for p in vae.parameters()),
               "moved": float((a.flat[inside] - prev[inside]).abs().max())}
        args = (1.0, lr, sr.ADAM["betas"], sr.ADAM["eps"], sr.ADAM["wd"], s)
        sub = [t[pick].cpu() for t in (prev, grad, m0, v0)]
        p64, m64, v64 = sr.adamw_ref64(*sub, sq64, *args)
        # torch's own fp32 step on the same elements; its clip coefficient must come from the whole trainable gradient, so the
        # gradient is clipped here in float64 and handed over with clipping off
        gc = (sub[1].double() * sr.clip_coef64(sq64, 1.0)).float()
        pt, mt, vt = sr.adamw_torch32(sub[0], gc, sub[2], sub[3], 0.0, *args[1:])
        rec["update"] = (sr.update_error(a.flat[pick], p64, sub[0]), sr.update_error(pt, p64, sub[0]))
        rec["m"] = (sr.rel(opt.exp_avg[pick], m64), sr.rel(mt, m64))
        rec["v"] = (sr.rel(opt.exp_avg_sq[pick], v64), sr.rel(vt, v64))
        steps.append(rec)
    _RUNS[which] = (g, w, tr, steps)
    return _RUNS[which]


@pytest.mark.parametrize("which", SETS)
def test_step_moves_the_trainable_weights_and_nothing_else(cuda, which):
    """per step: frozen weights bitwise unchanged (one of them a nudged GroupNorm scale), their moments 0, their .grad None;
    the trainable ones against the float64 AdamW of tests/streaming_refs.py on the device's own gradients with the float64 norm
    over the trainable ranges, at the bars tests/test_streaming_edges_gpu.py holds vae_adamw to"""
    g, w, tr, steps = _run(which, cuda)
    for s, r in enumerate(steps, start=1):
        key = f"{which},step={s}"
        assert r["frozen_unchanged"] and r["frozen_moments_zero"] and r["frozen_grad_none"], (key, r)
        assert (r["moved"] > 0) == (r["lr"] > 0), (key, r["moved"], r["lr"])
        assert abs(r["grad_norm"] - r["sq64"] ** 0.5) <= 1e-5 * r["sq64"] ** 0.5, key
        got, cpu = r["update"]
        sr.check("adamw_ranges", key + ",p_update", got, 2 * cpu, cpu, strict=False)
        for name in ("m", "v"):
            got, cpu = r[name]
            sr.check("adamw_ranges", f"{key},{name}", got, sr.bar(4, cpu, 1e-6), cpu)


TOL_TRAJECTORY = 1e-4  # twice the oracle's own fp32-vs-float64 drift on this scenario (4.6e-5 at worst, `encoder`), never below 1e-4


@pytest.mark.parametrize("which", SETS)
def test_trajectory_matches_the_oracle_with_the_same_parameters_frozen(cuda, which):
    import vae_oracle as vo
    g, w, tr, steps = _run(which, cuda)
    o = vo.OracleWrapper(seed=42)
    if NUDGED[which]:
        with torch.no_grad():
            dict(o.vae.named_parameters())[NUDGED[which]].mul_(1.05)
    trainable = {n for n, p in w.vae.named_parameters() if p.requires_grad}
    for n, p in o.vae.named_parameters():
        p.requires_grad_(n in trainable)
    ot = vo.OracleTrainer(o, lr=g["lr"], warmup=g["warmup"], max_steps=g["max_steps"], kl_weight=g["kl_weight"], max_grad_norm=1.0)
    for s, got in enumerate(steps, start=1):
        ref = ot.step(vo.synthetic_pixels(g["B"], g["R"], 42, s), vo.synthetic_eps(g["B"], g["R"], 42, s))
        for k in ("rec", "kl", "total", "grad_norm"):
            err = abs(got[k] - ref[k]) / abs(ref[k])
            print(f"{which} step {s} {k}: device {got[k]:.8g} oracle {ref[k]:.8g} rel {err:.2e}")
            assert err <= TOL_TRAJECTORY, (which, s, k, got[k], ref[k])
        assert got["lr"] == pytest.approx(ref["lr"], rel=1e-12, abs=1e-15)


def test_decoder_only_step_keeps_no_encoder_activation(cuda):
    from vaehip.trainer import HipTrainer
    w = _wrapper(cuda)
    tr = HipTrainer(w, max_train_steps=20)
    x, eps = _batch(2, 64, 1, cuda)
    peak = {}
    for rnd in ("warm", "measured"):  # the first step of either kind allocates optimizer state and tables
        for which in ("all", "decoder"):
            tr.set_trainable(which)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tr.train_step(x, eps)
            torch.cuda.synchronize()
            peak[which] = torch.cuda.max_memory_allocated() - base
            tr.last = None
    print("peak above the resident state, bytes:", peak)
    assert peak["decoder"] < peak["all"]


def test_checkpointed_decoder_with_encoder_trainable_is_bitwise_the_same(full):
    from vaehip.trainable import apply_trainable
    g, w, x, eps, ref, ref_grad = full
    vae = w.vae
    try:
        apply_trainable(vae, "encoder")
        vae.engine.checkpoint_decoder = True
        vae.arena.grad.fill_(float("nan"))
        res = vae.engine.forward_backward(x, eps, g["kl_weight"])
        _compare_grads(vae, ref_grad, ref, res, "encoder, checkpointed decoder")
    finally:
        vae.engine.checkpoint_decoder = False
        vae.requires_grad_(True)


def test_accumulated_micro_batches_with_decoder_trainable(cuda):
    """two B = 1 micro-batches against the B = 2 step, at the bar of test_gradient_accumulation_equals_full_batch_step"""
    from vaehip.trainer import HipTrainer
    x, eps = _batch(2, 32, 3, cuda)
    params, gnorm, w0 = {}, {}, None
    for accum in (1, 2):
        w = _wrapper(cuda)
        w0 = w.vae.arena.flat.clone()
        tr = HipTrainer(w, lr=1e-3, kl_weight=1e-3, lr_warmup_steps=1, max_train_steps=10, gradient_accumulation_steps=accum,
                        trainable="decoder")
        for it in range(2):
            if accum == 1:
                tr.train_step(x, eps)
            else:
                tr.train_step(x[:1], eps[:1])
                assert not tr.sync_gradients
                with pytest.raises(RuntimeError, match="pending"):
                    tr.set_trainable("all")
                tr.train_step(x[1:], eps[1:])
            assert tr.sync_gradients and tr.global_step == it + 1
        params[accum], gnorm[accum] = w.vae.arena.flat.clone(), float(tr.optimizer.grad_norm())
        frozen = ~_inside(w.vae.arena, cuda)
        assert torch.equal(_bits(params[accum][frozen]), _bits(w0[frozen]))
    assert abs(gnorm[1] - gnorm[2]) / gnorm[1] < 1e-5
    moved = float((params[1] - w0).abs().max())
    assert moved > 0 and float((params[1] - params[2]).abs().max()) < 2e-2 * moved


def test_weight_average_of_a_frozen_element_is_the_element(cuda):
    from vaehip.trainer import HipTrainer
    g = _golden()
    w = _wrapper(cuda)
    tr = HipTrainer(w, lr=g["lr"], lr_warmup_steps=0, max_train_steps=10, kl_weight=g["kl_weight"], trainable="decoder", use_ema=True,
                    ema_decay=0.5)
    for s in (1, 2, 3):
        tr.train_step(*_batch(2, 32, s, cuda))
    a = w.vae.arena
    inside = _inside(a, cuda)
    with torch.no_grad():
        w.vae.encoder.down_blocks[0].resnets[0].norm1.weight.mul_(1.05)  # a nudge of a frozen scale after the average started
    live, ema = a.flat.clone(), tr.optimizer.ema.clone()
    assert not torch.equal(live[inside], ema[inside])
    with tr.ema_weights():
        assert torch.equal(_bits(a.flat[~inside]), _bits(live[~inside]))   # frozen: the live weights, the nudge included
        assert torch.equal(_bits(a.flat[inside]), _bits(ema[inside]))      # trainable: the average
    assert torch.equal(_bits(a.flat), _bits(live)) and torch.equal(_bits(tr.optimizer.ema), _bits(ema))


def test_state_round_trip_continues_bitwise_and_refuses_another_set(cuda):
    from vaehip.trainer import HipTrainer
    g = _golden()
    kw = dict(lr=g["lr"], lr_warmup_steps=0, max_train_steps=10, kl_weight=g["kl_weight"], use_ema=True)
    w = _wrapper(cuda)
    tr = HipTrainer(w, trainable="decoder", **kw)
    for s in (1, 2):
        tr.train_step(*_batch(2, 32, s, cuda))
    sd = tr.state_dict()
    weights = {k: v.detach().clone() for k, v in w.vae.state_dict().items()}
    w2 = _wrapper(cuda)
    w2.vae.load_state_dict(weights)
    with pytest.raises(ValueError, match="trainable"):
        HipTrainer(w2, trainable="encoder", **kw).load_state_dict(sd)
    tr2 = HipTrainer(w2, trainable="decoder", **kw)
    tr2.load_state_dict(sd)
    for t in (tr, tr2):
        t.train_step(*_batch(2, 32, 3, cuda))
    assert torch.equal(_bits(w.vae.arena.flat), _bits(w2.vae.arena.flat))
    assert torch.equal(_bits(tr.optimizer.exp_avg), _bits(tr2.optimizer.exp_avg))
    inside = _inside(w.vae.arena, cuda)
    assert torch.equal(_bits(tr.optimizer.ema[inside]), _bits(tr2.optimizer.ema[inside]))


def test_autograd_path_honours_requires_grad(full, cuda):
    """vae.encoder.requires_grad_(False) as in the reference, loss.backward() through SDXLVAEWrapper.forward, stock AdamW"""
    g, wf, x, eps, ref, ref_grad = full
    w = _wrapper(cuda)
    vae = w.vae
    vae.encoder.requires_grad_(False)
    vae.quant_conv.requires_grad_(False)
    opt = torch.optim.AdamW([p for p in vae.parameters() if p.requires_grad], lr=1e-4)
    out = w(x, sample_posterior=False)
    rec = torch.nn.functional.mse_loss(out["reconstruction"].float(), x, reduction="mean")
    loss = rec + g["kl_weight"] * out["latent_dist"].kl().mean()
    loss.backward()
    # the fused path on the same weights, set and input (deterministic latents: the posterior mean)
    w2 = _wrapper(cuda)
    w2.vae.encoder.requires_grad_(False)
    w2.vae.quant_conv.requires_grad_(False)
    w2.vae.engine.forward_backward(x, None, g["kl_weight"], sample_posterior=False)
    for (n, p), (_n2, p2) in zip(vae.named_parameters(), w2.vae.named_parameters()):
        if n.startswith("encoder.") or n.startswith("quant_conv."):
            assert p.grad is None and p2.grad is None, n
        else:
            assert p.grad is not None and torch.equal(_bits(p.grad.contiguous()), _bits(p2.grad.contiguous())), n
    before = vae.arena.flat.clone()
    opt.step()
    inside = _inside(vae.arena, cuda)
    assert torch.equal(_bits(vae.arena.flat[~inside]), _bits(before[~inside])) and not torch.equal(vae.arena.flat[inside], before[inside])
