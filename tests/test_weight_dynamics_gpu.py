"""ops.weight_dynamics (csrc/wdyn.hip): six sums and max |w| per output slice and per input slice of every tensor of a table, in
one read of the parameter, gradient and Adam-moment arenas, against the float64 references and the derived bounds of
tests/wdyn_refs.py (max |w| bit for bit); then the WeightDynamicsTracker on the small synthetic VAE (every default target against
the references of copies of the four arenas, the update identity, nothing changed by tracking, a frozen encoder); then
src/train.py on configs/experiment_synthetic_weight_dynamics.yaml."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wdyn_refs as R
from guarded import GuardedPool, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 32768  # vae_wdyn_chunk(), asserted below
SHAPES = [(1, 1, 1), (5, 1, 1), (3, 1, 7), (4, 1, 8), (2, 9, 3), (3, 9, 4), (5, 9, 5), (8, 9, 64), (2, 1, 260), (130, 1, 4),
          (2, 1, CHUNK + 4)]
HP = (0.9, 0.999, 1e-8, 3)  # beta1, beta2, eps, step
PAD = 1e6


def _consts(hp=HP):
    from tracking.weightdynamics import adam_constants
    return adam_constants(*hp)


def _arenas(cuda, entries, total, seed, plant=None):
    """four arenas of `total` elements, 1e6 everywhere except the listed tensors (name, off, O, K, I), which hold draw()'s
    values; plant(name, w) may edit a tensor's weights.  -> (device arenas [w, g, m, v], {name: host (w, g, m, v)})"""
    host = [np.full(total, PAD, dtype=np.float32) for _ in range(4)]
    vals = {}
    for n, (name, off, O, K, I) in enumerate(entries):
        t = list(R.draw((O, K, I), seed + 17 * n))
        if plant is not None:
            plant(name, t[0])
        vals[name] = tuple(t)
        for a, x in zip(host, t):
            a[off:off + O * K * I] = x.ravel()
    return [torch.from_numpy(a).to(cuda) for a in host], vals


def _check_all(table, res, vals, mode, skip=None):
    out_sums, in_sums, out_amax, in_amax = (t.cpu().numpy() for t in res)
    assert out_sums.dtype == np.float64 and out_sums.shape == (table.n_out, 6) and in_sums.shape == (table.n_in, 6)
    assert out_amax.dtype == np.float32 and out_amax.shape == (table.n_out,) and in_amax.shape == (table.n_in,)
    worst = 0.0
    for s in table.slots:
        w, g, m, v = vals[s.name]
        r = R.ref(w, g if mode >= 1 else None, m if mode >= 2 else None, v if mode >= 2 else None, _consts())
        bd = R.bounds(r, s.O, s.K, s.I, CHUNK)
        sk = (skip or {}).get(s.name, {})
        worst = max(worst, R.check(out_sums[table.out_slice(s)], out_amax[table.out_slice(s)], r["out"], bd["out"], mode, sk.get("out", ())))
        assert ("in" in r) == (s.I > 1)
        if s.I > 1:
            worst = max(worst, R.check(in_sums[table.in_slice(s)], in_amax[table.in_slice(s)], r["in"], bd["in"], mode, sk.get("in", ())))
    return worst


def _run(arenas, table, mode, hp=HP):
    from vaehip import ops
    w, g, m, v = arenas
    return ops.weight_dynamics(w, g if mode >= 1 else None, m if mode >= 2 else None, v if mode >= 2 else None, table, *hp)


def _same(x, y):
    return all(torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32)) for a, b in zip(x, y))


# ---------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("O,K,I", SHAPES)
def test_sweep_within_the_derived_bounds(cuda, O, K, I, mode):
    from vaehip.lib import lib
    from vaehip.weight_table import WeightTable
    assert lib.query("vae_wdyn_chunk") == CHUNK
    entries = [("t", 8, O, K, I)]
    total = 8 + O * K * I + 8
    table = WeightTable.from_entries(entries, total, cuda)
    arenas, vals = _arenas(cuda, entries, total, O * 1000 + K * 37 + I)
    res = _run(arenas, table, mode)
    worst = _check_all(table, res, vals, mode)
    assert _same(res, _run(arenas, table, mode))  # two calls agree bit for bit
    print(f"[{O}][{K}][{I}] mode {R.MODES[mode]}: worst error / bound {worst:.3f}, chains {R.chains(O, K, I, CHUNK)}")


@pytest.mark.parametrize("O,K,I", SHAPES)
def test_max_abs_with_a_planted_nan_and_inf(cuda, O, K, I):
    """-inf in the first element, a NaN in the last (alone: the NaN): max |w| of their slices is +inf / the canonical NaN bit
    for bit, every other slice keeps its sums within bound"""
    from vaehip.weight_table import WeightTable

    def plant(name, w):
        w[0, 0, 0] = -np.inf
        w[-1, -1, -1] = np.nan
    entries = [("t", 8, O, K, I)]
    total = 8 + O * K * I + 8
    table = WeightTable.from_entries(entries, total, cuda)
    arenas, vals = _arenas(cuda, entries, total, 5 + O + K + I, plant)
    res = _run(arenas, table, 2)
    _check_all(table, res, vals, 2, {"t": {"out": (0, O - 1), "in": (0, I - 1)}})
    amax = res[2].cpu().numpy()
    assert amax.view(np.uint32)[O - 1] == 0x7FC00000 and (O == 1 or np.isposinf(amax[0]))
    assert np.isfinite(amax[1:O - 1]).all()
    if I > 1:
        imax = res[3].cpu().numpy()
        assert imax.view(np.uint32)[I - 1] == 0x7FC00000 and np.isposinf(imax[0]) and np.isfinite(imax[1:I - 1]).all()


MIXED = [("c3", 9, 64), ("g5", 5, 1, 1), ("lin", 130, 1, 4), ("skip_a", 40, 1, 1), ("s3", 2, 9, 3), ("one", 1, 1, 1), ("skip_b", 4, 9, 8),
         ("wide", 2, 1, 260), ("c5", 5, 9, 5), ("v4", 3, 9, 4), ("l7", 3, 1, 7), ("l8", 4, 1, 8)]


def _mixed_entries():
    """tensors laid out in memory in MIXED's order with gaps between them; the table lists them (without the skip_*) in another"""
    off, placed = 4, {}
    for e in MIXED:
        name, shape = e[0], ((8,) + e[1:] if len(e) == 3 else e[1:])
        placed[name] = (name, off) + tuple(shape)
        off += (int(np.prod(shape)) + 5 + 3) // 4 * 4  # a gap of at least five elements
    order = ["l7", "wide", "c3", "one", "g5", "v4", "s3", "lin", "c5", "l8"]
    return [placed[n] for n in order], off + 8


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_mixed_table_in_guarded_memory(cuda, mode):
    """a table of all the sweep's paths, listed out of memory order with unlisted tensors and gaps (1e6 in all four arrays)
    between them, operands, workspace and results in guarded, poisoned blocks: nothing leaks into a sum, no store outside a
    block, no operand changed, every result word written"""
    from vaehip import ops
    from vaehip.weight_table import WeightTable
    entries, total = _mixed_entries()
    table = WeightTable.from_entries(entries, total, cuda)
    assert table.nseg == 10 and [s.off for s in table.slots] != sorted(s.off for s in table.slots)
    arenas, vals = _arenas(cuda, entries, total, 900)
    pool = GuardedPool(cuda)
    arenas = [pool.put(a, n) for a, n in zip(arenas, "wgmv")]
    pool.snapshot()
    with guarded(pool, ops):
        res = _run(arenas, table, mode)
    torch.cuda.synchronize()
    assert len(pool.blocks) == 4 + 5  # the operands, the workspace and four results
    assert pool.violations() == [] and pool.changed() == []
    ws = [b for b in pool.blocks if b.tensor.dtype == torch.int32]
    assert len(ws) == 1 and ws[0].tensor.numel() == table.nwords
    # every result word is written; of the workspace, every word of the mode's sums (mode 2: all of it)
    assert pool.unwritten_report(skip=() if mode == 2 else tuple(ws)) == []
    for t in res:
        pool.block_of(t)
        assert float(torch.nan_to_num(t.double(), nan=0.0).abs().max()) < 1e4  # 1e6^2 from a gap would show
    worst = _check_all(table, res, vals, mode)
    print(f"mixed table, mode {R.MODES[mode]}: worst error / bound {worst:.3f}")


def test_argument_errors_are_refused_with_their_message(cuda):
    import ctypes as C
    from vaehip import ops
    from vaehip.lib import lib, VaeHipError
    from vaehip.weight_table import WeightTable
    entries, total = [("a", 8, 4, 9, 8), ("b", 400, 5, 1, 1)], 512
    table = WeightTable.from_entries(entries, total, cuda)
    arenas, vals = _arenas(cuda, entries, total, 31)
    w, g, m, v = arenas
    ws = torch.full((table.nwords + 4,), -1, device=cuda, dtype=torch.int32)
    osum = torch.full((table.n_out, 6), -1.0, device=cuda, dtype=torch.float64)
    isum = torch.full((table.n_in, 6), -1.0, device=cuda, dtype=torch.float64)
    oa, ia = torch.full((table.n_out,), -1.0, device=cuda), torch.full((table.n_in,), -1.0, device=cuda)
    p = ops._p

    def partial(wp=p(w), gp=p(g), mp=p(m), vp=p(v), tab=p(table.tab), nseg=table.nseg, nchunk=table.nchunk, n_out=table.n_out, step=3,
                wsp=p(ws), os_=p(osum), oa_=p(oa)):
        lib.call("vae_wdyn_partial", wp, gp, mp, vp, tab, nseg, nchunk, n_out, 0.9, 0.999, 1e-8, step, wsp, os_, oa_, ops._stream())

    def final(wsp=p(ws), tab=p(table.tab), nseg=table.nseg, n_in=table.n_in, mode=2, is_=p(isum), ia_=p(ia)):
        lib.call("vae_wdyn_final", wsp, tab, nseg, n_in, mode, is_, ia_, ops._stream())

    for kw, msg in [(dict(wp=None), "null args"), (dict(tab=None), "null args"), (dict(wsp=None), "null args"), (dict(os_=None), "null args"),
                    (dict(oa_=None), "null args"), (dict(vp=None), "modes are"), (dict(mp=None), "modes are"), (dict(gp=None), "modes are"),
                    (dict(nseg=0), "counts do not add up"), (dict(nseg=-1), "counts do not add up"),
                    (dict(nchunk=1), "counts do not add up"), (dict(n_out=1), "counts do not add up"),
                    (dict(wp=w.data_ptr() + 4), "unaligned"), (dict(gp=g.data_ptr() + 8), "unaligned"), (dict(mp=m.data_ptr() + 4), "unaligned"),
                    (dict(vp=v.data_ptr() + 4), "unaligned"), (dict(wsp=ws.data_ptr() + 4), "unaligned"),
                    (dict(tab=table.tab.data_ptr() + 8), "unaligned"), (dict(step=0), "step=0 with Adam moments")]:
        with pytest.raises(VaeHipError, match="wdyn_partial.*" + msg):
            partial(**kw)
    for kw, msg in [(dict(wsp=None), "null args"), (dict(tab=None), "null args"), (dict(is_=None), "null args"), (dict(ia_=None), "null args"),
                    (dict(nseg=0), "counts do not add up"), (dict(n_in=-1), "counts do not add up"), (dict(mode=3), "counts do not add up"),
                    (dict(wsp=ws.data_ptr() + 4), "unaligned")]:
        with pytest.raises(VaeHipError, match="wdyn_final.*" + msg):
            final(**kw)
    bad = table.host.clone()
    bad[1, 0] = 402  # an offset that is no multiple of 4: refused where the table is checked
    out = [C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)]
    with pytest.raises(VaeHipError, match="wdyn_workspace.*multiple of 4"):
        lib.call("vae_wdyn_workspace", C.c_void_p(bad.data_ptr()), 2, *[C.byref(o) for o in out])
    torch.cuda.synchronize()
    # nothing was launched by any of them
    assert all(bool((t == -1).all()) for t in (ws, osum, isum, oa, ia))
    with pytest.raises(ValueError, match="modes are"):
        ops.weight_dynamics(w, None, m, v, table)
    with pytest.raises(ValueError, match="flat contiguous fp32 CUDA"):
        ops.weight_dynamics(w, g.double(), None, None, table)
    with pytest.raises(ValueError, match="the table reaches"):
        ops.weight_dynamics(w[:300], None, None, None, table)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.weight_dynamics(w[1:], None, None, None, WeightTable.from_entries(entries[:1], 300, cuda))
    with pytest.raises(ValueError, match="step 0 with Adam moments"):
        ops.weight_dynamics(w, g, m, v, table, step=0)
    # and the same arguments, valid, run
    partial()
    final()
    _check_all(table, (osum, isum, oa, ia), vals, 2)
    # step < 1 is no error without moments
    _check_all(table, ops.weight_dynamics(w, g, None, None, table, step=0), vals, 1)


# ---------------------------------------------------------------------------------------------------- engine
R_, B_, SEED = 32, 2, 7


def _setup(cuda, mode, **trainer_kw):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.trainer import HipTrainer
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), SEED))
    w.to(cuda)
    kw = dict(lr=1e-4, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mode)
    kw.update(trainer_kw)
    return w, HipTrainer(w, **kw)


def _batch(cuda, step):
    import vae_oracle as vo
    return vo.synthetic_pixels(B_, R_, 5, step).to(cuda), vo.synthetic_eps(B_, R_, 5, step).to(cuda)


def _host_arenas(w, tr):
    a, o = w.vae.arena, tr.optimizer
    return [t.detach().cpu().numpy().copy() for t in (a.flat, a.grad, o.exp_avg, o.exp_avg_sq)]


def _tensor_of(arena, p, host):
    from vaehip.weight_table import okI_of
    off, shape = arena.offset_of[id(p)], okI_of(p.shape)
    return host[off:off + p.numel()].reshape(shape)


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_default_targets_against_the_references(cuda, mode):
    from tracking.weightdynamics import METRICS, WeightDynamicsTracker, derive
    w, tr = _setup(cuda, mode)
    for s in (1, 2):
        tr.train_step(*_batch(cuda, s))
    wdt = WeightDynamicsTracker({"enabled": True})
    logs = wdt.track(w, tr.optimizer, 2)
    host = _host_arenas(w, tr)
    g0 = tr.optimizer.param_groups[0]
    consts = _consts((g0["betas"][0], g0["betas"][1], g0["eps"], 2))
    named = dict(w.vae.named_parameters())
    want = [n for n, p in named.items() if p.dim() in (1, 2, 4)]
    assert sorted(wdt.last_raw) == sorted(want) and len(want) > 100 and tr.optimizer.step_count == 2
    worst = 0.0
    for n in want:
        p = named[n]
        t = [_tensor_of(w.vae.arena, p, h) for h in host]
        r = R.ref(*t, consts)
        bd = R.bounds(r, *t[0].shape, CHUNK)
        assert sorted(wdt.last_raw[n]) == sorted(r)
        for view in r:
            sums, amax = wdt.last_raw[n][view]
            worst = max(worst, R.check(sums, amax.astype(np.float32), r[view], bd[view], 2))
            vals = derive(sums, amax, wdt.last_lr)
            for metric in METRICS:  # the history holds exactly the derived vectors
                (step, vec), = wdt.history[(n, view, metric)]
                assert step == 2 and np.array_equal(vec, vals[metric], equal_nan=True) and np.isfinite(vec).all(), (n, view, metric)
                assert logs[f"weight_dynamics/{n}/{view}/{metric}_max"] == float(vec.max())
    assert wdt.last_lr == tr.optimizer.last_lr and wdt.last_lr > 0
    print(f"{mode}: {len(want)} parameters, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_update_identity(cuda, mode):
    """lr sqrt(S_uu) of a row is the norm of the Adam part of the update just applied: w' - w (1 - lr wd)"""
    from tracking.weightdynamics import WeightDynamicsTracker
    w, tr = _setup(cuda, mode, lr=1e-2)
    tr.train_step(*_batch(cuda, 1))
    before = w.vae.arena.flat.detach().cpu().numpy().copy()
    tr.train_step(*_batch(cuda, 2))
    wdt = WeightDynamicsTracker({"enabled": True, "views": ["out"]})
    wdt.track(w, tr.optimizer, 2)
    host = _host_arenas(w, tr)
    g0 = tr.optimizer.param_groups[0]
    lr, wd = tr.optimizer.last_lr, g0["weight_decay"]
    assert lr > 1e-3 and wd > 0
    consts = _consts((g0["betas"][0], g0["betas"][1], g0["eps"], 2))
    worst, checked, far, rows = 0.0, 0, 0, 0
    for n, p in w.vae.named_parameters():
        if n not in wdt.last_raw:
            continue
        wb = _tensor_of(w.vae.arena, p, before)
        wa, g, m, v = (_tensor_of(w.vae.arena, p, h) for h in host)
        r = R.ref(wa, g, m, v, consts)["out"]
        n_out, _ = R.chains(*wa.shape, CHUNK)
        delta = wa.astype(np.float64) - wb.astype(np.float64) * (1.0 - lr * wd)
        lhs = np.sqrt((delta * delta).sum(axis=(1, 2)))
        rhs = lr * np.sqrt(wdt.last_raw[n]["out"][0][:, 5])
        bound = R.update_identity_bound(wb, wa, lr, r["sums"][:, 5], r["scale"][:, 5], n_out)
        err = np.abs(lhs - rhs)
        assert (err <= bound).all(), (n, np.argwhere(err > bound)[:4], err.max(), bound.max())
        far += int((rhs > 100 * bound).sum())
        rows += rhs.size
        worst, checked = max(worst, float((err / bound).max())), checked + 1
    assert checked > 100
    assert far >= 0.9 * rows, (far, rows)  # the update stands far above the bound: the identity is not vacuous
    print(f"{mode}: update identity over {checked} parameters, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("mode", ["no", "bf16"])
def test_engine_parameters_are_bitwise_the_same_with_the_tracker(cuda, mode):
    from tracking.weightdynamics import WeightDynamicsTracker
    flats = []
    for tracked in (False, True):
        w, tr = _setup(cuda, mode)
        wdt = WeightDynamicsTracker({"enabled": True}) if tracked else None
        for s in (1, 2, 3):
            tr.train_step(*_batch(cuda, s))
            if wdt:
                wdt.track(w, tr.optimizer, s)
        flats.append([t.clone() for t in (w.vae.arena.flat, w.vae.arena.grad, tr.optimizer.exp_avg, tr.optimizer.exp_avg_sq)])
    for a, b in zip(*flats):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_engine_frozen_encoder_reports_weights_only(cuda):
    from tracking.weightdynamics import METRICS, WEIGHT_METRICS, WeightDynamicsTracker
    w, tr = _setup(cuda, "no", trainable="decoder")
    for p in w.vae.parameters():  # a frozen parameter's gradient slot may hold anything
        if not p.requires_grad:
            w.vae.arena.grad_view(p).fill_(1e6)
    for s in (1, 2):
        tr.train_step(*_batch(cuda, s))
    wdt = WeightDynamicsTracker({"enabled": True})
    wdt.track(w, tr.optimizer, 2)
    seen = {True: 0, False: 0}
    for (n, view, metric), hist in wdt.history.items():
        vec = hist[0][1]
        frozen = n.startswith("encoder.") or n.startswith("quant_conv.")
        assert frozen == (not dict(w.vae.named_parameters())[n].requires_grad)
        if frozen and metric not in WEIGHT_METRICS:
            assert np.isnan(vec).all(), (n, view, metric)
        else:
            assert np.isfinite(vec).all(), (n, view, metric)
        seen[frozen] += 1
    assert seen[True] > 100 and seen[False] > 100 and len(METRICS) == 6


# ---------------------------------------------------------------------------------------------------- CLI
def test_train_cli_with_the_weight_dynamics_config(cuda, tmp_path):
    """src/train.py with configs/experiment_synthetic_weight_dynamics.yaml writes weight_dynamics_history.csv with one row per
    (tracked step, parameter, view, metric); gamma's update ratio is finite at every tracked step"""
    import yaml
    src = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
    c = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_weight_dynamics.yaml")))
    c["output_dir"] = str(tmp_path)
    c["data"]["dataset_name"] = "synthetic:48"  # 6 steps/epoch x 2 epochs: the tracker fires at steps 5 and 10
    c["data"]["resolution"] = 32
    assert c["weight_dynamics"]["track_interval"] == 5 and c["intervention"]["enabled"]
    cpath = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(c, open(cpath, "w"))
    env = dict(os.environ, PYTHONPATH=src)
    r = subprocess.run([sys.executable, os.path.join(src, "train.py"), "--config_path", cpath], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = list(csv.DictReader(open(tmp_path / c["run_name"] / "weight_dynamics_history.csv")))
    res = "decoder.up_blocks.1.resnets.0."
    views = {res + "conv1.weight": ("out", "in"), res + "norm2.weight": ("out",), res + "conv2.weight": ("out", "in")}
    assert [p[4:] for p in c["weight_dynamics"]["target_parameters"]] == list(views)
    want = sorted((s, p, v, m) for s in (5, 10) for p, vs in views.items() for v in vs for m in c["weight_dynamics"]["metrics"])
    assert sorted((int(x["global_step"]), x["parameter"], x["view"], x["metric"]) for x in rows) == want and len(want) == 60
    for x in rows:
        vec = np.array(json.loads(x["metric_value"]))
        assert len(vec) == int(x["num_channels"]) and np.isfinite(vec).all() and float(x["max"]) == vec.max()
        if x["parameter"].endswith("norm2.weight") and x["metric"] == "update_ratio_per_channel":
            assert (vec > 0).all() and float(x["min"]) > 0
    chans = {(x["parameter"], x["view"]): int(x["num_channels"]) for x in rows}
    # the rows of conv1, gamma and the columns of conv2 are the same channels
    assert chans[(res + "conv1.weight", "out")] == chans[(res + "norm2.weight", "out")] == chans[(res + "conv2.weight", "in")]
    metrics = [json.loads(line) for line in open(tmp_path / c["run_name"] / "metrics.jsonl")] \
        if os.path.exists(tmp_path / c["run_name"] / "metrics.jsonl") else []
    if metrics:
        assert any(f"weight_dynamics/{res}norm2.weight/out/update_ratio_per_channel_max" in json.dumps(m) for m in metrics)
