"""conv3_tile_bf16_kernel, conv3_wide_bf16_kernel and conv1_bf16_kernel at the ends of their loops, against float64.

Every case of tests/bf16_tile_refs.py::CASES (the table says which line of which kernel a case is there for; the host module
tests/test_bf16_tile_edges_host.py holds the table, the restated plans and the reference without a GPU) is launched through the
library entry under ops.LaunchProfiler, into NaN-prefilled outputs:

  * the kernel-name list is exactly the case's instantiation;
  * every element is finite, and bf16_refs.ratio(stage) <= 1 with NO element left out: fp32 result max|got - v| <= bar max|v|, bf16
    result every element |got - v| <= ulp_bf16(v) / 2 + bar max|v|, bar = bf16_refs.BAR_DIRECT (2e-5); epilogue statistics within
    BAR_STATS (1e-5) of a separate gn_stats pass over the stored tensor; the tracker within 1e-5 (test_conv_track_epilogue's bar)
    of the float64 mean |v|; a fused transform's operand is the device's own gn_apply_bf16, held to float64 at BAR_GN_APPLY;
  * a ragged N with ldc > N leaves the columns at and beyond N untouched;
  * in guarded, poisoned memory (tests/guarded.py): no guard byte and no operand changed, nothing unwritten, the same bits;
  * twenty launches give the same bits;
  * library options: no_wide within BAR_DIRECT (another kernel, another order of sums), wide_reserved_cus = 24 bitwise;
  * ops.conv_fwd / ops.conv_dgrad, where they route the shape, give the same bits as the direct launch.

The worst ratio per case is printed and recorded with the suite's other measured figures (test_engine_gpu._record, kind
"bf16_tile_edges"); profiles/bf16_tile_edges_measured.json is that record of a run on MI355X."""
import ctypes as C
import time

import pytest
import torch

import bf16_tile_refs as R
import guarded as G

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ops(cuda):
    from vaehip import ops as o
    return o


def _record(key, value):
    from test_engine_gpu import _record as rec
    rec("bf16_tile_edges", key, value)


class Launch:
    """the case's operands on the device (from a guarded pool when one is given), its NaN-prefilled outputs and its block"""

    def __init__(self, c, ops, pool=None, ldc=0):
        self.c, self.ops, self.pool = c, ops, pool
        inp = R.inputs(c.name)
        self.x = self._put(inp["x"].contiguous(), "x")
        self.w = self._put(inp["w"].permute(0, 2, 3, 1).contiguous(), "w")   # OHWI memory
        self.wh = self._put(torch.zeros(self.w.shape, dtype=torch.bfloat16), "wh")
        ops.pack_bf16(self.w, self.wh)
        self.opt = {k: self._put(inp[k].contiguous(), k) for k in ("bias", "res", "scale", "shift") if k in inp}
        B, Ho, Wo, N = R.out_shape(c)
        odt = torch.bfloat16 if c.out16 else torch.float32
        if "res" in self.opt and ldc:
            raise ValueError("a residual has the output's row stride")
        self.full = self._out((B, Ho, Wo, ldc or N), odt, "out")
        self.a = a = R.args(c, ops, ldc)
        a.A, a.W, a.Wh, a.C = ops._p(self.x), ops._p(self.w), ops._p(self.wh), ops._p(self.full)
        if c.a == "a16" and c.fam != "conv1":
            a.A16 = ops._p(self.x)
        a.bias, a.res = ops._p(self.opt.get("bias")), ops._p(self.opt.get("res"))
        a.scale, a.shift = ops._p(self.opt.get("scale")), ops._p(self.opt.get("shift"))
        self.track = self.gstat = None
        if "t" in c.epi:
            self.track = self._out((a.M // 128, N), torch.float32, "track")
            a.track = ops._p(self.track)
        if "s" in c.epi:
            self.nch = int(ops.lib.query("vae_conv_gstat_chunks", C.byref(a)))
            assert self.nch == R.plan(c)["gstat_chunks"] > 0
            self.gstat = self._out((B, self.nch, 32, 2), torch.float32, "gstat")
            a.gstat = ops._p(self.gstat)
        if pool is not None:
            pool.snapshot()   # everything handed out so far, outputs included: `changed` is asked for the operands' labels

    def _put(self, t, label):
        return self.pool.put(t, label) if self.pool is not None else t.cuda()

    def _out(self, shape, dtype, label):
        if self.pool is not None:
            return self.pool.alloc(shape, dtype, fill=None, label=label)   # the poison is a NaN in every dtype
        return torch.full(shape, NAN, device="cuda", dtype=dtype)

    @property
    def out(self):
        return self.full[..., :self.c.N]

    def run(self):
        """-> the kernel names of the launch (four for a phase set)"""
        c, a, ops = self.c, self.a, self.ops
        prof = ops.PROFILER = ops.LaunchProfiler()
        try:
            if c.form != "phase":
                ops._launch_igemm(a)
            else:
                for ph, (pa, pb) in enumerate(R.PHASES):
                    a.tapmask = R.tapmask(pa, pb)
                    if c.dgrad:   # the phases add up through the residual input (ops._upconv_phase_dgrad)
                        a.a_oy, a.a_ox, a.res = pa, pb, (ops._p(self.full) if ph else None)
                    else:
                        a.c_oy, a.c_ox = pa, pb
                    ops._launch_igemm(a)
        finally:
            ops.PROFILER = None
        torch.cuda.synchronize()
        return [r[0] for r in prof.records]

    def expected_names(self):
        return [self.c.kernel] * (4 if self.c.form == "phase" else 1)


_DEVICE_ACT = {}


def _reference(c, L):
    """float64 value of the case; a fused transform's operand is the device's own gn_apply_bf16 (held to float64 by the caller)"""
    if c.a not in ("xf1", "xf2"):
        return R.reference(c)
    if c.name not in _DEVICE_ACT:
        ops = L.ops
        st = ops.Stats(None, None, L.opt["scale"], L.opt["shift"])
        _DEVICE_ACT[c.name] = ops.gn_apply_bf16(L.x, st, L.a.xf).cpu()
    return R.reference(c, _DEVICE_ACT[c.name])


_RESULT = {}   # case name -> the ordinary run's stored result (CPU), for the bitwise comparisons


def _ordinary(c, ops):
    if c.name not in _RESULT:
        L = Launch(c, ops)
        assert L.run() == L.expected_names()
        _RESULT[c.name] = L.out.cpu()
    return _RESULT[c.name]


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_case_against_float64(ops, c):
    t0 = time.time()
    L = Launch(c, ops)
    names = L.run()
    assert names == L.expected_names(), names
    got = L.out.cpu()
    _RESULT.setdefault(c.name, got)
    assert bool(torch.isfinite(got.float()).all()), f"{int((~torch.isfinite(got.float())).sum())} elements not written"
    v = _reference(c, L)
    entry = {"kernels": names, "plan": {k: v_ for k, v_ in R.plan(c).items()}, "regimes": list(c.regimes), "route": R.route(c)}
    if c.a in ("xf1", "xf2"):
        sa = R.Stage(c.name + ".act", "fused", R.transform64(c, R.inputs(c.name)), _DEVICE_ACT[c.name], "bf16", R.BAR_GN_APPLY, None)
        entry["ratio_act"] = R.ratio(sa)
        assert entry["ratio_act"] <= 1.0, entry
    entry["ratio"] = R.ratio(R.stage(c, got, v))
    entry["share_of_bar_used"] = R.br.bar_used(R.stage(c, got, v))   # (a bf16 result: what half an ulp does not explain)
    entry["rel"] = float((got.double() - v).abs().max() / v.abs().max())
    print(f"{c.name:20s} {names[0]:45s} ratio {entry['ratio']:.3f} bar used {entry['share_of_bar_used']:.3f} (max error {entry['rel']:.2e} of max|v|)")
    if L.gstat is not None:
        assert bool(torch.isfinite(L.gstat).all())
        y = L.full
        y._gstat = (L.gstat, 32, L.nch)
        g1, b0 = torch.ones(c.N, device="cuda"), torch.zeros(c.N, device="cuda")
        st_f, st_p = ops.gn_stats(y, g1, b0), ops.gn_stats(y.clone(), g1, b0)   # from the epilogue's moments / a pass over the stored tensor
        rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())  # noqa: E731
        entry["stats_mean"], entry["stats_rstd"] = rel(st_f.mean, st_p.mean), rel(st_f.rstd, st_p.rstd)
        print(f"{'':20s} statistics: mean {entry['stats_mean']:.2e} rstd {entry['stats_rstd']:.2e} (bar {R.BAR_STATS:.0e})")
        assert entry["stats_mean"] <= R.BAR_STATS and entry["stats_rstd"] <= R.BAR_STATS, entry
    if L.track is not None:
        assert bool(torch.isfinite(L.track).all()), "tracker rows not written"
        tr = ops.track_final(L.track, L.a.M).double().cpu()
        ref = v.abs().mean(dim=(0, 1, 2))
        entry["track"] = float(((tr - ref).abs() / ref).max())
        print(f"{'':20s} tracker: {entry['track']:.2e} (bar {R.BAR_TRACK:.0e})")
        assert entry["track"] <= R.BAR_TRACK, entry
    entry["seconds"] = round(time.time() - t0, 2)
    _record(c.name, entry)
    assert entry["ratio"] <= 1.0, entry


@pytest.mark.parametrize("name", R.LDC_PAD)
def test_columns_beyond_a_ragged_n_keep_their_prefill(ops, name):
    c = R.BY_NAME[name]
    L = Launch(c, ops, ldc=c.N + 8)
    assert L.run() == L.expected_names()
    pad = L.full[..., c.N:]
    assert bool(torch.isnan(pad.float()).all()), f"{int((~torch.isnan(pad.float())).sum())} elements beyond N written"
    assert torch.equal(L.out.cpu(), _ordinary(c, ops))   # the same values at another row stride


@pytest.mark.parametrize("name", R.GUARDED)
def test_guarded_memory(ops, name):
    c = R.BY_NAME[name]
    pool = G.GuardedPool("cuda")
    L = Launch(c, ops, pool=pool)
    outs = [t for t in (L.full, L.track, L.gstat) if t is not None]
    assert L.run() == L.expected_names()
    assert pool.violations() == []
    changed = [lab for lab in pool.changed() if not lab.startswith(("out", "track", "gstat"))]
    assert changed == [], changed
    assert pool.unwritten_report() == [] and all(pool.unwritten(t) == 0 for t in outs)
    assert torch.equal(L.out.cpu(), _ordinary(c, ops))


@pytest.mark.parametrize("name", R.REPEAT)
def test_twenty_launches_give_the_same_bits(ops, name):
    c = R.BY_NAME[name]
    first = _ordinary(c, ops)
    L = Launch(c, ops)
    for i in range(20):
        L.full.fill_(NAN)
        assert L.run() == L.expected_names()
        assert torch.equal(L.out.cpu(), first), f"launch {i} differs in {int((L.out.cpu() != first).sum())} elements"


@pytest.mark.parametrize("name", R.OPTIONS)
def test_library_options(ops, name):
    c = R.BY_NAME[name]
    first = _ordinary(c, ops)
    L = Launch(c, ops)
    with ops.option("wide_reserved_cus", 24):   # 232 workgroups: another deal of the same tiles, the same sums
        assert L.run() == L.expected_names()
    assert torch.equal(L.out.cpu(), first)
    L.full.fill_(NAN)
    with ops.option("no_wide"):                 # the 128-pixel kernel on the same images
        names = L.run()
    assert names == [f"conv3_tile_bf16_kernel<{'true' if c.dgrad else 'false'},false,0,true>"], names
    r = R.ratio(R.stage(c, L.out.cpu()))
    print(f"{c.name}: no_wide ratio {r:.3f}")
    _record(c.name + "|no_wide", {"ratio": r, "kernels": names})
    assert r <= 1.0


@pytest.mark.parametrize("name", R.OPS)
def test_ops_routes_the_case_to_the_same_bits(ops, name):
    c = R.BY_NAME[name]
    first = _ordinary(c, ops)
    L = Launch(c, ops)
    B, H, W = c.bhw
    kind = "c1" if c.fam == "conv1" else "c3"
    prev = ops.PRECISION, ops.WEIGHTS16
    ops.PRECISION, ops.WEIGHTS16 = ops.PREC_BF16, (L.w.data_ptr(), L.w.numel() * 4, L.wh.data_ptr())
    prof = ops.PROFILER = ops.LaunchProfiler()
    try:
        odt = torch.bfloat16 if c.out16 else torch.float32
        if c.dgrad:
            y = ops.conv_dgrad(L.x, L.w.permute(0, 3, 1, 2), kind, (H, W), out_dtype=odt)
        else:
            y = ops.conv_fwd(L.x, L.w.permute(0, 3, 1, 2), L.opt.get("bias"), kind, out_dtype=odt)
    finally:
        ops.PROFILER = None
        ops.PRECISION, ops.WEIGHTS16 = prev
    assert [r[0] for r in prof.records] == [c.kernel], [r[0] for r in prof.records]
    assert y.dtype == first.dtype and torch.equal(y.cpu(), first)
