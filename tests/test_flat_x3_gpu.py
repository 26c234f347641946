"""The vectorised fp32 flat kernels of csrc/igemm.hip through the ops entry points, against float64, at the smallest shapes where
the staging, the plane layout or the term list can go wrong: the 128 x 128 tile runs under the split-bf16 policy F32X3 (three bf16
planes per operand, six plane products on the bf16 matrix pipe, a K step of 16), the skinny tiles (N <= 32, or M <= 32 of a weight
gradient) keep exact fp32 products and are held to the same bars.  Every case asserts the kernel name the library reports.

Bars: conv_routes.BAR_DIRECT (2e-5, rows), BAR_WGRAD (3e-5), BAR_WGRAD_GN (5e-5, behind a fused GroupNorm), on the scale of the
float64 reference's max.  The error model behind them: tests/test_flat_x3_host.py.

Shapes the issue's list could not select as written, and what runs instead:
  * the parity-class stride-2 dgrad needs B H W / 4 to be a multiple of 128 (ops.dgrad_args): B = 2, 12 x 12 gives the PLAIN
    stride-2 dgrad (tested as such); the parity-class form is tested at the smallest map that selects it, B = 2, 16 x 16.
  * split-K: the plan gives npix / 256 splits at most; 60 pixels give one.  The smallest size with two: 1x1, B = 2, 16 x 16."""
import math

import pytest
import torch

import conv_routes as cr
from test_flat_x3_host import C_CRAFTED, crafted

pytestmark = pytest.mark.gpu
TF = {False: "false", True: "true"}


def rows_name(N, bkm, xf=0):
    return f"igemm_rows_kernel<{'128,32,4,1' if N <= 32 else '128,128,4,2'},{TF[bkm]},true,{xf}>"


def wgrad_name(M, N, xf=0):
    return f"wgrad_kernel<{'32,128,1,4' if M <= 32 else '128,32,4,1' if N <= 32 else '128,128,4,2'},true,{xf}>"


def launched(ops, monkeypatch, fn):
    """fn() with the launch profiler installed -> (result, names of the flat-kernel launches)"""
    prof = ops.LaunchProfiler()
    monkeypatch.setattr(ops, "PROFILER", prof)
    with ops.precision(ops.PREC_F32):
        out = fn()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "PROFILER", None)
    return out, [r[0] for r in prof.records if r[0].startswith(("igemm_rows", "wgrad_"))]


def check(what, got, ref, bar):
    e = cr.rel(got, ref)
    print(f"{what}: {e:.3e} of the reference's max (bar {bar:.0e})")
    assert bool(torch.isfinite(got).all()) and e <= bar, (what, e, bar)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 11)


def _ohwi_dev(w):  # [Co, Ci, kh, kw] -> the same logical tensor over OHWI memory on the device
    return w.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)


def _nchw64(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _conv64(x, w, kind):
    return cr._conv(x, w, kind)


def _affine(ops, B, Ci, g, x):
    """a GroupNorm's per-image scale and shift rows as the kernels take them (the statistics pass itself needs 4 channels per
    group and is not under test) -> (Stats, float64 silu(x scale + shift))"""
    scale, shift = torch.rand(B, Ci, generator=g) + 0.5, torch.randn(B, Ci, generator=g) * 0.5
    u = x.double() * scale.double()[:, None, None, :] + shift.double()[:, None, None, :]
    return ops.Stats(None, None, scale.cuda(), shift.cuda()), u * torch.sigmoid(u)


SHAPE = {"c3s2": (2, 12, 12), "c1": (1, 12, 12)}  # 72 output rows: one ragged tile; 144: a full tile and a ragged one


# ------------------------------------------------------------------------------------------------ rows, k-contiguous weights
# K in {36, 64}: a tail chunk past the 16- / 32-channel step, whole chunks; N in {32, 40}: the 128 x 32 tile, ragged columns of the 128 x 128
# tile; the epilogue variants at one channel pair per geometry
FWD = ([(kind, Ci, Co, "plain") for kind in SHAPE for Ci in (36, 64) for Co in (32, 40)]
       + [(kind, 64 if epi == "gn_silu" else 36, 40, epi) for kind in SHAPE for epi in ("bias_res", "track", "gn_silu")])


@pytest.mark.parametrize("kind,Ci,Co,epi", FWD)
def test_forward(cuda, monkeypatch, kind, Ci, Co, epi):
    from vaehip import ops
    B, H, W = SHAPE[kind]
    k = 1 if kind == "c1" else 3
    g = _gen(B, H, Ci, Co, k)
    x = torch.randn(B, H, W, Ci, generator=g) * 1.3 + 0.2
    w = torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(k * k * Ci)
    bias = torch.randn(Co, generator=g) if epi in ("bias_res", "gn_silu") else None
    Ho, Wo = ops.out_hw(kind, H, W)
    res = torch.randn(B, Ho, Wo, Co, generator=g) if epi == "bias_res" else None
    xd, kw = x.cuda(), {}
    act = x.double()
    xf = 0
    if epi == "gn_silu":
        xf = ops.XF_AFFINE_SILU
        st, act = _affine(ops, B, Ci, g, x)
        kw = {"xf": xf, "stats": st}
    M = B * Ho * Wo
    track = ops.conv_track_buffer(M, Co, cuda) if epi == "track" else None
    if track is not None:
        track.fill_(float("nan"))
    y, names = launched(ops, monkeypatch, lambda: ops.conv_fwd(xd, _ohwi_dev(w), None if bias is None else bias.cuda(), kind,
                                                               res=None if res is None else res.cuda(), track=track, **kw))
    assert names == [rows_name(Co, False, xf)], names
    ref = _conv64(_nchw64(act), w.double(), kind)
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
    ref = ref.permute(0, 2, 3, 1)
    if res is not None:
        ref = ref + res.double()
    check(f"fwd {kind} {Ci}->{Co} {epi}", y, ref, cr.BAR_DIRECT)
    if track is not None:  # per 128-row tile and column: the sum of |result|
        r2 = ref.reshape(M, Co).abs()
        tref = torch.stack([r2[t * 128:(t + 1) * 128].sum(0) for t in range((M + 127) // 128)])
        check(f"fwd {kind} track", track, tref, cr.BAR_DIRECT)


# ------------------------------------------------------------------------------------------------ rows, n-contiguous weights
@pytest.mark.parametrize("kind,B,H,W,Ci,Co,parity", [("c3s2", 2, 12, 12, 64, 36, False), ("c3s2", 2, 16, 16, 40, 36, True),
                                                     ("c1", 1, 12, 12, 40, 36, False), ("c1", 1, 12, 12, 32, 64, False)])
def test_dgrad(cuda, monkeypatch, kind, B, H, W, Ci, Co, parity):
    """contraction over Co (K = 36: a tail chunk; 64: two chunks); parity: the class-major stride-2 form, whose four classes meet
    4 / 2 / 2 / 1 taps"""
    from vaehip import ops
    assert (ops.dgrad_args(kind, B, H, W, Co, Ci).g.mode == ops.MODE_DGRAD_S2) == parity
    k = 1 if kind == "c1" else 3
    g = _gen(B, H, Ci, Co, k, 1)
    w = torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(k * k * Co)
    dy = torch.randn(B, *ops.out_hw(kind, H, W), Co, generator=g)
    dx, names = launched(ops, monkeypatch, lambda: ops.conv_dgrad(dy.cuda(), _ohwi_dev(w), kind, (H, W)))
    assert names == [rows_name(Ci, True)], names
    a0 = torch.zeros(B, Ci, H, W, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(_conv64(a0, w.double(), kind), a0, _nchw64(dy))
    check(f"dgrad {kind} {Co}->{Ci} parity={parity}", dx, gx.permute(0, 2, 3, 1), cr.BAR_DIRECT)


# ------------------------------------------------------------------------------------------------ batched GEMMs
def _gemm_forms(ops, A, Bt, Pm, alpha):
    """(form, launch, float64 reference, expected name) of the three GEMMs of the attention position"""
    d = torch.float64
    T, Cc = A.shape[1], A.shape[2]
    return (("nt", lambda: ops.gemm_nt(A.cuda(), Bt.cuda(), alpha), alpha * A.to(d) @ Bt.to(d).transpose(1, 2), rows_name(T, False)),
            ("nn", lambda: ops.gemm_nn(Pm.cuda(), Bt.cuda()), Pm.to(d) @ Bt.to(d), rows_name(Cc, True)),
            ("tn", lambda: ops.gemm_tn(Pm.cuda(), Bt.cuda()), Pm.to(d).transpose(1, 2) @ Bt.to(d), wgrad_name(T, Cc)))


def test_gemms_in_the_attention_position(cuda, monkeypatch):
    from vaehip import ops
    T, Cc, g = 36, 64, _gen(36, 64)
    A, Bt, Pm = torch.randn(2, T, Cc, generator=g), torch.randn(2, T, Cc, generator=g), torch.randn(2, T, T, generator=g)
    for form, run, ref, name in _gemm_forms(ops, A, Bt, Pm, Cc ** -0.5):
        got, names = launched(ops, monkeypatch, run)
        assert names == [name], (form, names)
        check(f"gemm_{form} T={T} C={Cc}", got, ref, cr.BAR_WGRAD if form == "tn" else cr.BAR_DIRECT)


# ------------------------------------------------------------------------------------------------ wgrad
@pytest.mark.parametrize("kind,B,H,W,Ci,Co,gn,nsplit", [("c3s2", 1, 20, 12, 36, 40, False, 1), ("c1", 1, 10, 6, 36, 40, False, 1),
                                                        ("c3s2", 1, 20, 12, 64, 32, False, 1), ("c1", 1, 10, 6, 32, 64, False, 1),
                                                        ("c1", 1, 10, 6, 64, 40, True, 1), ("c1", 2, 16, 16, 36, 40, False, 2)])
def test_wgrad_and_bias_gradient(cuda, monkeypatch, kind, B, H, W, Ci, Co, gn, nsplit):
    """60 pixels (10 x 6; the stride-2 layer reads a 20 x 12 map): no multiple of the 16- or 32-pixel step; Cout = 32: the 32 x 128 tile;
    Cin = 32: the 128 x 32 tile; 512 pixels: two splits"""
    from vaehip import ops
    k = 1 if kind == "c1" else 3
    g = _gen(B, H, Ci, Co, k, 2)
    x = torch.randn(B, H, W, Ci, generator=g) * 1.3 + 0.2
    Ho, Wo = ops.out_hw(kind, H, W)
    dy = torch.randn(B, Ho, Wo, Co, generator=g)
    xd, kw, act, xf = x.cuda(), {}, x.double(), 0
    if gn:
        xf = ops.XF_AFFINE_SILU
        st, act = _affine(ops, B, Ci, g, x)
        kw = {"xf": xf, "stats": st}
    a = ops.wgrad_args(kind, B, H, W, Ci, Co, Ci)
    assert (B * Ho * Wo) % 32 != 0 or nsplit > 1
    gw = torch.full((Co, k, k, Ci), float("nan"), device=cuda).permute(0, 3, 1, 2)
    gb = torch.full((Co,), float("nan"), device=cuda)
    _, names = launched(ops, monkeypatch, lambda: ops.conv_wgrad(dy.cuda(), xd, kind, gw, gb, **kw))
    assert names == [wgrad_name(Co, Ci, xf)], names
    assert max(1, min(512 // (a.g.taps * ((Co + 127) // 128) * ((Ci + 127) // 128)), (B * Ho * Wo) // 256)) == nsplit
    w0 = torch.zeros(Co, Ci, k, k, dtype=torch.float64, requires_grad=True)
    (rw,) = torch.autograd.grad(_conv64(_nchw64(act), w0, kind), w0, _nchw64(dy))
    check(f"wgrad {kind} {Ci}->{Co} gn={gn} splits={nsplit}", gw, rw, cr.BAR_WGRAD_GN if gn else cr.BAR_WGRAD)
    check(f"bias gradient {kind} {Co}", gb, dy.double().sum(dim=(0, 1, 2)), cr.BAR_WGRAD)


# ------------------------------------------------------------------------------------------------ the term check
def test_every_plane_product_is_there_once(cuda, monkeypatch):
    """crafted operands (test_flat_x3_host.py): all positive, every element c 2^e, K = 16, in the three operand forms.  A missing,
    doubled or swapped plane moves a result by at least 5.69e-6 of sum |a b|; the bar is a third of that, above the split's
    truncation (3.3e-8) and the accumulation in fp32 (<= 1.5e-7 at K <= 1024)."""
    from vaehip import ops
    K, M, N = 16, 36, 40
    A, Bt = crafted(2 * M, K, 1).view(2, M, K), crafted(2 * N, K, 2).view(2, N, K)     # nt: A [z,M,K] . Bt [z,N,K]^T
    Bn = Bt.transpose(1, 2).contiguous()                                              # nn: A . Bn [z,K,N]
    At = A.transpose(1, 2).contiguous()                                               # tn: At [z,K,M]^T . Bn
    ref = A.double() @ Bt.double().transpose(1, 2)
    sab = A.double().abs() @ Bt.double().abs().transpose(1, 2)
    assert float(A.min()) > 0 and float(A.max()) <= 4 * C_CRAFTED
    for form, run, name in (("nt", lambda: ops.gemm_nt(A.cuda(), Bt.cuda()), rows_name(N, False)),
                            ("nn", lambda: ops.gemm_nn(A.cuda(), Bn.cuda()), rows_name(N, True)),
                            ("tn", lambda: ops.gemm_tn(At.cuda(), Bn.cuda()), wgrad_name(M, N))):
        got, names = launched(ops, monkeypatch, run)
        assert names == [name], (form, names)
        e = float(((got.double().cpu() - ref).abs() / sab).max())
        print(f"term check {form}: {e:.3e} of sum|ab| (bar 1.9e-6; a dropped term: >= 5.69e-6)")
        assert e <= 1.9e-6, (form, e)


# ------------------------------------------------------------------------------------------------ non-finite, tiny, repeatable
def test_infinity_stays_in_its_rows_and_tiny_operands_keep_their_digits(cuda, monkeypatch):
    from vaehip import ops
    g = _gen(5)
    A, Bt = torch.randn(1, 144, 64, generator=g), torch.randn(1, 40, 64, generator=g)
    Ai = A.clone()
    Ai[0, 5, 7] = float("inf")
    Ai[0, 133, 63] = float("inf")
    got, names = launched(ops, monkeypatch, lambda: ops.gemm_nt(Ai.cuda(), Bt.cuda()))
    assert names == [rows_name(40, False)], names
    fin = torch.isfinite(got.cpu())[0]
    hit = torch.zeros(144, dtype=torch.bool)
    hit[[5, 133]] = True
    assert bool((~fin[hit]).all()), "a row that read +Inf has finite results"
    assert bool(fin[~hit].all()), "a row that read no Inf has non-finite results"
    tiny, names = launched(ops, monkeypatch, lambda: ops.gemm_nt((A * 1e-30).cuda(), Bt.cuda()))
    assert names == [rows_name(40, False)], names
    check("operand of 1e-30-scale values", tiny, (A * 1e-30).double() @ Bt.double().transpose(1, 2), cr.BAR_DIRECT)


def test_twenty_launches_are_bitwise_identical(cuda, monkeypatch):
    from vaehip import ops
    g = _gen(7)
    x = (torch.randn(2, 12, 12, 36, generator=g) * 1.3 + 0.2).cuda()
    w = _ohwi_dev(torch.randn(40, 36, 3, 3, generator=g) / 18)
    dy = torch.randn(2, 6, 6, 40, generator=g).cuda()

    def run():
        gw, gb = torch.empty((40, 3, 3, 36), device=cuda).permute(0, 3, 1, 2), torch.empty(40, device=cuda)
        ops.conv_wgrad(dy, x, "c3s2", gw, gb)
        return ops.conv_fwd(x, w, None, "c3s2"), ops.conv_dgrad(dy, w, "c3s2", (12, 12)), gw, gb

    first, names = launched(ops, monkeypatch, run)
    assert names == [wgrad_name(40, 36), rows_name(40, False), rows_name(36, True)], names
    with ops.precision(ops.PREC_F32):
        for it in range(20):
            for a, b in zip(run(), first):
                assert torch.equal(a, b), f"launch {it} differs"
