"""Split-K reductions called directly: vae_wgrad_wino_reduce (Winograd slab -> dW / db in one launch, csrc/igemm.hip) and
vae_reduce_splits / vae_reduce_splits2, on seeded random slabs whose magnitudes span six decades (so that splits cancel), against
the same sums and transforms in numpy float64.

Bound, derived per element and not measured: an output is a sum of at most npos * nsplit slab terms with coefficients of
magnitude <= 1 (npos = 1 for the flat sums and the bias gradient); the splits are added one after the other or in a tree
(<= nsplit - 1 roundings on any path), the transform adds <= 2 * npos terms (the factors 0.5 and 0.25 are exact), so
    |out - ref| <= (nsplit + 2 * npos) * 2^-24 * sum |coef * term|,
with the right-hand side computed in float64 from |slab|.  Each call is made twice on the same slab: bit-identical results.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import GuardedPool
from vaehip.lib import lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
AT16 = np.array([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, -1]], dtype=np.float64) * np.array([1, .5, .5, 1])  # A^T diag(c)
AT9 = np.array([[1, 1, 0], [0, 1, 0], [0, 1, -1]], dtype=np.float64)                                        # A''^T


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _slab(dev, shape, seed):
    """standard normal values times 10^u, u uniform in [-3, 3)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(shape, device=dev, generator=g)
    x.mul_(torch.pow(10.0, torch.rand(shape, device=dev, generator=g).mul_(6.0).sub_(3.0)))
    return x


def _sums(x):
    """float64 sum and sum of magnitudes over the splits (axis 0) of a device slab"""
    h = x.cpu().numpy()
    return h.sum(axis=0, dtype=np.float64), np.abs(h).sum(axis=0, dtype=np.float64)


def _close(out, ref, bound, terms, what):
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    tol = terms * U * bound
    bad = ~(err <= tol)  # (a NaN left in the output is beyond the bound too)
    worst = float(np.nanmax(err / np.maximum(tol, 1e-300))) if not np.isnan(err).all() else float("nan")
    print(f"{what}: max err / bound = {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements beyond the bound, worst err / bound = {worst:.3f}"


def _wino_ref(S, Sabs, npos, Cin, Cout):
    r = 4 if npos == 16 else 3
    At = AT16 if npos == 16 else AT9
    ref = np.einsum("ai,bj,ijnm->mabn", At, At, S.reshape(r, r, Cin, Cout))
    bound = np.einsum("ai,bj,ijnm->mabn", np.abs(At), np.abs(At), Sabs.reshape(r, r, Cin, Cout))
    return ref, bound


def _wino_call(slab, ns, npos, Cin, Cout, dW, bpart, db):
    lib.call("vae_wgrad_wino_reduce", _p(slab), ns, npos, Cin, Cout, None, _p(dW), _p(bpart), _p(db), _stream())


def _wino_case(dev, npos, Cin, Cout, ns, seed):
    slab = _slab(dev, (ns, npos, Cin, Cout), seed)
    bpart = _slab(dev, (ns, Cout), seed + 1)
    ref, bound = _wino_ref(*_sums(slab), npos, Cin, Cout)
    bref, bbound = _sums(bpart)
    what = f"npos {npos} Cin {Cin} Cout {Cout} nsplit {ns}"
    for bias in (False, True):
        res = []
        for _ in range(2):
            dW = torch.full((Cout, 3, 3, Cin), float("nan"), device=dev)
            db = torch.full((Cout,), float("nan"), device=dev) if bias else None
            _wino_call(slab, ns, npos, Cin, Cout, dW, bpart if bias else None, db)
            res.append((dW, db))
        _close(res[0][0], ref, bound, ns + 2 * npos, f"dW {what} bias {bias}")
        assert torch.equal(res[0][0], res[1][0]), f"dW {what}: two calls differ"
        if bias:
            _close(res[0][1], bref, bbound, ns + 2, f"db {what}")
            assert torch.equal(res[0][1], res[1][1]), f"db {what}: two calls differ"


@pytest.mark.parametrize("ns", [1, 2, 5, 8, 31, 32, 33, 64])
@pytest.mark.parametrize("Cin,Cout", [(32, 32), (32, 128), (96, 160), (128, 128)])
@pytest.mark.parametrize("npos", [16, 9])
def test_wino_reduce(cuda, npos, Cin, Cout, ns):
    _wino_case(cuda, npos, Cin, Cout, ns, 1000 * npos + Cin + Cout + ns)


@pytest.mark.parametrize("npos,Cin,Cout,ns", [(16, 512, 512, 4), (9, 256, 256, 16)])
def test_wino_reduce_wide_layers(cuda, npos, Cin, Cout, ns):
    """the tile choices only layers with >= 256 x 256 channel pairs reach: 32 x 32 tiles with several splits, 8 x 32 tiles on a
    256-workgroup grid"""
    _wino_case(cuda, npos, Cin, Cout, ns, 7)


def _flat_case(dev, n, ns):
    n2 = 3 if n <= 4608 else 128
    part, part2 = _slab(dev, (ns, n), 31 * n + ns), _slab(dev, (ns, n2), 31 * n + ns + 1)
    (ref, bound), (ref2, bound2) = _sums(part), _sums(part2)
    what = f"n {n} nsplit {ns}"
    for second in (False, True):
        res = []
        for _ in range(2):
            out = torch.full((n,), float("nan"), device=dev)
            out2 = torch.full((n2,), float("nan"), device=dev) if second else None
            if second:
                lib.call("vae_reduce_splits2", _p(part), ns, n, _p(out), _p(part2), n2, _p(out2), _stream())
            else:
                lib.call("vae_reduce_splits", _p(part), ns, n, _p(out), _stream())
            res.append((out, out2))
        _close(res[0][0], ref, bound, ns + 2, f"flat {what} second {second}")
        assert torch.equal(res[0][0], res[1][0]), f"flat {what}: two calls differ"
        if second:
            _close(res[0][1], ref2, bound2, ns + 2, f"flat second {what}")
            assert torch.equal(res[0][1], res[1][1]), f"flat second {what}: two calls differ"


@pytest.mark.parametrize("ns", [1, 7, 32, 257, 1024])
@pytest.mark.parametrize("n", [4, 36, 4608, 147456])
def test_flat_reduce(cuda, n, ns):
    _flat_case(cuda, n, ns)


def test_reductions_in_guarded_memory(cuda):
    """slabs and outputs between poisoned guards: every element of dW / db / out is written, nothing else changes"""
    for npos, Cin, Cout, ns in [(16, 96, 160, 33), (9, 32, 128, 5), (16, 32, 32, 1)]:
        pool = GuardedPool(cuda)
        slab = pool.put(_slab(cuda, (ns, npos, Cin, Cout), 11), "slab")
        bpart = pool.put(_slab(cuda, (ns, Cout), 12), "bias slab")
        pool.snapshot()
        dW, db = pool.alloc((Cout, 3, 3, Cin), label="dW"), pool.alloc((Cout,), label="db")
        _wino_call(slab, ns, npos, Cin, Cout, dW, bpart, db)
        torch.cuda.synchronize()
        assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
        ref, bound = _wino_ref(*_sums(slab), npos, Cin, Cout)
        _close(dW, ref, bound, ns + 2 * npos, f"guarded dW npos {npos}")
        _close(db, *_sums(bpart), ns + 2, f"guarded db npos {npos}")
    for n, ns in [(4608, 1024), (36, 257), (4608, 7)]:
        pool = GuardedPool(cuda)
        part, part2 = pool.put(_slab(cuda, (ns, n), 13), "partial"), pool.put(_slab(cuda, (ns, 3), 14), "partial2")
        pool.snapshot()
        out, out2 = pool.alloc((n,), label="out"), pool.alloc((3,), label="out2")
        lib.call("vae_reduce_splits2", _p(part), ns, n, _p(out), _p(part2), 3, _p(out2), _stream())
        torch.cuda.synchronize()
        assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
        _close(out, *_sums(part), ns + 2, f"guarded flat n {n} nsplit {ns}")
        _close(out2, *_sums(part2), ns + 2, f"guarded flat second n {n} nsplit {ns}")
