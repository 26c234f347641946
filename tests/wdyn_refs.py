"""Float64 references and error bounds for ops.weight_dynamics / tracking.weightdynamics (a helper module, not a test).

Operands are [O][K][I] fp32 arrays w, g, m, v (the arena's memory order of a parameter); they widen exactly to float64, so every
reference product of two operands is exact and every reference sum carries float64 rounding only.  u is formed in float64 from
the float-rounded constants bc1, bc2_sqrt, eps (tracking.weightdynamics.adam_constants), as the issue of the kernel states it.

Bounds (nothing here is measured; they follow from the arithmetic stated at the head of csrc/wdyn.hip).  With U = 2^-24 and S
the sum of the absolute terms of a slice, a sum is within (n_fp32 + c) U S:
  n_fp32: the most fp32 additions any term passes through (chains()).
    out slice, I == 1: one thread adds the K elements in order: K.
    out slice, I > 1: units of W = 4 (I % 4 == 0) or 1 columns, tiles of 256 units, PR = 256 // min(256, I / W) thread rows.
      A thread adds ceil(K / PR) * W elements of a tile in order; wave_reduce adds 6 levels; the wave's value is added to its
      LDS slot once per tile (ntile); combine4 adds 2 levels: ceil(K / PR) * W + 6 + ntile + 2.
    in slice: a thread adds its ceil(K / PR) elements of each of the chunk's min(rpc, O) rows in order (rpc = the rows that fit
      the chunk, at most 8), the PR thread rows are added in order from zero, everything after is float64:
      min(rpc, O) * ceil(K / PR) + PR.
  c: 1 for the product's rounding (the library is built without contraction) + 2 for the higher orders and the float64 tail = 3.
    S_uu also carries the rounding of u: fl(m / bc1), fl(sqrtf(v)), fl(. / bc2_sqrt), fl(. + eps), fl(. / .) are five correctly
    rounded operations (hipcc's default for fp32 division and square root), the three of the positive denominator and the one
    of the numerator each move u by at most U relative, the last by U: 5 U on u, 10 U on u^2: c = 13.  S_gm = sum g m holds no
    u (the issue's definition): its terms are products of two stored operands, c = 3 like the others.
max |w| is bit-exact, NaN if the slice holds one.

update_identity_bound: after a step, w' = fl(fl(w d) - fl(step_size fl(m' / denom))) with d = (float)(1 - lr wd) (adam_elem of
elementwise.hip).  Against the exact w (1 - lr wd): the rounding of d moves w d by |w| 2^-25 <= ulp(w) / 2, the product rounds
by ulp / 2, the subtraction by ulp / 2: within 2 ulp of the larger of |w|, |w'| per element.  The update itself,
fl(step_size fl(m' / denom)) with step_size = (float)(lr / bc1), and lr u with u = fl(fl(m' / bc1) / denom), bc1 rounded to
float, are each three roundings from lr m' / (bc1 denom): 6 U relative per element.  By the triangle inequality the row norms
differ by at most the 2-norm of the per-element 2 ulp, plus 6 U lr sqrt(S_uu), plus lr times the error of sqrt(S_uu) itself
(half the relative bound of S_uu)."""
import numpy as np

U = 2.0 ** -24
SUMS = ("S_ww", "S_gg", "S_wg", "S_mm", "S_gm", "S_uu")
C_PLAIN, C_UU = 3, 13
MODES = ("w", "w+g", "w+g+m+v")
NEEDS = (0, 1, 1, 2, 2, 2)  # the mode (index into MODES) from which each sum exists


def chains(O: int, K: int, I: int, chunk: int):
    """(n_fp32 of an out slice, n_fp32 of an in slice or None) for a tensor [O][K][I]"""
    if I == 1:
        return K, None
    W = 4 if I % 4 == 0 else 1
    nu = I // W
    ntile = (nu + 255) // 256
    PR = 256 // min(256, nu)
    per_thread = -(-K // PR)
    rpc = min(8, max(1, chunk // (K * I)))
    return per_thread * W + 6 + ntile + 2, min(rpc, O) * per_thread + PR


def adam_u(m64, v64, consts):
    bc1, bc2_sqrt, eps = consts
    return (m64 / bc1) / (np.sqrt(v64) / bc2_sqrt + eps)


def ref(w, g=None, m=None, v=None, consts=None):
    """{view: dict(sums float64 [n, 6], scale float64 [n, 6] (the sums of the absolute terms), absmax fp32 [n])}; a sum whose
    operands are missing is NaN.  No `in` view when I == 1."""
    w = np.asarray(w, dtype=np.float32)
    d = lambda a: None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731
    w64, g64, m64, v64 = d(w), d(g), d(m), d(v)
    terms = [w64 * w64, None, None, None, None, None]
    if g64 is not None:
        terms[1], terms[2] = g64 * g64, w64 * g64
    if m64 is not None:
        u = adam_u(m64, v64, consts)
        terms[3], terms[4], terms[5] = m64 * m64, g64 * m64, u * u
    out = {}
    for view, ax in (("out", (1, 2)), ("in", (0, 1))):
        if view == "in" and w.shape[2] == 1:
            continue
        n = w.shape[0] if view == "out" else w.shape[2]
        nan = np.full(n, np.nan)
        with np.errstate(invalid="ignore", over="ignore"):
            sums = np.stack([t.sum(axis=ax) if t is not None else nan for t in terms], axis=1)
            scale = np.stack([np.abs(t).sum(axis=ax) if t is not None else nan for t in terms], axis=1)
            absmax = np.abs(w).max(axis=ax).astype(np.float32)  # np.max hands a NaN on
        out[view] = {"sums": sums, "scale": scale, "absmax": absmax}
    return out


def bounds(r, O, K, I, chunk):
    """{view: float64 [n, 6]} absolute bounds for ref()'s result r"""
    n_out, n_in = chains(O, K, I, chunk)
    c = np.array([C_PLAIN] * 5 + [C_UU], dtype=np.float64)
    return {view: (n + c)[None, :] * U * r[view]["scale"] for view, n in (("out", n_out), ("in", n_in)) if view in r}


def same_bits(got, want) -> bool:
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return bool(got.shape == want.shape and np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def check(got_sums, got_absmax, r_view, bound, mode: int, skip=()):
    """one view's device results against its reference within `bound`; the sums a mode cannot form must be NaN; `skip`: slices
    that hold an inf or a NaN (only their max |w| is held).  -> the worst error / bound"""
    got = np.asarray(got_sums, dtype=np.float64)
    assert got.shape == r_view["sums"].shape, (got.shape, r_view["sums"].shape)
    assert same_bits(got_absmax, r_view["absmax"]), (got_absmax, r_view["absmax"])
    keep = np.ones(got.shape[0], dtype=bool)
    keep[list(skip)] = False
    worst = 0.0
    for j in range(6):
        if NEEDS[j] > mode:
            assert np.isnan(got[:, j]).all(), (SUMS[j], MODES[mode])
            continue
        err = np.abs(got[keep, j] - r_view["sums"][keep, j])
        assert np.isfinite(got[keep, j]).all(), SUMS[j]
        assert (err <= bound[keep, j]).all(), (SUMS[j], np.argwhere(err > bound[keep, j])[:8], err.max(), bound[keep, j].max())
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.nan_to_num(err / bound[keep, j], nan=0.0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    return worst


def draw(shape, seed: int):
    """(w, g, m, v) fp32 [O][K][I]: w, g, m with both signs, each scaled by 2^k with k in -3..3 per element (several binades),
    v > 0 over the binades of g^2; w g and g m cancel to about sqrt(n) of their absolute terms"""
    rng = np.random.default_rng(seed)
    sc = lambda: np.exp2(rng.integers(-3, 4, size=shape)).astype(np.float32)  # noqa: E731
    w = (rng.standard_normal(shape) * 0.05).astype(np.float32) * sc()
    g = (rng.standard_normal(shape) * 1e-3).astype(np.float32) * sc()
    m = (rng.standard_normal(shape) * 1e-3).astype(np.float32) * sc()
    v = (((np.abs(rng.standard_normal(shape)) + 0.25) * 1e-3) ** 2).astype(np.float32) * sc()  # no v near 0: u stays O(1)
    return w, g, m, v


def ulp(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def update_identity_bound(w_before, w_after, lr, suu_ref, suu_scale, n_out):
    """[O] bound on | ||w' - w (1 - lr wd)||_row - lr sqrt(S_uu) | for [O][K][I] weights and the out view's S_uu (docstring)"""
    e = 2.0 * np.maximum(ulp(w_before), ulp(w_after))
    rounding = np.sqrt((e * e).sum(axis=(1, 2)))
    root = np.sqrt(suu_ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        root_err = np.where(root > 0, 0.5 * (n_out + C_UU) * U * suu_scale / np.where(root > 0, root, 1.0), 0.0)
    return rounding + 6.0 * U * lr * root + lr * root_err
