"""Time of ops.chancov (channel covariance and mean in one read, split-bf16 products; csrc/chancov.hip) against the torch
formula on the same device tensor (materialise y, centre, Z.T @ Z in fp32) and against ops.moments, at the two ends of the
shipped shapes: 16 x 256 x 256 x 128 fp32 behind GroupNorm + SiLU (memory-bound: 537 MB read once) and 16 x 64 x 64 x 512
(compute-bound: ten tile pairs).  Device events around each call after a warm-up, the three arms alternated in one process,
medians and quartiles; before anything is timed the result is held to a float64 covariance computed on the device (the
criterion of tests/chancov_refs.py), and a sweep of small shapes records the worst error per case group.
    python tools/chancov_bench.py [--reps 30] [--out profiles/chancov_measured.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import torch  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "chancov_measured.json")
BAR, MEAN_TOL = 3e-5, 1e-6  # conv_routes.BAR_WGRAD; the mean's tolerance


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def y_of(x, st, xf, dtype):
    """y = XF(x) as `dtype` [N, C]"""
    B, Cc = x.shape[0], x.shape[-1]
    v = x.to(dtype).reshape(B, -1, Cc)
    if st is not None:
        v = v * st.scale.to(dtype)[:, None, :Cc] + st.shift.to(dtype)[:, None, :Cc]
        if xf == 2:
            v = v * torch.sigmoid(v)
    return v.reshape(-1, Cc)


def torch_formula(x, st, xf):
    """what a user would write: materialise y, centre it, Z.T @ Z in fp32"""
    y = y_of(x, st, xf, torch.float32)
    mean = y.mean(dim=0)
    z = y - mean
    return (z.t() @ z) / (y.shape[0] - 1), mean


def errors(got, x, st, xf):
    """(worst |cov - cov64| (N - 1) / sqrt(S_c S_c'), worst |mean - mean64| / (|mean| + sqrt(S_c / N))), float64 on the device"""
    y = y_of(x, st, xf, torch.float64)
    n = y.shape[0]
    mean = y.mean(dim=0)
    S = ((y - y[0]) ** 2).sum(dim=0)
    z = y - mean
    cov = (z.t() @ z) / (n - 1)
    den = torch.sqrt(S[:, None] * S[None, :])
    e = ((got[0].double() - cov).abs() * (n - 1) / den).max()
    m = ((got[1].double() - mean).abs() / (mean.abs() + torch.sqrt(S / n))).max()
    return float(e), float(m)


def quart(v):
    s = sorted(v)
    return {"median_ms": round(s[len(s) // 2], 4), "q1_ms": round(s[len(s) // 4], 4), "q3_ms": round(s[(3 * len(s)) // 4], 4),
            "min_ms": round(s[0], 4)}


def measure(x, st, xf, reps):
    from vaehip import ops
    from vaehip.lib import lib
    B, H, W, Cc = x.shape
    got = ops.chancov(x, st, xf)
    e_cov, e_mean = errors(got, x, st, xf)
    t_cov, t_mean = errors(torch_formula(x, st, xf), x, st, xf)
    assert e_cov <= BAR and e_mean <= MEAN_TOL, (e_cov, e_mean)
    nch = ops.chancov_chunks(B, H * W, Cc)
    n = ctypes.c_int64(0)
    lib.call("vae_chancov_workspace", B, H * W, Cc, nch, ctypes.byref(n))
    arms = {"chancov": lambda: ops.chancov(x, st, xf), "torch_formula": lambda: torch_formula(x, st, xf),
            "moments": lambda: ops.moments(x, st, xf)}
    for _ in range(3):
        for fn in arms.values():
            fn()
    t = {k: [] for k in arms}
    for _ in range(reps):  # alternated
        for k, fn in arms.items():
            t[k].append(timed(fn))
    res = {k: dict(quart(v), all_ms=[round(u, 4) for u in v]) for k, v in t.items()}
    in_bytes = x.numel() * x.element_size()
    tiles = -(-Cc // 128)
    c, f, m = (res[k]["median_ms"] for k in ("chancov", "torch_formula", "moments"))
    spread = max(res["chancov"]["q3_ms"] - res["chancov"]["q1_ms"], res["torch_formula"]["q3_ms"] - res["torch_formula"]["q1_ms"])
    res.update({"input_bytes": in_bytes, "nchunk": nch, "workgroups": B * nch * tiles * (tiles + 1) // 2,
                "workspace_bytes": n.value * 4, "error_cov": e_cov, "error_mean": e_mean,
                "torch_formula_error_cov": t_cov, "torch_formula_error_mean": t_mean,
                "ratio_torch_formula_over_chancov": round(f / c, 3), "ratio_chancov_over_moments": round(c / m, 3),
                "gain_ms": round(f - c, 4), "larger_quartile_spread_ms": round(spread, 4),
                # the input's bytes over the call's time (the workspace, written and read once more, not counted)
                "chancov_input_bytes_per_s": round(in_bytes / (c * 1e-3), 0),
                "chancov_flop": 2 * B * H * W * Cc * Cc, "chancov_tflops_of_the_gram": round(2 * B * H * W * Cc * Cc / (c * 1e-3) / 1e12, 2)})
    return res


def accuracy_sweep(dev):
    """worst error per case group over small shapes around the tile edges (the GPU suite's sweep, in short)"""
    from vaehip import ops
    from vaehip.ops import Stats
    out = {}
    g = torch.Generator(device="cpu").manual_seed(1)
    for Cc in (1, 3, 8, 127, 128, 129, 257, 512):
        for B, H, W in ((1, 7, 13), (3, 7, 13), (3, 16, 16), (1, 32, 24)):
            for dt in (torch.float32, torch.bfloat16):
                for xf in (0, 1, 2):
                    x = ((torch.randn((B, H, W, Cc), generator=g) * 1.3 + 0.4) * (torch.rand((Cc,), generator=g) + 0.5)
                         + torch.randn((Cc,), generator=g)).to(dev).to(dt)
                    st = Stats(None, None, (torch.rand((B, Cc), generator=g) * 1.5 + 0.25).to(dev),
                               (torch.randn((B, Cc), generator=g) * 0.5).to(dev)) if xf else None
                    e, m = errors(ops.chancov(x, st, xf), x, st, xf)
                    w = out.setdefault(f"{str(dt)[6:]}_xf{xf}", {"worst_error_cov": 0.0, "worst_error_mean": 0.0, "cases": 0})
                    w["worst_error_cov"], w["worst_error_mean"] = max(w["worst_error_cov"], e), max(w["worst_error_mean"], m)
                    w["cases"] += 1
    # every channel's mean 1000 sigma away, exactly representable values
    k = torch.round(torch.randn((3, 16, 16, 129), generator=g) * 1024.0)
    x = (1024.0 + k / 1024.0).to(dev)
    e, m = errors(ops.chancov(x), x, None, 0)
    out["mean_1000_sigma_float32"] = {"worst_error_cov": e, "worst_error_mean": m, "cases": 1}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    from vaehip.ops import XF_AFFINE_SILU, XF_NONE, Stats
    dev = torch.device("cuda:0")
    res = {"gpu": torch.cuda.get_device_name(0), "reps": a.reps, "bar_cov": BAR, "bar_mean": MEAN_TOL,
           "what": "ops.chancov against the torch formula (materialise y, centre, Z.T @ Z in fp32) and ops.moments on one "
                   "tensor (allocations included); device events per call, arms alternated in one process, median and "
                   "quartiles; errors on the scale of tests/chancov_refs.py against float64 on the device"}
    res["accuracy"] = accuracy_sweep(dev)
    print("accuracy", json.dumps(res["accuracy"]), flush=True)
    g = torch.Generator(device="cpu").manual_seed(11)
    for name, shape, xf in (("c128_groupnorm_silu", (16, 256, 256, 128), XF_AFFINE_SILU), ("c512", (16, 64, 64, 512), XF_NONE)):
        torch.manual_seed(3)
        x = torch.randn(shape, device=dev) * 0.8 + 0.3
        st = Stats(None, None, (torch.rand((shape[0], shape[3]), generator=g) * 1.5 + 0.25).to(dev),
                   (torch.randn((shape[0], shape[3]), generator=g) * 0.5).to(dev)) if xf else None
        r = measure(x, st, xf, a.reps)
        r["shape"], r["dtype"], r["xf"] = list(shape), "float32", xf
        res[name] = r
        print(name, json.dumps({k: v for k, v in r.items() if not isinstance(v, dict)}),
              json.dumps({k: {q: u for q, u in v.items() if q != "all_ms"} for k, v in r.items() if isinstance(v, dict)}), flush=True)
        del x, st
    c = res["c128_groupnorm_silu"]
    res["condition_c128_faster_than_formula_by_more_than_the_spreads"] = bool(c["gain_ms"] > c["larger_quartile_spread_ms"])
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)
    assert res["condition_c128_faster_than_formula_by_more_than_the_spreads"], (c["gain_ms"], c["larger_quartile_spread_ms"])


if __name__ == "__main__":
    main()
