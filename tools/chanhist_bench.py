"""Time of ops.chanhist (per-channel magnitude histogram, near-zero count, max |A|) against ops.moments on the same tensor:
the encoder's first GroupNorm at the benchmark shape, 16 x 256 x 256 x 128 fp32 (537 MB), untransformed and behind a
GroupNorm + SiLU transform.  Both ops read the same bytes once; chanhist adds one LDS atomic per element where moments does
three FMAs.  Device events around each call after a warm-up, the two arms alternated in one process, median per arm; the
results are checked (row sums, near-zero count and max |A| against torch) before anything is timed.
    python tools/chanhist_bench.py [--reps 30] [--out profiles/chanhist_measured.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import torch  # noqa: E402

SHAPE = (16, 256, 256, 128)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "chanhist_measured.json")
TAU = 1e-3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(x, st, xf, reps):
    from vaehip import ops
    from vaehip.lib import lib
    B, H, W, Cc = x.shape
    hist, nz, amax = ops.chanhist(x, st, xf, TAU)
    assert bool((hist.sum(dim=1) == B * H * W).all())
    if st is None:
        assert torch.equal(amax, x.abs().amax(dim=(0, 1, 2))) and torch.equal(nz, (x.abs() < TAU).sum(dim=(0, 1, 2)))
    # the workspace of the launch ops.chanhist makes for this shape: written by the partial pass, read by the final one
    nch = 1024 // B  # ops.chanhist's chunking at this shape (one channel tile, 8 pixel rows)
    n = ctypes.c_int64(0)
    lib.call("vae_chanhist_workspace", B, H * W, Cc, nch, ctypes.byref(n))
    for _ in range(3):
        ops.chanhist(x, st, xf, TAU)
        ops.moments(x, st, xf)
    t_h, t_m = [], []
    for _ in range(reps):  # alternated
        t_h.append(timed(lambda: ops.chanhist(x, st, xf, TAU)))
        t_m.append(timed(lambda: ops.moments(x, st, xf)))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    in_bytes = x.numel() * x.element_size()
    res = {"input_bytes": in_bytes, "chanhist_workspace_bytes": n.value * 4, "workgroups": B * nch,
           "chanhist_median_ms": round(med(t_h), 4), "chanhist_min_ms": round(min(t_h), 4),
           "moments_median_ms": round(med(t_m), 4), "moments_min_ms": round(min(t_m), 4),
           "ratio_chanhist_over_moments": round(med(t_h) / med(t_m), 3),
           # input once; the workspace once out and once back in
           "chanhist_bytes_per_s": round((in_bytes + 2 * n.value * 4) / (med(t_h) * 1e-3), 0),
           "moments_bytes_per_s": round(in_bytes / (med(t_m) * 1e-3), 0),
           "chanhist_ms": [round(v, 4) for v in t_h], "moments_ms": [round(v, 4) for v in t_m]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    from vaehip.ops import XF_AFFINE_SILU, XF_NONE, Stats
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    x = torch.randn(SHAPE, device=dev) * 0.8 + 0.3
    g = torch.Generator(device="cpu").manual_seed(11)
    st = Stats(None, None, (torch.rand((SHAPE[0], SHAPE[3]), generator=g) * 1.5 + 0.25).to(dev),
               (torch.randn((SHAPE[0], SHAPE[3]), generator=g) * 0.5).to(dev))
    res = {"gpu": torch.cuda.get_device_name(0), "shape": list(SHAPE), "dtype": "float32", "reps": a.reps,
           "what": "ops.chanhist against ops.moments on one tensor (each: partial pass + final pass, allocations included); "
                   "device events per call, arms alternated in one process, median"}
    for name, s, xf in (("xf_none", None, XF_NONE), ("xf_affine_silu", st, XF_AFFINE_SILU)):
        res[name] = measure(x, s, xf, a.reps)
        print(name, json.dumps({k: v for k, v in res[name].items() if not k.endswith("_ms") or "median" in k or "min" in k}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
