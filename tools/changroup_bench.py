"""Time of ops.changroup (float64 sums of y, y^2 and |y| per (sample, channel): the GroupNorm group dynamics and per-sample
activity metrics) against ops.moments and ops.chanhist on the same tensor: the encoder's first GroupNorm at the benchmark shape,
16 x 256 x 256 x 128, in fp32 (537 MB) and bf16 (268 MB) storage, untransformed and behind a GroupNorm + SiLU transform.  All
three read the tensor once; changroup adds five float64 instructions per element where moments does three fp32 FMAs and chanhist
one LDS atomic.  Device events around each call after a warm-up, the three arms alternated in one process, median per arm; the
sums are checked against torch (float64) before anything is timed.
    python tools/changroup_bench.py [--reps 30] [--out profiles/changroup_measured.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import torch  # noqa: E402

SHAPE = (16, 256, 256, 128)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "changroup_measured.json")
TAU = 1e-3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def check(x, sums):
    """float64 torch sums of the untransformed tensor, an image at a time (a float64 copy of 537 MB would not fit beside it)"""
    for b in range(x.shape[0]):
        y = x[b].double().reshape(-1, x.shape[-1])
        ref = torch.stack([y.sum(dim=0), (y * y).sum(dim=0), y.abs().sum(dim=0)], dim=1)
        err = ((sums[b] - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
        assert err < 1e-12, (b, err)  # two float64 summation orders of 65536 terms


def measure(x, st, xf, reps):
    from vaehip import ops
    from vaehip.lib import lib
    B, H, W, Cc = x.shape
    sums = ops.changroup(x, st, xf)
    assert sums.shape == (B, Cc, 3) and bool(torch.isfinite(sums).all())
    if st is None:
        check(x, sums)
    nch = ops.changroup_chunks(B, H * W, Cc)
    n = ctypes.c_int64(0)
    lib.call("vae_changroup_workspace", B, H * W, Cc, nch, ctypes.byref(n))
    arms = {"changroup": lambda: ops.changroup(x, st, xf), "moments": lambda: ops.moments(x, st, xf),
            "chanhist": lambda: ops.chanhist(x, st, xf, TAU)}
    for _ in range(3):
        for fn in arms.values():
            fn()
    t = {k: [] for k in arms}
    for _ in range(reps):  # alternated
        for k, fn in arms.items():
            t[k].append(timed(fn))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    in_bytes = x.numel() * x.element_size()
    res = {"input_bytes": in_bytes, "changroup_workspace_bytes": n.value * 8, "workgroups": B * nch}
    for k in arms:
        res[k + "_median_ms"], res[k + "_min_ms"] = round(med(t[k]), 4), round(min(t[k]), 4)
    res["ratio_changroup_over_moments"] = round(med(t["changroup"]) / med(t["moments"]), 3)
    res["ratio_chanhist_over_moments"] = round(med(t["chanhist"]) / med(t["moments"]), 3)
    # input once; the workspace once out and once back in
    res["changroup_bytes_per_s"] = round((in_bytes + 2 * n.value * 8) / (med(t["changroup"]) * 1e-3), 0)
    res["moments_bytes_per_s"] = round(in_bytes / (med(t["moments"]) * 1e-3), 0)
    for k in arms:
        res[k + "_ms"] = [round(v, 4) for v in t[k]]
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
    x32 = torch.randn(SHAPE, device=dev) * 0.8 + 0.3
    g = torch.Generator(device="cpu").manual_seed(11)
    st = Stats(None, None, (torch.rand((SHAPE[0], SHAPE[3]), generator=g) * 1.5 + 0.25).to(dev),
               (torch.randn((SHAPE[0], SHAPE[3]), generator=g) * 0.5).to(dev))
    res = {"gpu": torch.cuda.get_device_name(0), "shape": list(SHAPE), "reps": a.reps,
           "what": "ops.changroup against ops.moments and ops.chanhist on one tensor (each: partial pass + final pass, allocations "
                   "included); device events per call, arms alternated in one process, median"}
    for dname, x in (("float32", x32), ("bfloat16", x32.to(torch.bfloat16))):
        for name, s, xf in (("xf_none", None, XF_NONE), ("xf_affine_silu", st, XF_AFFINE_SILU)):
            key = f"{dname}_{name}"
            res[key] = measure(x, s, xf, a.reps)
            print(key, json.dumps({k: v for k, v in res[key].items() if not k.endswith("_ms") or "median" in k or "min" in k}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
