"""What a reconstruction loss other than MSE costs in the train step (vaehip/losses.py, csrc/recon_loss.hip), on one GPU:

  step     HipTrainer at 256x256, batch 16, one trainer per leg (mse = the default spec, l1, huber + 0.2 ssim), blocks of --steps
           timed steps after an untimed one, legs alternating, in fp32 and in bf16 mode; per leg the median step and the spread.
  kernels  the loss launches alone on tensors of that shape under ops.LaunchProfiler (device events around every launch):
           time per launch of pixel_loss_kernel, ssim_fwd_kernel, ssim_bwd_kernel, recon_final_kernel, with the bytes each must
           move and the rate that gives.

    timeout -k 10 900 python tools/recon_loss_bench.py [--legs mse,l1,huber_ssim] [--label new] [--out profiles/recon_loss_measured.json]

--src names the `src` directory of ANOTHER checkout (the parent commit) to time its step with this program: use --legs mse there,
the only leg such a checkout has.  Results are merged into --out under runs[label].  The program ends itself after --limit
seconds.  No GPU: it fails (there is nothing to measure on a CPU)."""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

B, R = 16, 256


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3), "n": len(xs)}


def specs(legs):
    out = {}
    for leg in legs:
        if leg == "mse":
            out[leg] = None   # HipTrainer without the argument: also what a checkout from before the feature accepts
        else:
            from vaehip.losses import ReconLoss
            out[leg] = {"l1": ReconLoss("l1"), "huber_ssim": ReconLoss("huber", 0.5, 0.2)}[leg]
    return out


def step_legs(legs, mode, steps, rounds, dev):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.trainer import HipTrainer
    gen = torch.Generator(device=dev).manual_seed(42)
    x = torch.rand((B, 3, R, R), device=dev, generator=gen) * 2 - 1
    eps = torch.randn((B, 4, R // 8, R // 8), device=dev, generator=gen)
    trs = {}
    for leg, spec in specs(legs).items():
        w = SDXLVAEWrapper("synthetic:42", device=dev)
        kw = {} if spec is None else {"recon_loss": spec}
        trs[leg] = HipTrainer(w, lr=1e-5, max_grad_norm=1.0, kl_weight=1e-6, lr_warmup_steps=100, max_train_steps=10000,
                              mixed_precision=mode, **kw)
        trs[leg].train_step(x, eps)   # every shape of the timed window, once
    torch.cuda.synchronize()
    ms = {k: [] for k in trs}
    for _ in range(rounds):
        for leg, tr in trs.items():
            tr.train_step(x, eps)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(steps):
                tr.train_step(x, eps)
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms[leg] += [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    out = {leg: {"step_ms": spread(xs)} for leg, xs in ms.items()}
    for leg in out:
        if leg != "mse" and "mse" in out:
            out[leg]["minus_mse_ms"] = round(out[leg]["step_ms"]["median"] - out["mse"]["step_ms"]["median"], 3)
    return out


def kernel_times(calls, dev):
    from vaehip import ops
    from vaehip.losses import ReconLoss
    gen = torch.Generator(device=dev).manual_seed(7)
    t = torch.rand((B, R, R, 3), device=dev, generator=gen) * 2 - 1
    r = t + 0.2 * torch.randn((B, R, R, 3), device=dev, generator=gen)
    klp = torch.ones((B, 16), device=dev)
    spec = ReconLoss("huber", 0.5, 0.2)
    for _ in range(3):
        ops.recon_loss(r, t, klp, 1e-6, spec)
    prof = ops.LaunchProfiler()
    ops.PROFILER = prof
    try:
        for _ in range(calls):
            ops.recon_loss(r, t, klp, 1e-6, spec)
        summ = prof.summary()
    finally:
        ops.PROFILER = None
    n, pos = r.numel(), B * 3 * (R - 10) * (R - 10)
    # what each launch must move: operands read once, results written once (halo re-reads are served by the caches or not)
    need = {"pixel_loss_kernel": 3 * n * 4, "ssim_fwd_kernel": 2 * n * 4 + 3 * pos * 8, "ssim_bwd_kernel": 3 * pos * 8 + 4 * n * 4,
            "recon_final_kernel": 0}
    out = {}
    for k, v in summ.items():
        us = v["ms"] * 1e3 / v["launches"]
        out[k] = {"us_per_launch": round(us, 2), "launches": v["launches"], "bytes_needed": need.get(k, 0),
                  "GB_per_s": round(need.get(k, 0) / (us * 1e-6) / 1e9, 1) if us > 0 else None}
    out["all_four_us"] = round(sum(v["us_per_launch"] for v in out.values()), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="mse,l1,huber_ssim")
    ap.add_argument("--modes", default="no,bf16")
    ap.add_argument("--steps", type=int, default=8, help="train steps per timed block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50, help="loss calls of the kernel timing (0: skip it)")
    ap.add_argument("--src", default=os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))
    ap.add_argument("--label", default="this_tree")
    ap.add_argument("--limit", type=int, default=900, help="seconds after which the program ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_loss_measured.json"))
    a = ap.parse_args()
    signal.alarm(a.limit)
    sys.path.insert(0, os.path.abspath(a.src))
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    dev = torch.device("cuda:0")
    legs = [s for s in a.legs.split(",") if s]
    res = {"gpu": torch.cuda.get_device_name(0), "src": os.path.relpath(os.path.abspath(a.src), ROOT), "batch": B, "resolution": R,
           "steps_per_block": a.steps, "rounds": a.rounds}
    for mode in [m for m in a.modes.split(",") if m]:
        res["fp32" if mode == "no" else mode] = step_legs(legs, mode, a.steps, a.rounds, dev)
        print(mode, json.dumps(res["fp32" if mode == "no" else mode]), flush=True)
        torch.cuda.empty_cache()
    if a.calls > 0 and "huber_ssim" in legs:
        res["kernels"] = kernel_times(a.calls, dev)
        print("kernels", json.dumps(res["kernels"]), flush=True)
    try:
        doc = json.load(open(a.out))
    except Exception:
        doc = {}
    doc.setdefault("runs", {})[a.label] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
