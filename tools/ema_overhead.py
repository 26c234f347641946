"""What the weight average (training.use_ema) costs, measured two ways on one GPU, one process, arms alternating:

  kernel   at the real arena size (83 653 863 floats): vae_adamw_ema  |  vae_adamw followed by torch.lerp_ on the same tensors
           (what a user had to do from outside)  |  vae_adamw alone.  Device events around windows of --calls calls; per arm the
           median, minimum and maximum window, as time per call and as bytes/s of the array passes the arm needs
           (9, 10 and 7 passes of n floats).
  trainer  HipTrainer at 256x256, batch 16, fp32: two trainers, use_ema on and off, blocks of --steps timed steps after an untimed
           one, alternating; per arm the median step and the spread.

    timeout -k 10 900 python tools/ema_overhead.py [--out profiles/ema_measured.json]

The program ends itself after --limit seconds as well.  No GPU: it fails (there is nothing to measure on a CPU)."""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import torch  # noqa: E402

N_ARENA = 83_653_863
HYPER = (1e-5, 0.9, 0.999, 1e-8, 1e-2)   # lr, betas, eps, weight decay: small steps, the state stays of the size it starts with
PASSES = {"adamw_ema": 9, "adamw+lerp_": 10, "adamw": 7}


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def kernel_arms(n, calls, rounds, dev):
    from vaehip import ops
    gen = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, device=dev, generator=gen) * 0.05
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m = torch.randn(n, device=dev, generator=gen) * 1e-4
    v = torch.rand(n, device=dev, generator=gen) * 1e-6
    e = p.clone()
    sq = ops.sqnorm(g, torch.zeros(1, device=dev))
    d = 0.9999
    omd = 1.0 - d

    def fused():
        ops.adamw_ema(p, g, m, v, e, sq, 1.0, *HYPER, 100, d)

    def two():
        ops.adamw(p, g, m, v, sq, 1.0, *HYPER, 100)
        e.lerp_(p, omd)

    def alone():
        ops.adamw(p, g, m, v, sq, 1.0, *HYPER, 100)

    arms = {"adamw_ema": fused, "adamw+lerp_": two, "adamw": alone}
    us = {k: [] for k in arms}
    for fn in arms.values():   # code objects loaded, torch's lerp_ kernel picked
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in arms.items():
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    out = {}
    for name, xs in us.items():
        s = spread(xs)
        out[name] = {"us_per_call": {k: round(x, 2) if k != "n" else x for k, x in s.items()},
                     "array_passes": PASSES[name],
                     "GB_per_s_at_median": round(PASSES[name] * n * 4 / (s["median"] * 1e-6) / 1e9, 1)}
    med = {k: out[k]["us_per_call"]["median"] for k in out}
    out["fused_over_two_launches"] = round(med["adamw_ema"] / med["adamw+lerp_"], 4)
    out["fused_minus_adamw_us"] = round(med["adamw_ema"] - med["adamw"], 2)
    return out


def trainer_arms(steps, rounds, dev, B=16, R=256):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.trainer import HipTrainer
    gen = torch.Generator(device=dev).manual_seed(42)
    x = torch.rand((B, 3, R, R), device=dev, generator=gen) * 2 - 1
    eps = torch.randn((B, 4, R // 8, R // 8), device=dev, generator=gen)
    trs = {}
    for name, on in (("use_ema_off", False), ("use_ema_on", True)):
        w = SDXLVAEWrapper("synthetic:42", device=dev)
        trs[name] = HipTrainer(w, lr=1e-5, max_grad_norm=1.0, kl_weight=1e-6, lr_warmup_steps=100, max_train_steps=10000, use_ema=on)
        trs[name].train_step(x, eps)   # every shape of the timed window, once
    torch.cuda.synchronize()
    ms = {k: [] for k in trs}
    for _ in range(rounds):
        for name, tr in trs.items():
            tr.train_step(x, eps)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(steps):
                tr.train_step(x, eps)
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms[name] += [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    same = torch.equal(trs["use_ema_on"].vae.arena.flat, trs["use_ema_off"].vae.arena.flat)
    out = {name: {"step_ms": {k: round(x, 3) if k != "n" else x for k, x in spread(xs).items()}} for name, xs in ms.items()}
    on, off = out["use_ema_on"]["step_ms"]["median"], out["use_ema_off"]["step_ms"]["median"]
    out["on_minus_off_ms"] = round(on - off, 3)
    out["on_over_off"] = round(on / off, 5)
    out["images_per_s_off"] = round(B / off * 1e3, 2)
    out["weights_equal_after_the_run"] = bool(same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="optimizer calls per timed window")
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8, help="train steps per timed block")
    ap.add_argument("--trainer-rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=N_ARENA)
    ap.add_argument("--limit", type=int, default=900, help="seconds after which the program ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_measured.json"))
    a = ap.parse_args()
    signal.alarm(a.limit)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    dev = torch.device("cuda:0")
    res = {"gpu": torch.cuda.get_device_name(0), "n": a.n, "calls_per_window": a.calls, "kernel_rounds": a.kernel_rounds,
           "steps_per_block": a.steps, "trainer_rounds": a.trainer_rounds}
    res["kernel"] = kernel_arms(a.n, a.calls, a.kernel_rounds, dev)
    print("kernel", json.dumps(res["kernel"]), flush=True)
    torch.cuda.empty_cache()
    if a.trainer_rounds > 0:
        res["trainer_256_b16_fp32"] = trainer_arms(a.steps, a.trainer_rounds, dev)
        print("trainer", json.dumps(res["trainer_256_b16_fp32"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
