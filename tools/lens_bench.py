"""Time of the logit lens's work on one captured activation (one GPU), two ways, in one process:
  host   -- the path before the lens kernels existed: the hook's .cpu() of the whole captured tensor, then torch on the CPU:
            min/max normalisation and the fp32 mini-decoder on 1 sample x 4 channels (what the reference's VAELogitLens computes)
  device -- VAELogitLens.channel_maps + project on the device tensor (csrc/lens.hip), including the copy of their results
            (the pictures' pixels) to the host
on tensors with the shapes of evaluate.py's default lens layer encoder.down_blocks.0.resnets.0.norm1 at 256 x 256, batch 16
([16, 256, 256, 128]) and of a 512-channel mid-block layer ([16, 32, 32, 512]), fp32 NHWC as add_device_captures stores
them.  Random values: neither path's time depends on them.  Wall clock around each repetition, ending in a synchronise; arms
alternated after a warm-up; median per arm.  The bytes each path brings to the host are computed from the shapes.  The two
arms' results are compared before anything is timed.
    python tools/lens_bench.py [--reps 10] [--out profiles/logit_lens_measured.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import torch  # noqa: E402

LAYERS = {"encoder.down_blocks.0.resnets.0.norm1@256x256_b16": (16, 256, 256, 128), "mid_block_512ch@256x256_b16": (16, 32, 32, 512)}
DEFAULT_OUT = os.path.join(ROOT, "profiles", "logit_lens_measured.json")
S, K = 1, 4


def host_path(act_dev, decoder):
    full = act_dev.permute(0, 3, 1, 2).detach().cpu()  # the hook's capture: the whole tensor as the (B, C, H, W) view it receives
    maps, imgs = [], []
    with torch.no_grad():
        for s in range(S):
            for c in range(K):
                p = full[s, c]
                d = p.max() - p.min()
                maps.append((p - p.min()) / d if d > 1e-6 else torch.zeros_like(p))
                imgs.append(decoder(p[None, None])[0].permute(1, 2, 0))
    return torch.stack(maps), torch.stack(imgs)


def device_path(act_dev, lens):
    norm = lens.channel_maps(act_dev, S, range(K))[2].cpu()
    imgs = lens.project(act_dev, S, range(K)).cpu()
    return norm.reshape(S * K, *norm.shape[2:]), imgs.reshape(S * K, *imgs.shape[2:])


def wall(fn, reps):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def measure(name, shape, reps, lens):
    dev = torch.device("cuda:0")
    B, H, W, C = shape
    act = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(42)) * 3.0
    decoder = lens.mini_decoder
    (n_h, i_h), (n_d, i_d) = host_path(act, decoder), device_path(act, lens)
    res = {"shape_nhwc": list(shape), "samples": S, "channels": K,
           "host_path_bytes_to_host": B * C * H * W * 4,
           "device_path_bytes_to_host": S * K * H * W * 4 + S * K * 16 * H * W * 3 * 4,
           "normalisation_identical": bool(torch.equal(n_h, n_d)), "projection_max_difference": float((i_h - i_d).abs().max())}
    assert res["normalisation_identical"] and res["projection_max_difference"] < 1e-5, res
    wall(lambda: host_path(act, decoder), 1), wall(lambda: device_path(act, lens), 2)  # warm-up
    t_host, t_dev = [], []
    for _ in range(2):  # two blocks per arm, alternated
        t_dev += wall(lambda: device_path(act, lens), reps // 2)
        t_host += wall(lambda: host_path(act, decoder), reps // 2)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    res.update(device_median_ms=round(med(t_dev), 3), host_median_ms=round(med(t_host), 3),
               device_ms=[round(x, 3) for x in t_dev], host_ms=[round(x, 2) for x in t_host])
    print(name, json.dumps({k: v for k, v in res.items() if not k.endswith("_ms") or "median" in k}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    from analysis.logit_lens import VAELogitLens
    torch.manual_seed(0)
    res = {"gpu": torch.cuda.get_device_name(0), "reps": a.reps,
           "what": "logit lens of 1 sample x 4 channels of one captured activation: host path (.cpu() of the whole tensor + torch on the "
                   "CPU) against the device path (lens kernels + copy of the results); wall clock incl. synchronise, median"}
    with tempfile.TemporaryDirectory() as tmp:
        lens = VAELogitLens(logit_lens_config={"mini_decoder_input_channels": 1}, main_experiment_output_dir=tmp)
        for name, shape in LAYERS.items():
            res[name] = measure(name, shape, a.reps, lens)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
