"""Times the split-K reductions alone, at the shapes the fp32 step ships (256^2, batch 16): vae_wgrad_wino_reduce per (npos, Cin,
Cout, nsplit) and vae_reduce_splits for the <= 4-channel weight gradients.  Device events around `rounds` passes over a ring of
slabs larger than 512 MB in all, so that no pass finds its slab in the 256 MB memory-side cache.  GB/s = (slab + dW bytes) / time.
Run it once per library build (VAEHIP_LIB selects another one) and compare; a `scratch` buffer is always passed, which builds
that read the slab once ignore.

usage: python tools/wgrad_reduce_bench.py [--rounds 20] [--out FILE]   (prints one JSON line)"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vae-channel-dynamics_amd", "src"))
import torch  # noqa: E402

from vaehip.lib import LIB_PATH, lib  # noqa: E402

# (npos, Cin, Cout, nsplit): the seven plain 3x3 shapes of the step; the upsampler convolutions (npos 9) with the split count of
# the plain layer of their width
WINO = [(16, 128, 128, 64), (16, 128, 256, 32), (16, 256, 128, 32), (16, 256, 256, 16), (16, 256, 512, 8), (16, 512, 256, 8),
        (16, 512, 512, 4), (9, 512, 512, 4), (9, 256, 256, 16), (16, 128, 128, 1), (16, 512, 512, 1)]
FLAT = [(4608, 1024), (147456, 128)]  # (n, nsplit): conv_in / conv_out weight gradients; a 128-channel layer of the bf16 step
RING_BYTES = 512 << 20


def _p(t):
    return C.c_void_p(t.data_ptr())


def _time(fn, ring, rounds):
    for i in range(ring):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        for i in range(ring):
            fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (rounds * ring)  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for npos, Ci, Co, ns in WINO:
        n = npos * Ci * Co
        ring = max(2, -(-RING_BYTES // (4 * n * ns)))
        slabs = [torch.randn((ns, n), device=dev) for _ in range(ring)]
        bpart, scratch = torch.randn((ns, Co), device=dev), torch.empty((n,), device=dev)
        dW, db = torch.empty((Co, 3, 3, Ci), device=dev), torch.empty((Co,), device=dev)
        us = _time(lambda i: lib.call("vae_wgrad_wino_reduce", _p(slabs[i]), ns, npos, Ci, Co, _p(scratch), _p(dW), _p(bpart), _p(db), st),
                   ring, a.rounds)
        mb = 4 * (n * ns + 9 * Ci * Co) / 1e6
        rows.append({"call": "vae_wgrad_wino_reduce", "npos": npos, "Cin": Ci, "Cout": Co, "nsplit": ns, "us": round(us, 2), "MB": round(mb, 2),
                     "GBps": round(mb / us * 1e3, 1)})
        del slabs
    for n, ns in FLAT:
        ring = max(2, -(-RING_BYTES // (4 * n * ns)))
        slabs = [torch.randn((ns, n), device=dev) for _ in range(ring)]
        out = torch.empty((n,), device=dev)
        us = _time(lambda i: lib.call("vae_reduce_splits", _p(slabs[i]), ns, n, _p(out), st), ring, a.rounds)
        mb = 4 * (n * ns + n) / 1e6
        rows.append({"call": "vae_reduce_splits", "n": n, "nsplit": ns, "us": round(us, 2), "MB": round(mb, 2), "GBps": round(mb / us * 1e3, 1)})
        del slabs
    res = {"lib": os.path.basename(LIB_PATH), "rounds": a.rounds, "ring_bytes": RING_BYTES, "rows": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
