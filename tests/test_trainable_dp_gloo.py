"""Data parallelism with frozen parameters on CPU: world_size 2, gloo, in the style of tests/test_dp_gloo.py.  With `decoder`
trainable the ranks exchange only the span of the trainable ranges; the device kernels are replaced by host stand-ins."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from models.sdxl_vae_wrapper import SDXLVAEWrapper
        from vaehip.trainer import HipTrainer
        w = SDXLVAEWrapper("synthetic:%d" % (rank + 1))  # replicas start different: the trainer broadcasts rank 0's, whole arena
        tr = HipTrainer(w, lr=1.0, lr_warmup_steps=0, max_train_steps=10, bucket_mb=16.0, trainable="decoder",
                        gradient_accumulation_steps=2)
        a = w.vae.arena
        (lo, hi), = tr.trainable_ranges
        start = a.flat.clone()
        eng = w.vae.engine
        launched = []

        def fake_fwd_bwd(pv, eps, klw, sample, gen, grad_scale=1.0):
            # what the tape does with the encoder frozen: decoder gradients, watermarks from the top of the arena down to the
            # first trainable offset, then the closing ready(0); the frozen stretch keeps a rank's own stale values
            a.grad[:lo] = 1000.0 + rank
            a.grad[lo:] = float(pv) * grad_scale
            if eng.reducer is not None:
                eng.reducer.ready((lo + hi) // 2)
                eng.reducer.ready(lo)
                eng.reducer.ready(0)
                launched.extend(eng.reducer.launched)
            return {"scalars": torch.zeros(3)}
        eng.forward_backward = fake_fwd_bwd
        tr._add = lambda x, y, out: torch.add(x, y, out=out)

        seen = []

        def fake_step():  # plain SGD on the trainable span, nothing else: what the ranges kernels are held to on the GPU
            seen.append((float(a.grad[lo:hi].min()), float(a.grad[lo:hi].max())))
            a.flat[lo:hi] -= a.grad[lo:hi]
        tr.optimizer.step = fake_step
        vals = [[2.0, 4.0, 8.0], [20.0, 40.0, 80.0]][rank]
        tr.train_step(vals[0])
        tr.train_step(vals[1])      # the window's update: the earlier sum through the second reducer, this one by watermarks
        tr.train_step(vals[2])
        tr.flush()                  # a window of one, exchanged by flush()'s all-reduce over the span
        acc = tr._accum_reducer
        q.put((rank, lo, hi, a.total, launched, list(acc.buckets) if acc is not None else None, list(tr.reducer.buckets),
               float(a.flat[lo:hi].double().sum()), seen,
               bool(torch.equal(a.flat[:lo], start[:lo])), float(a.flat[:lo].double().sum()), float(a.grad[0]), tr.global_step))
    finally:
        dist.destroy_process_group()


def test_decoder_only_exchange_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    sums, frozen_sums = [], []
    for rank, lo, hi, total, launched, acc_buckets, buckets, s, seen, frozen_same, fs, g0, gstep in out:
        assert 0 < lo < hi == total and gstep == 2
        for plan in (buckets, acc_buckets, launched):
            assert plan and all(lo <= b0 < b1 <= hi for b0, b1 in plan), (rank, plan[:3])
        assert buckets[0][1] == hi and buckets[-1][0] == lo and len(buckets) > 2
        assert sorted(set(launched)) == sorted(buckets)      # every bucket of the span went out, none outside it
        # mean over ranks of the 1/2-scaled window sums: ((2 + 4) / 2 + (20 + 40) / 2) / 2 = 16.5, then (8 / 2 + 80 / 2) / 2 = 22
        assert seen == [(16.5, 16.5), (22.0, 22.0)]
        assert frozen_same                                     # frozen weights: what rank 0 broadcast, untouched since
        assert g0 == 1000.0 + rank                             # the frozen stretch of the gradient never travelled
        sums.append(s)
        frozen_sums.append(fs)
    assert sums[0] == sums[1] and frozen_sums[0] == frozen_sums[1]   # both ranks end with identical weights
