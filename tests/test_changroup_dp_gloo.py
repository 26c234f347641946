"""ActivityMonitor.step() on the group dynamics and per-sample activity metrics under data parallelism, on CPU: world_size 2,
gloo, in the style of tests/test_chanhist_dp_gloo.py.  The ranks hold DIFFERENT batch sizes (3 and 5 samples of one batch of 8,
in two forwards each): what a layer keeps are sums over its samples and the sample count, so adding them across the ranks gives
exactly the values a single process computes on the concatenated batch -- which an average of per-rank means would not.  Both
the hook path (a plain module) and buffered ops.changroup results as a device-served layer's sink receives them (CPU tensors
stand in) are run; ranks that buffered different numbers of forwards are refused."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import changroup_refs as R
from changroup_refs import FIVE

G_, EPS_, TAU_ = 2, 1e-5, 0.6
SPLIT = (3, 5)  # samples of each forward's batch of 8 on rank 0 and rank 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _batch(fwd):
    """forward `fwd`'s whole batch [8, 8, 5, 6] (NCHW); channel 3 is strongly active in sample 6 only, channel 5 an outlier"""
    x = R.draw((8, 8, 5, 6), 40 + fwd)
    x[:, 3] *= 0.01
    x[6, 3] *= 500.0
    x[:, 5] *= 20.0
    return x


def _mine(rank, fwd):
    x = _batch(fwd)
    return x[:SPLIT[0]] if rank == 0 else x[SPLIT[0]:]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tracking.monitor import ActivityMonitor, per_sample_sums

        def run(forwards, sync=True, device=False):
            cfg = {"enabled": True, "track_interval": 1, "sync_across_ranks": sync, "near_zero_threshold": TAU_, "group_eps": EPS_,
                   "target_layers": []}
            net = torch.nn.Identity()
            mon = ActivityMonitor(net, cfg)
            if device:  # what Engine._emit hands a device-served layer's sink: changroup = (sums [B, C, 3], HW)
                mon._groups["layer.output"] = (G_, EPS_)
                sink = mon._device_sink("layer.output", FIVE)
                for f in range(forwards):
                    x = _mine(rank, f)
                    sink(None, None, changroup=(per_sample_sums(x), 30))
            else:  # the forward hook _register_hooks() places on a plain module
                mon._groups["layer.output"] = (G_, EPS_)
                mon.hooks.append(net.register_forward_hook(mon._hook("layer.output", FIVE, "output")))
                for f in range(forwards):
                    net(_mine(rank, f))
            mon.step(1)
            return {k: np.asarray(v).tolist() for k, v in mon.get_data_for_step(1)["layer.output"].items()}

        hook, dev, local = run(2), run(2, device=True), run(2, sync=False)
        try:
            run(2 + rank)
            refused = ""
        except RuntimeError as e:
            refused = str(e)
        q.put((rank, hook, dev, local, refused))
    finally:
        dist.destroy_process_group()


def _single(xs):
    """the values a single process gives on the concatenated batch (float64, two-pass)"""
    y = torch.cat(xs).double().numpy()
    y = np.moveaxis(y.reshape(y.shape[0], y.shape[1], -1), 1, 2)
    return R.ref_metrics(y, G_, EPS_, TAU_)


def test_step_adds_the_ranks_sums_world2():
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
    want = _single([_batch(0), _batch(1)])
    # the per-rank means differ, and their plain average is not the batch's value: the sample counts matter
    per_rank = [_single([_mine(r, 0), _mine(r, 1)]) for r in range(2)]
    assert not np.allclose((per_rank[0][R.ACTIVE] + per_rank[1][R.ACTIVE]) / 2, want[R.ACTIVE], rtol=1e-3, atol=0)
    for rank, hook, dev, local, refused in out:
        for got in (hook, dev):
            assert list(got) == FIVE
            for k in FIVE:
                assert np.allclose(got[k], want[k], rtol=1e-6, atol=1e-7), (rank, k)
        assert hook == dev  # both paths buffer the same sums
        # without sync_across_ranks a rank sees its own samples only
        for k in FIVE:
            assert np.allclose(local[k], per_rank[rank][k], rtol=1e-6, atol=1e-7), (rank, k)
        assert "different numbers of forwards" in refused
    assert out[0][1] == out[1][1]  # both ranks hold the same aggregate
    # the selective channel: one sample in 8 activates it
    assert out[0][1][R.ACTIVE][3] == 1.0 / 8 and out[0][1][R.VARIATION][3] > 2.0
