"""ActivityMonitor.step() on buffered ops.chanhist triples under data parallelism, on CPU: world_size 2, gloo, in the style of
tests/test_dp_gloo.py.  The triples a device-served layer buffers are stood in for by CPU tensors: the histograms are summed
across ranks, the maxima maxed (a NaN survives), the near-zero fractions averaged, and ranks that buffered different numbers
of forwards are refused."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HIST, AMAX, NZ = "log2_histogram_per_channel", "abs_max_activation_per_channel", "near_zero_fraction_per_channel"
C_, N_ = 3, 40  # channels, B * H * W of a forward


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _triple(rank, fwd):
    """(hist [C, 48], nzero [C], absmax [C]) of forward `fwd` on rank `rank`: every row sums to N_"""
    hist = torch.zeros((C_, 48), dtype=torch.int64)
    for c in range(C_):
        hist[c, 10 + rank + c] = N_ - 7 - fwd
        hist[c, 47] = 7 + fwd
    nzero = torch.tensor([rank * 10 + fwd + c for c in range(C_)], dtype=torch.int64)
    absmax = torch.tensor([1.0 + rank + 0.5 * fwd, 100.0 * (1 - rank) + fwd, 3.0])
    if rank == 0 and fwd == 1:
        absmax[2] = float("nan")
    return hist, nzero, absmax


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tracking.monitor import ActivityMonitor, _ChanHist

        def run(forwards, sync=True):
            mon = ActivityMonitor(torch.nn.Identity(), {"enabled": True, "track_interval": 1, "sync_across_ranks": sync})
            for f in range(forwards):
                t = _ChanHist(_triple(rank, f))
                for m in (HIST, AMAX, NZ):
                    mon.hook_collected_buffer["layer.output"][m].append(t)
            mon.step(1)
            return {k: np.asarray(v).tolist() for k, v in mon.get_data_for_step(1)["layer.output"].items()}

        synced, local = run(2), run(2, sync=False)
        try:
            run(2 + rank)
            refused = ""
        except RuntimeError as e:
            refused = str(e)
        q.put((rank, synced, local, refused))
    finally:
        dist.destroy_process_group()


def test_step_combines_the_ranks_world2():
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
    t = {(r, f): _triple(r, f) for r in range(2) for f in range(2)}
    want_hist = sum(t[k][0] for k in t).tolist()
    want_frac = np.mean([np.mean([(t[(r, f)][1].double() / N_).numpy() for r in range(2)], axis=0) for f in range(2)], axis=0)
    for rank, synced, local, refused in out:
        assert synced[HIST] == want_hist and all(sum(row) == 4 * N_ for row in synced[HIST])
        assert synced[AMAX][:2] == [2.5, 101.0] and np.isnan(synced[AMAX][2])  # rank 1's 2.5, rank 0's 101, rank 0's NaN
        assert np.allclose(synced[NZ], want_frac, rtol=1e-6, atol=0)
        # without sync_across_ranks a rank sees its own forwards only
        assert local[HIST] == (t[(rank, 0)][0] + t[(rank, 1)][0]).tolist()
        assert local[AMAX][:2] == [1.5 + rank, 100.0 * (1 - rank) + 1] and np.isnan(local[AMAX][2]) == (rank == 0)
        assert "different numbers of forwards" in refused
    assert out[0][1][HIST] == out[1][1][HIST] and out[0][1][NZ] == out[1][1][NZ]  # both ranks hold the same aggregate
