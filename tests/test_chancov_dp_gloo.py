"""ActivityMonitor.step() on a device-served layer's running covariance sum under data parallelism, on CPU: world_size 2, gloo,
in the style of tests/test_chanhist_dp_gloo.py.  The sum a device-served layer keeps is stood in for by CPU tensors: step()'s
covariance is the mean of the two ranks' averages, the correlation matrix, the per-channel redundancy and the effective rank
are derived from it, and ranks that buffered different numbers of forwards are refused."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

COV, RHO, MAXR, RANK = ("channel_covariance_matrix", "channel_correlation_matrix", "max_abs_correlation_per_channel",
                        "effective_rank")
FOUR = (COV, RHO, MAXR, RANK)
C_ = 4


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _cov(rank, fwd):
    """the float64 covariance of forward `fwd` on rank `rank`: positive definite, different on every (rank, forward)"""
    g = torch.Generator().manual_seed(10 * rank + fwd)
    a = torch.randn((C_, 12), generator=g, dtype=torch.float64) * (1.0 + rank)
    a[3] = a[0] * (2.0 + fwd) + a[3] * 0.01 * rank  # channel 3 nearly a copy of channel 0
    return a @ a.T / 11.0


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tracking.monitor import ActivityMonitor, _CovSum

        def run(forwards, sync=True):
            mon = ActivityMonitor(torch.nn.Identity(), {"enabled": True, "track_interval": 1, "sync_across_ranks": sync})
            acc = _CovSum(device_served=True)
            for f in range(forwards):
                acc.add(_cov(rank, f))
            for m in FOUR:
                mon.hook_collected_buffer["layer.output"][m].append(acc)
            log = mon.step(1)
            return ({k: np.asarray(v).tolist() for k, v in mon.get_data_for_step(1)["layer.output"].items()},
                    {k: float(v) for k, v in log.items()})

        synced, local = run(2), run(2, sync=False)
        try:
            run(2 + rank)
            refused = ""
        except RuntimeError as e:
            refused = str(e)
        q.put((rank, synced, local, refused))
    finally:
        dist.destroy_process_group()


def test_step_averages_the_covariance_over_the_ranks_world2():
    from tracking.monitor import correlation_summary
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
    per_rank = [((_cov(r, 0) + _cov(r, 1)) / 2).numpy() for r in range(2)]
    want = (per_rank[0] + per_rank[1]) / 2
    for rank, (synced, slog), (local, _), refused in out:
        assert list(synced) == list(FOUR)
        assert np.allclose(synced[COV], want, rtol=1e-14, atol=0)
        s = correlation_summary(np.array(synced[COV]), 0.95)  # the summary is derived from the averaged covariance
        assert np.array_equal(np.array(synced[RHO], dtype=np.float32), s["correlation"].astype(np.float32))
        assert np.array_equal(np.array(synced[MAXR], dtype=np.float32), s["max_abs"].astype(np.float32))
        assert synced[RANK] == s["effective_rank"] and synced[MAXR][0] > 0.95 and synced[MAXR][3] > 0.95
        assert slog["tracking/layer.output/" + RANK] == synced[RANK]
        assert slog["tracking/layer.output/" + MAXR + "_overall_max"] == max(synced[MAXR])
        assert abs(slog["tracking/layer.output/" + RHO + "_mean_abs_offdiag"] - s["mean_abs_offdiag"]) <= 1e-6
        # without sync_across_ranks a rank sees its own forwards only
        assert np.allclose(local[COV], per_rank[rank], rtol=1e-14, atol=0)
        assert local[RANK] == correlation_summary(np.array(local[COV]))["effective_rank"] != synced[RANK]
        assert "different numbers of forwards" in refused
    assert out[0][1][0] == out[1][1][0]  # both ranks hold the same aggregate
