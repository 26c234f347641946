"""ActivityMonitor.step() on the gradient metrics of `output_grad` under data parallelism, on CPU: world_size 2, gloo, in the
style of tests/test_chancov_dp_gloo.py.  Each rank runs the hook path on a plain module with its own data: step()'s three sums
are the mean of the two ranks' values, the maxima are maxed on their bit patterns (a NaN on one rank stays), without
sync_across_ranks a rank sees its own passes only, and ranks that buffered different numbers of passes are refused."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

MEAN, AMAX, GAIN, SAL = ("mean_abs_gradient_per_channel", "abs_max_gradient_per_channel", "gain_gradient_per_channel",
                         "taylor_saliency_per_channel")
FOUR = (MEAN, AMAX, GAIN, SAL)
C_ = 4


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pair(rank, fwd, nan=False):
    """(output, gradient) of backward pass `fwd` on rank `rank`, NCHW: different on every (rank, pass)"""
    g = torch.Generator().manual_seed(10 * rank + fwd)
    a = torch.randn((2, C_, 3, 5), generator=g) * (1.0 + rank)
    d = torch.randn((2, C_, 3, 5), generator=g) * 0.1 * (1.0 + fwd)
    d[:, 3] = 0.0  # a channel without gradient on every rank
    if nan and rank == 1:
        d[0, 1, 0, 0] = float("nan")
    return a, d


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tracking.monitor import ActivityMonitor

        def run(passes, sync=True, nan=False):
            cfg = {"enabled": True, "track_interval": 1, "sync_across_ranks": sync,
                   "target_layers": [{"name": "0", "capture_point": "output_grad", "metrics": list(FOUR)}]}
            mon = ActivityMonitor(torch.nn.Sequential(torch.nn.Identity()), cfg)
            for f in range(passes):
                a, d = _pair(rank, f, nan)
                x = a.clone().requires_grad_(True)
                mon.model(x).backward(d)  # the hook keeps the output (= a) and receives d as its gradient
            log = mon.step(1)
            return ({k: np.asarray(v).tolist() for k, v in mon.get_data_for_step(1)["0.output_grad"].items()},
                    {k: float(v) for k, v in log.items()})

        synced, local, with_nan = run(2), run(2, sync=False), run(2, nan=True)
        try:
            run(2 + rank)
            refused = ""
        except RuntimeError as e:
            refused = str(e)
        q.put((rank, synced, local, with_nan, refused))
    finally:
        dist.destroy_process_group()


def _local(rank, passes=2):
    """what a rank's own step() gives: per pass the fp32 of compute_grad_metrics, then the mean / maximum over the passes"""
    from tracking.monitor import compute_grad_metrics
    rows = [compute_grad_metrics(*_pair(rank, f)) for f in range(passes)]
    return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


def test_step_averages_the_sums_and_maxes_the_maxima_over_the_ranks_world2():
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
    sums = [_local(r)[0] for r in range(2)]
    amax = [_local(r)[1] for r in range(2)]
    row = {MEAN: 0, GAIN: 1, SAL: 2}

    def stepped(per_pass_f64):  # fp32 per pass, then the unweighted mean over the passes, as step() does
        return np.mean(per_pass_f64.numpy().astype(np.float32), axis=0)

    for rank, (synced, slog), (local, _), (with_nan, nlog), refused in out:
        assert list(synced) == list(FOUR)
        for m, i in row.items():
            want = stepped((sums[0][:, i] + sums[1][:, i]) / 2)  # averaged across the ranks in float64, per pass
            assert np.array_equal(np.array(synced[m], dtype=np.float32), want), m
            assert np.array_equal(np.array(local[m], dtype=np.float32), stepped(sums[rank][:, i])), m
        both = torch.maximum(amax[0], amax[1]).amax(dim=0).numpy()
        assert np.array_equal(np.array(synced[AMAX], dtype=np.float32), both)
        assert np.array_equal(np.array(local[AMAX], dtype=np.float32), amax[rank].amax(dim=0).numpy())
        assert synced[MEAN][3] == synced[SAL][3] == synced[AMAX][3] == 0.0 and synced[GAIN][3] == 0.0
        base = "tracking/0.output_grad/"
        assert slog[base + AMAX + "_overall_max"] == max(synced[AMAX])
        assert slog[base + SAL + "_overall_max"] == max(synced[SAL])
        assert abs(slog[base + GAIN + "_overall_mean"] - np.mean(synced[GAIN])) <= 1e-6 * max(abs(v) for v in synced[GAIN])
        # a NaN gradient on rank 1 only: the maximum of channel 1 is NaN on BOTH ranks, the other channels are what they were
        assert np.isnan(with_nan[AMAX][1]) and np.isnan(nlog[base + AMAX + "_overall_max"])
        assert [with_nan[AMAX][c] for c in (0, 2, 3)] == [synced[AMAX][c] for c in (0, 2, 3)]
        assert "different numbers of forwards" in refused
    assert out[0][1][0] == out[1][1][0]  # both ranks hold the same aggregate
