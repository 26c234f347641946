"""ActivityMonitor with the reference's API and aggregation semantics
(reference src/tracking/monitor.py:11-274), served by fused device-side reductions.

Same constructor, layer ids (`f"{name}.{capture_point}"`), `step()` keys, `get_data_for_step`,
`export_all_processed_data_to_records`, `remove_hooks`.  What changes is WHERE the numbers come
from: when a target layer belongs to the HIP engine and asks only for
`mean_abs_activation_per_channel`, no torch hook is registered; the engine emits the per-channel
vector from a fused reduction (no activation tensor, no device->host sync per forward -- the
reference does `.cpu().numpy()` inside every hook, monitor.py:67).  Vectors stay on the device
until `step()`, which performs ONE transfer per layer.  Any other metric / any foreign model
falls back to ordinary forward hooks with the reference's formulas.

Reference quirks kept on purpose: values are appended on EVERY forward, train or
eval (validation pollutes the buffer, monitor.py:98-101); `step()` takes the UNWEIGHTED mean over
the buffered forwards (monitor.py:181-182); `full_activation_map` keeps only the first
(monitor.py:166-167).
Deliberate fix: under data parallelism the buffered vectors are averaged across ranks in step()
(the reference classifies rank-0-local statistics, train.py:311).

`tracking.device_metrics: true` (opt-in) serves every other engine target with a 4-D capture point and any subset of the
four metrics from the device as well (`device_layers`): one moments vector per forward (ops.moments: per-channel mean
|A|, mean, unbiased std) on the tensor the hook would have received, and a `full_activation_map` snapshot on the first
forward after the last step() only (step() keeps only that one).  step() makes one transfer per layer and aggregates
exactly as the hook path does; the scalars stay rank-local like the hook path's, the mean |A| vectors are averaged
across ranks like the fused ones.

Three metrics the reference does not have, valid for any layer and capture point (CHANHIST_METRICS):
`log2_histogram_per_channel` (int64 [C][48] counts over batch and pixels, bin = clamp(floor(log2 |A|) + 31, 0, 47) from the
fp32 exponent: bin 0 is |A| < 2^-30, bin 47 is |A| >= 2^16, inf and NaN -- what fp16 cannot hold), `abs_max_activation_per_channel`
(fp32 [C], NaN if the channel holds one) and `near_zero_fraction_per_channel` (fp32 [C], share of |A| <
`tracking.near_zero_threshold`, default 1e-3).  They tell a dead channel from a small one and find outlier channels without a
full map.  Hooks compute them with torch (compute_metrics); a device-served layer gets all three from ONE ops.chanhist pass
per forward.  step() sums the histograms over the buffered forwards, takes the maximum of the maxima and the unweighted mean
of the fractions; device-served layers sum / max / average them across ranks as well and come to the host in one transfer.

Four more answer "which channels carry the same signal" (CHANCOV_METRICS, any layer and capture point):
`channel_covariance_matrix` (float64 [C][C], unbiased over batch and all trailing axes, channel = dim 1),
`channel_correlation_matrix` (fp32 [C][C]; 0 wherever a variance is <= 0, the diagonal 1 on live channels),
`max_abs_correlation_per_channel` (fp32 [C], max over c' != c of |rho|: a channel near 1 is a copy of another) and
`effective_rank` (tr(cov)^2 / ||cov||_F^2, the participation ratio: how many directions the layer uses).  All four derive from
ONE covariance per forward: torch.cov in the hook (compute_metrics), ONE ops.chancov pass on a device-served layer.  A layer
keeps a running float64 sum and a forward count, not a list; step() averages it over the forwards (device-served: across
ranks too), brings it to the host in one transfer and derives the rest in float64 with correlation_summary().

Four metrics of the BACKWARD pass, valid only at the capture point `output_grad` (CHANGRAD_METRICS; layer id
`f"{name}.output_grad"`), with a the module's output, g the gradient of the loss with respect to it as the backward carries it
(the 1 / gradient_accumulation_steps factor included, rank-local) and N = B * H * W: `mean_abs_gradient_per_channel` (sum |g| / N),
`abs_max_gradient_per_channel` (max |g|, NaN if the channel holds one), `gain_gradient_per_channel` (sum_b sum_p a g: dL/ds_c at
s_c = 1 for an output multiplied by a per-channel gain, minus the first-order change of the loss when the channel is zeroed) and
`taylor_saliency_per_channel` ((1 / B) sum_b |sum_p a g|, the Taylor criterion of Molchanov et al. 2017 without the per-layer
normalisation).  A channel with tiny |A| that still receives gradient is recoverable; one without is dead.  Values are buffered
once per backward pass that computes that gradient (an eval forward buffers nothing, a micro-batch of an accumulated update one
entry).  A plain torch module gets a forward hook that keeps the output and a tensor hook on it (compute_grad_metrics); an
engine module gets Engine.add_grad_tracker, whatever `device_metrics` says (no torch hook sees the engine's inner gradients):
ONE ops.changrad pass over the pair per backward.  step() takes the unweighted mean of the three sums over the buffered passes
and the maximum of the maxima (a NaN stays); across ranks the sums are averaged and the maxima maxed on their bit patterns, with
one host transfer per layer.

Five metrics look at a channel the way GroupNorm does, per SAMPLE and per GROUP (CHANGROUP_METRICS, any layer, capture points
`input` / `output`).  With n = H * W, cg = C / G, g(c) = c // cg, mu_bg the mean of group g in sample b, v_bc = sum_p (y - mu_bg)^2
and V_bg = sum_{c in g} v_bc: `group_variance_share_per_channel` (mean over samples of v_bc / V_bg, 0 where V_bg is 0: 1 / cg
means equal partners, near 1 the channel owns its group, near 0 it is squashed by a neighbour), `normalized_rms_per_channel` (mean of
sqrt((v_bc / n) / (V_bg / (n cg) + eps)): the channel's RMS as the norm passes it on, before gamma), `group_dominance_per_group`
([G], mean of max_{c in g} share), `active_sample_fraction_per_channel` (share of samples whose m_bc = mean_p |y| reaches
`tracking.near_zero_threshold`) and `sample_variation_per_channel` (population std of m_bc over the samples divided by its mean,
0 where the mean is 0: high for an input-selective channel, 0 for one that is equally active everywhere).  G and eps are the
module's own on a GroupNorm, `tracking.group_count` (32) and `tracking.group_eps` (1e-6) elsewhere, a target's `groups:` over
both; a target whose channels do not divide into G groups is refused if it names one of the first three.  All five derive from
the per-(sample, channel) sums of y, y^2 and |y| (per_sample_sums in a hook, ONE ops.changroup pass on a device-served layer)
through ops.changroup_metrics, whose result -- sums over the samples and the sample count -- is what a layer keeps: forwards
and ranks combine by adding, exactly, whatever their batch sizes; step() makes one transfer per layer.
"""
import logging
from collections import defaultdict
from typing import Any, Callable, Dict, List, Optional

import numpy as np
import torch

logger = logging.getLogger(__name__)

FUSED_METRIC = "mean_abs_activation_per_channel"
HIST_METRIC = "log2_histogram_per_channel"
ABSMAX_METRIC = "abs_max_activation_per_channel"
NEARZERO_METRIC = "near_zero_fraction_per_channel"
CHANHIST_METRICS = (HIST_METRIC, ABSMAX_METRIC, NEARZERO_METRIC)
KNOWN_METRICS = (FUSED_METRIC, "full_activation_map", "mean_activation", "std_activation") + CHANHIST_METRICS
HIST_BINS = 48             # bin = clamp(floor(log2 |y|) + 31, 0, 47), from the fp32 exponent field
NEAR_ZERO_THRESHOLD = 1e-3  # default of tracking.near_zero_threshold
DEAD_FRACTION = 0.99       # a channel with at least this share of near-zero values counts as dead in the records
COV_METRIC = "channel_covariance_matrix"
CORR_METRIC = "channel_correlation_matrix"
MAXCORR_METRIC = "max_abs_correlation_per_channel"
RANK_METRIC = "effective_rank"
CHANCOV_METRICS = (COV_METRIC, CORR_METRIC, MAXCORR_METRIC, RANK_METRIC)  # accepted beside KNOWN_METRICS; one covariance serves all
MEANGRAD_METRIC = "mean_abs_gradient_per_channel"
ABSMAXGRAD_METRIC = "abs_max_gradient_per_channel"
GAINGRAD_METRIC = "gain_gradient_per_channel"
SALIENCY_METRIC = "taylor_saliency_per_channel"
# valid only at GRAD_POINT; one pass over (output, gradient) serves all (the first, third and fourth are the rows of its sums)
CHANGRAD_METRICS = (MEANGRAD_METRIC, ABSMAXGRAD_METRIC, GAINGRAD_METRIC, SALIENCY_METRIC)
GRAD_POINT = "output_grad"
SHARE_METRIC = "group_variance_share_per_channel"
NRMS_METRIC = "normalized_rms_per_channel"
DOMINANCE_METRIC = "group_dominance_per_group"
ACTIVE_METRIC = "active_sample_fraction_per_channel"
VARIATION_METRIC = "sample_variation_per_channel"
GROUP_METRICS = (SHARE_METRIC, NRMS_METRIC, DOMINANCE_METRIC)  # need C % G == 0
SAMPLE_METRICS = (ACTIVE_METRIC, VARIATION_METRIC)
CHANGROUP_METRICS = GROUP_METRICS + SAMPLE_METRICS  # accepted beside KNOWN_METRICS; one pass of per-sample sums serves all
GROUP_COUNT = 32      # default of tracking.group_count (the VAE's GroupNorm(32))
GROUP_EPS = 1e-6      # default of tracking.group_eps
SQUASHED_SHARE = 0.1  # a channel whose variance share is below this fraction of the uniform share 1 / cg counts as squashed
ZERO_GRADIENT_THRESHOLD = 0.0  # default of tracking.zero_gradient_threshold: a channel whose mean |g| is not above it got no gradient
REDUNDANCY_THRESHOLD = 0.95  # default of tracking.redundancy_threshold: |rho| above it marks a redundant pair / channel


def _resolve(root: torch.nn.Module, dotted: str) -> torch.nn.Module:
    """getattr chain with a `.module` fallback at every level (DDP-wrapped roots), monitor.py:41-54."""
    cur = root
    for part in dotted.split("."):
        if hasattr(cur, part):
            cur = getattr(cur, part)
        elif hasattr(cur, "module") and hasattr(cur.module, part):
            cur = getattr(cur.module, part)
        else:
            raise AttributeError(f"Model (or its .module) does not have a layer named '{dotted}' (path: {part})")
    return cur


def _per_channel(tensor: torch.Tensor) -> torch.Tensor:
    """fp32 [C, N]: the values of each channel (dim 1, as FUSED_METRIC reduces); a tensor without a channel axis is one channel"""
    t = tensor.detach().float()
    if t.ndim >= 2:
        return t.transpose(0, 1).reshape(t.shape[1], -1)
    return t.reshape(1, -1)


def log2_bins(t32: torch.Tensor) -> torch.Tensor:
    """bin of every fp32 value, from its exponent field E: clamp(E - 96, 0, 47) = clamp(floor(log2 |y|) + 31, 0, 47).  Bin 0:
    |y| < 2^-30 (zeros, denormals); bin 47: |y| >= 2^16, inf, NaN (what fp16 cannot hold)"""
    e = (t32.contiguous().view(torch.int32) >> 23) & 0xFF
    return (e - 96).clamp_(0, HIST_BINS - 1).long()


def _near_zero_fraction(count, n) -> np.ndarray:
    """counts of |y| < tau over n values each -> the fp32 fraction (one rounding, of the float64 quotient)"""
    return (np.asarray(count, dtype=np.float64) / np.asarray(n, dtype=np.float64)).astype(np.float32)


def correlation_summary(cov: np.ndarray, redundancy_threshold: float = REDUNDANCY_THRESHOLD) -> Dict[str, Any]:
    """everything the CHANCOV_METRICS report, from a channel covariance, on the host in float64:
    correlation [C, C] = cov / sqrt(var_c var_c'), 0 wherever either variance is <= 0 (so its diagonal is 1 on live channels
    and 0 on dead ones); max_abs [C] = max over c' != c of |rho| (0 for C = 1); effective_rank = tr(cov)^2 / ||cov||_F^2, 0
    when the trace is 0; mean_abs_offdiag / max_abs_offdiag of rho and of cov (cov_*); redundant_pairs = pairs c < c' with
    |rho| above the threshold, redundant_channels = channels whose max_abs is above it"""
    cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
    Cc = cov.shape[0]
    var = np.diag(cov)
    live = var > 0
    sd = np.sqrt(np.where(live, var, 1.0))
    rho = np.where(live[:, None] & live[None, :], cov / (sd[:, None] * sd[None, :]), 0.0)
    np.fill_diagonal(rho, live.astype(np.float64))  # exactly 1 on live channels, whatever sqrt rounds to
    off = ~np.eye(Cc, dtype=bool)
    arho = np.where(off, np.abs(rho), 0.0)
    acov = np.where(off, np.abs(cov), 0.0)
    max_abs = arho.max(axis=1) if Cc > 1 else np.zeros(Cc)
    tr, fro2 = float(np.trace(cov)), float(np.sum(cov * cov))
    npairs = max(Cc * (Cc - 1), 1)
    return {"correlation": rho, "max_abs": max_abs, "effective_rank": tr * tr / fro2 if tr > 0 and fro2 > 0 else 0.0,
            "mean_abs_offdiag": float(arho.sum() / npairs), "max_abs_offdiag": float(arho.max()) if Cc > 1 else 0.0,
            "cov_mean_abs_offdiag": float(acov.sum() / npairs), "cov_max_abs_offdiag": float(acov.max()) if Cc > 1 else 0.0,
            "redundant_pairs": int((np.triu(arho, 1) > redundancy_threshold).sum()),
            "redundant_channels": int((max_abs > redundancy_threshold).sum())}


def channel_covariance(tensor: torch.Tensor) -> torch.Tensor:
    """float64 [C, C] on the tensor's device: unbiased covariance of the channels (dim 1) over batch and all trailing axes"""
    yc = _per_channel(tensor).double()
    return torch.cov(yc).reshape(yc.shape[0], yc.shape[0])


def per_sample_sums(tensor: torch.Tensor) -> torch.Tensor:
    """what ops.changroup computes, with torch on the tensor's device: float64 [B, C, 3] = sum y, sum y^2, sum |y| over all
    trailing axes of every (sample, channel).  Channel is dim 1; a tensor without a channel axis is one channel of one sample.
    The stored values are widened exactly, so every square is exact and every sum float64."""
    t = tensor.detach()
    t3 = t.reshape(t.shape[0], t.shape[1], -1) if t.ndim >= 2 else t.reshape(1, 1, -1)
    y = t3.double()
    return torch.stack([y.sum(dim=2), (y * y).sum(dim=2), y.abs().sum(dim=2)], dim=2)


def changroup_summary(chan: np.ndarray, grp: np.ndarray, samples: float) -> Dict[str, np.ndarray]:
    """the five CHANGROUP_METRICS from the sufficient sums a layer keeps (ops.changroup_metrics, added over forwards and ranks):
    chan float64 [5, C] = sums over the samples of share, nrms, m, m^2, [m >= tau]; grp [G] = sum of dom; in float64 on the host"""
    chan, S = np.asarray(chan, dtype=np.float64), float(samples)
    mean = chan[2] / S
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.where(chan[3] / S - mean * mean < 0.0, 0.0, chan[3] / S - mean * mean)  # (a NaN stays)
        variation = np.where(mean == 0.0, 0.0, np.sqrt(var) / mean)
    return {SHARE_METRIC: (chan[0] / S).astype(np.float32), NRMS_METRIC: (chan[1] / S).astype(np.float32),
            DOMINANCE_METRIC: (np.asarray(grp, dtype=np.float64) / S).astype(np.float32),
            ACTIVE_METRIC: (chan[4] / S).astype(np.float32), VARIATION_METRIC: variation.astype(np.float32)}


def compute_grad_metrics(a: torch.Tensor, g: torch.Tensor):
    """what ops.changrad computes, with torch on the tensors' device: (sums float64 [3, C], absmax fp32 [C]); the rows of sums are
    mean |g| over batch and all trailing axes, the gain gradient sum_b sum_p a g and the saliency (1 / B) sum_b |sum_p a g|.
    Channel is dim 1 (as _per_channel); a tensor without a channel axis is one channel of one image.  The stored values
    (whatever their dtype) are widened exactly, so every product is exact and every sum float64."""
    a, g = a.detach(), g.detach()
    if tuple(a.shape) != tuple(g.shape):
        raise ValueError(f"output {tuple(a.shape)} and its gradient {tuple(g.shape)} differ")
    if a.ndim >= 2:
        a3, g3 = a.reshape(a.shape[0], a.shape[1], -1), g.reshape(g.shape[0], g.shape[1], -1)
    else:
        a3, g3 = a.reshape(1, 1, -1), g.reshape(1, 1, -1)
    g64 = g3.double()
    P = (a3.double() * g64).sum(dim=2)  # [B, C]
    n = g3.shape[0] * g3.shape[2]
    sums = torch.stack([g64.abs().sum(dim=(0, 2)) / n, P.sum(dim=0), P.abs().sum(dim=0) / g3.shape[0]])
    absmax = g3.float().abs().amax(dim=(0, 2))  # NaN propagates
    return sums, absmax


def compute_metrics(tensor: torch.Tensor, metrics: List[str], near_zero_threshold: float = NEAR_ZERO_THRESHOLD,
                    group: Optional[tuple] = None) -> Dict[str, Any]:
    """slow-path formulas, identical to monitor.py:56-80; the three CHANHIST_METRICS are what ops.chanhist computes.  Each of
    the CHANCOV_METRICS named gets the forward's float64 covariance (one tensor, shared, on the tensor's device): step()
    derives the metric from the average over the forwards.  Each of the CHANGROUP_METRICS named gets the forward's
    (chan, grp, samples) of ops.changroup_metrics on per_sample_sums(tensor) (one tuple, shared); group = (G or None, eps)."""
    out: Dict[str, Any] = {}
    cov = None
    gsum, group_ok = None, True
    if not isinstance(tensor, torch.Tensor):
        logger.warning(f"Cannot calculate metrics for non-tensor type: {type(tensor)}")
        return out
    for name in metrics:
        try:
            if name in CHANCOV_METRICS:
                if cov is None:
                    cov = channel_covariance(tensor)
                out[name] = cov
            elif name in CHANGROUP_METRICS:
                if gsum is None:  # once per tensor, whatever happens
                    from vaehip.ops import changroup_metrics
                    G, eps = group if group is not None else (GROUP_COUNT, GROUP_EPS)
                    sums = per_sample_sums(tensor)
                    hw = int(np.prod(tensor.shape[2:])) if tensor.ndim >= 2 else tensor.numel()
                    if G is not None and sums.shape[1] % G:  # the sample metrics are still served
                        logger.error(f"Metrics {[m for m in metrics if m in GROUP_METRICS]}: {sums.shape[1]} channels do not divide "
                                     f"into {G} groups.")
                        G, group_ok = None, False
                    gsum = changroup_metrics(sums, hw, G, eps, near_zero_threshold)
                if group_ok or name in SAMPLE_METRICS:
                    out[name] = gsum
            elif name == HIST_METRIC:
                yc = _per_channel(tensor)
                idx = log2_bins(yc) + torch.arange(yc.shape[0], device=yc.device)[:, None] * HIST_BINS
                out[name] = torch.bincount(idx.flatten(), minlength=yc.shape[0] * HIST_BINS).view(-1, HIST_BINS).cpu().numpy()
            elif name == ABSMAX_METRIC:
                out[name] = _per_channel(tensor).abs().amax(dim=1).cpu().numpy()  # NaN propagates
            elif name == NEARZERO_METRIC:
                yc = _per_channel(tensor)
                tau = torch.tensor(near_zero_threshold, dtype=torch.float32, device=yc.device)
                out[name] = _near_zero_fraction((yc.abs() < tau).sum(dim=1).cpu().numpy(), yc.shape[1])  # NaN is not below
            elif name == FUSED_METRIC:
                if tensor.ndim >= 2:
                    dims = [0] + list(range(2, tensor.ndim))
                    out[name] = tensor.abs().mean(dim=dims).detach().cpu().numpy()
                else:
                    out[name] = tensor.abs().mean().detach().cpu().numpy()
            elif name == "full_activation_map":
                out[name] = tensor.detach().clone().cpu()
            elif name == "mean_activation":
                out[name] = tensor.mean().detach().cpu().numpy()
            elif name == "std_activation":
                out[name] = tensor.std().detach().cpu().numpy()
            else:
                logger.warning(f"Unknown metric '{name}' requested.")
        except Exception as e:  # metric failures are swallowed, monitor.py:78-79
            logger.error(f"Error calculating metric '{name}': {e}", exc_info=True)
    return out


class _Moments:
    """a buffered per-forward moments vector of a device-served layer (resolved to host values in step())"""
    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        self.t = t


class _ChanHist:
    """a buffered per-forward (hist, nzero, absmax) triple of a device-served layer (ops.chanhist; resolved in step())"""
    __slots__ = ("t",)

    def __init__(self, t: tuple):
        self.t = t


class _ChanGrad:
    """a buffered per-backward (sums float64 [3, C], absmax fp32 [C]) pair (ops.changrad on an engine layer,
    compute_grad_metrics in a hook; resolved in step()), shared by the CHANGRAD_METRICS the layer tracks"""
    __slots__ = ("t",)

    def __init__(self, t: tuple):
        self.t = t


class _GradHookHandle:
    """the forward hook of an `output_grad` target on a plain module; remove() also silences tensor hooks already placed"""

    def __init__(self, handle, state: dict):
        self._h, self._state = handle, state

    def remove(self):
        self._state["on"] = False
        self._h.remove()


class _CovSum:
    """a layer's running float64 sum of per-forward channel covariances and their count, shared by the CHANCOV_METRICS the
    layer tracks (resolved in step()); device_served: filled by ops.chancov, and averaged across ranks like the other
    device-served vectors"""
    __slots__ = ("sum", "n", "device_served")

    def __init__(self, device_served: bool = False):
        self.sum, self.n, self.device_served = None, 0, device_served

    def add(self, cov: torch.Tensor):
        self.sum = cov.clone() if self.sum is None else self.sum.add_(cov)  # a copy: the engine shares cov among its trackers
        self.n += 1


class _GroupSum:
    """a layer's running sums of ops.changroup_metrics results -- chan float64 [5, C], grp float64 [G] and the sample count --
    shared by the CHANGROUP_METRICS the layer tracks (resolved in step()); added over the ranks as well unless sync is off"""
    __slots__ = ("chan", "grp", "samples", "forwards")

    def __init__(self):
        self.chan, self.grp, self.samples, self.forwards = None, None, 0, 0

    def add(self, chan: torch.Tensor, grp: torch.Tensor, samples: int):
        # copies: the engine shares one result among its trackers
        self.chan = chan.clone() if self.chan is None else self.chan.add_(chan)
        self.grp = grp.clone() if self.grp is None else self.grp.add_(grp)
        self.samples += int(samples)
        self.forwards += 1


def _buffer_group(buf, name: str, res: tuple, seen: set):
    """add a forward's (chan, grp, samples) to the layer's running sums (once per forward: `seen`) and list them under `name`"""
    acc = next((buf[m][0] for m in CHANGROUP_METRICS if m in buf and buf[m]), None)
    if acc is None:
        acc = _GroupSum()
    if id(acc) not in seen:
        seen.add(id(acc))
        acc.add(*res)
    if not buf[name]:
        buf[name].append(acc)


def _buffer_cov(buf, name: str, cov: torch.Tensor, device_served: bool, seen: set):
    """add a forward's covariance to the layer's running sum (once per forward: `seen`) and list the sum under `name`"""
    acc = next((buf[m][0] for m in CHANCOV_METRICS if m in buf and buf[m]), None)
    if acc is None:
        acc = _CovSum(device_served)
    if id(acc) not in seen:
        seen.add(id(acc))
        acc.add(cov)
    if not buf[name]:
        buf[name].append(acc)


class ActivityMonitor:
    def __init__(self, model: torch.nn.Module, tracking_config: Dict[str, Any]):
        self.model = model
        self.config = tracking_config
        self.target_layers_config: List[Dict[str, Any]] = self.config.get("target_layers", [])
        self.hook_collected_buffer = defaultdict(lambda: defaultdict(list))
        self.processed_data_by_step = defaultdict(dict)
        self.hooks: list = []
        self.fused_layers: List[str] = []
        self.device_layers: List[str] = []
        self.device_metrics = bool(self.config.get("device_metrics", False))
        self.sync_across_ranks = bool(self.config.get("sync_across_ranks", True))
        self.near_zero_threshold = float(self.config.get("near_zero_threshold", NEAR_ZERO_THRESHOLD))
        self.redundancy_threshold = float(self.config.get("redundancy_threshold", REDUNDANCY_THRESHOLD))
        self.group_count = int(self.config.get("group_count", GROUP_COUNT))
        self.group_eps = float(self.config.get("group_eps", GROUP_EPS))
        self._groups: Dict[str, tuple] = {}  # layer id -> (G or None, eps) of its CHANGROUP_METRICS
        self._refused: set = set()  # layer ids dropped at their first forward: channels unknown at registration, C % G != 0
        self.zero_gradient_threshold = float(self.config.get("zero_gradient_threshold", ZERO_GRADIENT_THRESHOLD))
        if self.config.get("enabled", False):
            self._register_hooks()
            logger.info(f"ActivityMonitor initialized for {len(self.target_layers_config)} target(s) "
                        f"({len(self.fused_layers)} fused on device"
                        + (f", {len(self.device_layers)} device-served" if self.device_metrics else "") + ").")
        else:
            logger.info("ActivityMonitor is disabled in config.")

    # ------------------------------------------------------------------ registration
    def _sink(self, layer_id: str) -> Callable[[torch.Tensor], None]:
        def sink(vec: torch.Tensor):
            self.hook_collected_buffer[layer_id][FUSED_METRIC].append(vec)
        return sink

    def _device_sink(self, layer_id: str, metrics: List[str]) -> Callable:
        """engine sink of a device-served layer: buffers device tensors only, one entry per metric in config order (the
        order compute_metrics appends in); the moments vector and the histogram triple are shared by the metrics they serve,
        the covariance and the per-sample sums' metrics go into the layer's running sums"""
        def sink(mom: Optional[torch.Tensor], fmap: Optional[torch.Tensor], chanhist: Optional[tuple] = None,
                 chancov: Optional[tuple] = None, changroup: Optional[tuple] = None):
            buf = self.hook_collected_buffer[layer_id]
            gres = None
            if changroup is not None and self._undivided(layer_id, changroup[0].shape[1]):
                return
            hist = _ChanHist(chanhist) if chanhist is not None else None
            seen: set = set()
            for name in metrics:
                if name == "full_activation_map":
                    if fmap is not None:
                        buf[name].append(fmap)
                elif name in CHANCOV_METRICS:
                    _buffer_cov(buf, name, chancov[0], True, seen)
                elif name in CHANGROUP_METRICS:
                    if gres is None:  # B * C numbers, torch ops on the device: nothing synchronises the host
                        from vaehip.ops import changroup_metrics
                        G, eps = self._groups[layer_id]
                        gres = changroup_metrics(changroup[0], changroup[1], G, eps, self.near_zero_threshold)
                    _buffer_group(buf, name, gres, seen)
                elif name in CHANHIST_METRICS:
                    buf[name].append(hist)
                else:
                    buf[name].append(_Moments(mom))
        return sink

    def _grad_sink(self, layer_id: str, metrics: List[str]) -> Callable:
        """sink of an `output_grad` target: one (sums, absmax) pair per backward pass, listed under every metric asked for"""
        def sink(sums: torch.Tensor, absmax: torch.Tensor):
            entry = _ChanGrad((sums, absmax))
            buf = self.hook_collected_buffer[layer_id]
            for name in metrics:
                buf[name].append(entry)
        return sink

    def _grad_hook(self, layer_id: str, metrics: List[str], state: dict) -> Callable:
        """forward hook of an `output_grad` target on a plain module: keeps the output and, if a gradient will reach it, places
        a tensor hook that computes the metrics when it does (an eval forward under no_grad places none)"""
        sink = self._grad_sink(layer_id, metrics)

        def fn(module, hook_input, hook_output):
            out = hook_output
            if not (isinstance(out, torch.Tensor) and out.requires_grad and state["on"]):
                return

            def on_grad(grad):
                if state["on"]:
                    try:
                        sink(*compute_grad_metrics(out, grad))
                    except Exception as e:  # metric failures are swallowed, as compute_metrics does
                        logger.error(f"Error calculating gradient metrics for {layer_id}: {e}", exc_info=True)
            out.register_hook(on_grad)
        return fn

    def _map_due(self, layer_id: str) -> Callable[[], bool]:
        """a snapshot is taken while the buffer holds none: the first forward after the last step() (step() keeps values[0])"""
        def due():
            return not self.hook_collected_buffer.get(layer_id, {}).get("full_activation_map")
        return due

    def _hook(self, layer_id: str, metrics: List[str], point: str) -> Callable:
        def fn(module, hook_input, hook_output=None):
            if point == "input":
                t = hook_input[0] if isinstance(hook_input, tuple) and hook_input else hook_input
            else:
                t = hook_output
            if isinstance(t, torch.Tensor):
                if layer_id in self._groups and self._undivided(layer_id, t.shape[1] if t.ndim >= 2 else 1):
                    return
                seen: set = set()
                for k, v in compute_metrics(t, metrics, self.near_zero_threshold, self._groups.get(layer_id)).items():
                    if k in CHANCOV_METRICS:
                        _buffer_cov(self.hook_collected_buffer[layer_id], k, v, False, seen)
                    elif k in CHANGROUP_METRICS:
                        _buffer_group(self.hook_collected_buffer[layer_id], k, v, seen)
                    else:
                        self.hook_collected_buffer[layer_id][k].append(v)
        return fn

    def _register_hooks(self):
        self.remove_hooks()
        self.hook_collected_buffer.clear()
        for conf in self.target_layers_config:
            name = conf.get("name")
            point = conf.get("capture_point", "output")
            if not name:
                logger.warning("Skipping a target_layer entry with no name.")
                continue
            layer_id = f"{name}.{point}"
            metrics = conf.get("metrics", list(CHANGRAD_METRICS) if point == GRAD_POINT else [FUSED_METRIC])
            try:
                layer = _resolve(self.model, name)
                if point not in ("input", "output", GRAD_POINT):
                    logger.warning(f"Unknown capture_point '{point}' for layer {name}. Skipping.")
                    continue
                engine_ref = getattr(layer, "_vae_engine", None)
                engine = engine_ref() if engine_ref is not None else None
                if point == GRAD_POINT:
                    mlist = list(dict.fromkeys(metrics))
                    bad = [m for m in mlist if m not in CHANGRAD_METRICS]
                    if bad or not mlist:
                        logger.error(f"Capture point '{GRAD_POINT}' of layer {name} serves {CHANGRAD_METRICS}, not {bad or mlist}. "
                                     f"Skipping.")
                        continue
                    if engine is not None:  # no torch hook sees the engine's inner gradients: device_metrics or not
                        try:
                            self.hooks.append(engine.add_grad_tracker(layer, self._grad_sink(layer_id, mlist), mlist))
                        except ValueError as e:  # a GroupNorm, a module without a 4-D capture point: the engine says which
                            logger.error(f"Could not register a gradient tracker for {layer_id}: {e} Skipping.")
                            continue
                        self.device_layers.append(layer_id)
                        logger.info(f"Registered DEVICE gradient tracker for layer: {name} ({point}): {mlist}")
                    else:
                        state = {"on": True}
                        self.hooks.append(_GradHookHandle(layer.register_forward_hook(self._grad_hook(layer_id, mlist, state)), state))
                        logger.info(f"Registered FORWARD HOOK + TENSOR HOOK for layer: {name} ({point})")
                    continue
                bad = [m for m in metrics if m in CHANGRAD_METRICS]
                if bad:
                    logger.error(f"Metrics {bad} of layer {name} need capture_point '{GRAD_POINT}', not '{point}'. Skipping.")
                    continue
                if any(m in CHANGROUP_METRICS for m in metrics):
                    try:
                        self._groups[layer_id] = self._group_of(layer, point, conf, [m for m in metrics if m in GROUP_METRICS], engine)
                    except ValueError as e:
                        logger.error(f"Metrics {[m for m in metrics if m in GROUP_METRICS]} of layer {name} ({point}): {e} Skipping.")
                        continue
                if engine is not None and list(metrics) == [FUSED_METRIC]:
                    self.hooks.append(engine.add_tracker(layer, point, self._sink(layer_id)))
                    self.fused_layers.append(layer_id)
                    logger.info(f"Registered FUSED device tracker for layer: {name} ({point})")
                elif self.device_metrics and engine is not None and metrics and \
                        all(m in KNOWN_METRICS + CHANCOV_METRICS + CHANGROUP_METRICS for m in metrics) and \
                        engine.metric_trackable(layer):
                    mlist = list(dict.fromkeys(metrics))
                    extra = {"near_zero_threshold": self.near_zero_threshold} if any(m in CHANHIST_METRICS for m in mlist) else {}
                    self.hooks.append(engine.add_tracker(layer, point, self._device_sink(layer_id, mlist), metrics=mlist,
                                                         map_due=self._map_due(layer_id), **extra))
                    self.device_layers.append(layer_id)
                    logger.info(f"Registered DEVICE metric tracker for layer: {name} ({point}): {mlist}")
                elif point == "input":
                    self.hooks.append(layer.register_forward_pre_hook(self._hook(layer_id, metrics, point)))
                    logger.info(f"Registered FORWARD PRE-HOOK for layer: {name} (input)")
                else:
                    self.hooks.append(layer.register_forward_hook(self._hook(layer_id, metrics, point)))
                    logger.info(f"Registered FORWARD HOOK for layer: {name} (output)")
            except AttributeError as e:
                logger.error(f"Could not register hook for {layer_id} (AttributeError): {e}")
            except Exception as e:
                logger.error(f"Unexpected error registering hook for {layer_id}: {e}", exc_info=True)

    def _group_of(self, layer, point: str, conf: Dict[str, Any], group_metrics: List[str], engine) -> tuple:
        """(G, eps) of a target's CHANGROUP_METRICS: a `groups:` entry of the target, else the module's own on a GroupNorm, else
        tracking.group_count; eps the GroupNorm's own or tracking.group_eps.  (None, eps) when only the sample metrics are asked
        for.  ValueError: a group metric is asked for and G is not a positive integer, or the channels at the capture point do
        not divide into G groups (the 3- and 4-channel ends, the 8-channel latent moments).  Channels are known for a GroupNorm,
        a convolution and both ends of every engine module; for another torch module the first forward decides (_undivided)."""
        is_norm = isinstance(layer, torch.nn.GroupNorm)
        eps = float(layer.eps) if is_norm else self.group_eps
        if not group_metrics:
            return None, eps
        G = conf.get("groups", layer.num_groups if is_norm else self.group_count)
        if isinstance(G, bool) or not isinstance(G, int) or G < 1:
            raise ValueError(f"groups must be a positive integer, not {G!r}.")
        if is_norm:
            channels = layer.num_channels
        elif isinstance(layer, torch.nn.Conv2d):
            channels = layer.in_channels if point == "input" else layer.out_channels
        elif engine is not None and engine.metric_trackable(layer):
            channels = engine._in_channels(layer) if point == "input" else engine._out_channels(layer)
        else:
            channels = None
        if channels is not None and channels % G:
            raise ValueError(f"{channels} channels do not divide into {G} GroupNorm groups.")
        return G, eps

    def _undivided(self, layer_id: str, channels: int) -> bool:
        """at a forward: does a layer that tracks a group metric turn out to have channels that do not divide into its groups (a
        plain torch module, whose channels registration could not know)?  Then the layer is dropped, as registration would have
        dropped it, with ONE logged error; no exception leaves a forward"""
        if layer_id in self._refused:
            return True
        G = self._groups.get(layer_id, (None,))[0]
        if G is None or channels % G == 0:
            return False
        self._refused.add(layer_id)
        self.hook_collected_buffer.pop(layer_id, None)
        logger.error(f"Group metrics of layer {layer_id}: {channels} channels do not divide into {G} GroupNorm groups. "
                     f"The layer is no longer tracked.")
        return True

    def remove_hooks(self):
        for h in self.hooks:
            h.remove()
        self.hooks = []
        self.fused_layers = []
        self.device_layers = []
        self._refused = set()

    # ------------------------------------------------------------------ aggregation
    def _world(self) -> int:
        """ranks whose buffers step() combines (1 without data parallelism or with sync_across_ranks off)"""
        if self.sync_across_ranks and torch.distributed.is_available() and torch.distributed.is_initialized():
            return torch.distributed.get_world_size()
        return 1

    @staticmethod
    def _same_forward_count(forwards: int, device):
        """ranks must have buffered the same number of forwards (train.py makes them skip batches together)"""
        n = torch.tensor([forwards, -forwards], device=device, dtype=torch.int64)
        torch.distributed.all_reduce(n, op=torch.distributed.ReduceOp.MAX)
        if int(n[0]) != -int(n[1]):
            raise RuntimeError(f"ActivityMonitor: ranks buffered different numbers of forwards "
                               f"({forwards} here, {int(n[0])} max, {-int(n[1])} min); the per-rank "
                               f"tracker vectors cannot be averaged")

    def _rank_average(self, stacked: torch.Tensor) -> torch.Tensor:
        """[forwards, C] device vectors -> their average over the ranks (the identity without data parallelism)"""
        world = self._world()
        if world > 1:
            self._same_forward_count(stacked.shape[0], stacked.device)
            torch.distributed.all_reduce(stacked)
            stacked = stacked / world
        return stacked

    def _chanhist_to_host(self, metric_data: Dict[str, list]):
        """the buffered ops.chanhist triples of a layer -> per forward the host values the hook path would have buffered, in
        place: histogram int64 [C, 48], max |A| fp32 [C], near-zero fraction fp32 [C] = count / (B * H * W).  Across ranks the
        histograms are summed, the maxima maxed and the fractions averaged.  ONE transfer: a float64 [forwards, C, 50] tensor
        (counts below 2^53 and fp32 values are exact in it)"""
        rows: Dict[int, int] = {}  # id of a buffered triple -> its row
        stack = []
        for values in metric_data.values():
            for v in values:
                if isinstance(v, _ChanHist) and id(v) not in rows:
                    rows[id(v)] = len(stack)
                    stack.append(v.t)
        if not stack:
            return
        hist = torch.stack([t[0] for t in stack])
        count = hist[:, 0, :].sum(dim=1).double()  # B * H * W of each forward: what every row of its histogram sums to
        frac = torch.stack([t[1] for t in stack]).double() / count[:, None]
        amax = torch.stack([t[2] for t in stack])
        world = self._world()
        if world > 1:
            self._same_forward_count(hist.shape[0], hist.device)
            torch.distributed.all_reduce(hist)
            # as integers the bit patterns of |A| order like the values, a NaN above every number: it survives the maximum
            torch.distributed.all_reduce(amax.view(torch.int32), op=torch.distributed.ReduceOp.MAX)
            torch.distributed.all_reduce(frac)
            frac = frac / world
        host = torch.cat([hist.double(), frac[:, :, None], amax.double()[:, :, None]], dim=2).cpu().numpy()
        for metric, values in metric_data.items():
            for i, v in enumerate(values):
                if isinstance(v, _ChanHist):
                    row = host[rows[id(v)]]
                    if metric == HIST_METRIC:
                        values[i] = row[:, :HIST_BINS].astype(np.int64)
                    else:
                        values[i] = row[:, HIST_BINS if metric == NEARZERO_METRIC else HIST_BINS + 1].astype(np.float32)

    def _chancov_to_host(self, metric_data: Dict[str, list]):
        """a layer's running covariance sum -> per CHANCOV metric the ONE host value step() stores, in place: the average over
        the buffered forwards (device-served: over the ranks as well, like the mean |A| vectors), ONE transfer, then
        correlation_summary() in float64.  Covariance float64 [C, C], correlation fp32 [C, C], max |rho| fp32 [C], rank float"""
        acc = next((v for values in metric_data.values() for v in values if isinstance(v, _CovSum)), None)
        if acc is None:
            return
        cov = acc.sum / acc.n
        world = self._world() if acc.device_served else 1
        if world > 1:
            self._same_forward_count(acc.n, cov.device)
            torch.distributed.all_reduce(cov)
            cov = cov / world
        host = cov.cpu().numpy()
        summary = correlation_summary(host, self.redundancy_threshold)
        for metric, values in metric_data.items():
            if values and isinstance(values[0], _CovSum):
                values[0] = {COV_METRIC: host, CORR_METRIC: summary["correlation"].astype(np.float32),
                             MAXCORR_METRIC: summary["max_abs"].astype(np.float32),
                             RANK_METRIC: float(summary["effective_rank"])}[metric]

    def _changroup_to_host(self, metric_data: Dict[str, list]):
        """a layer's running per-sample sums -> per CHANGROUP metric the ONE host value step() stores, in place: fp32 [C] ([G]
        for the dominance).  Forwards are already added; ranks are added here (sums and sample counts: exact whatever the ranks'
        batch sizes).  ONE transfer: a float64 vector of 5 C + G + 1 numbers"""
        acc = next((v for values in metric_data.values() for v in values if isinstance(v, _GroupSum)), None)
        if acc is None:
            return
        Cc = acc.chan.shape[1]
        flat = torch.cat([acc.chan.reshape(-1), acc.grp.reshape(-1),
                          torch.tensor([float(acc.samples)], dtype=torch.float64, device=acc.chan.device)])
        if self._world() > 1:
            self._same_forward_count(acc.forwards, flat.device)
            torch.distributed.all_reduce(flat)
        host = flat.cpu().numpy()
        summary = changroup_summary(host[:5 * Cc].reshape(5, Cc), host[5 * Cc:-1], host[-1])
        for metric, values in metric_data.items():
            if values and isinstance(values[0], _GroupSum):
                values[0] = summary[metric]

    def _changrad_to_host(self, metric_data: Dict[str, list]):
        """the buffered (sums, absmax) pairs of a layer -> per backward pass the host vectors of each metric, in place: fp32 [C]
        each.  Across ranks the sums are averaged like the mean |A| vectors and the maxima maxed on their bit patterns.  ONE
        transfer: a float64 [passes, 4, C] tensor (fp32 maxima are exact in it)"""
        rows: Dict[int, int] = {}  # id of a buffered pair -> its row
        stack = []
        for values in metric_data.values():
            for v in values:
                if isinstance(v, _ChanGrad) and id(v) not in rows:
                    rows[id(v)] = len(stack)
                    stack.append(v.t)
        if not stack:
            return
        sums = torch.stack([t[0] for t in stack])
        amax = torch.stack([t[1] for t in stack]).contiguous()
        world = self._world()
        if world > 1:
            self._same_forward_count(sums.shape[0], sums.device)
            torch.distributed.all_reduce(sums)
            sums = sums / world
            # as integers the bit patterns of |g| order like the values, a NaN above every number: it survives the maximum
            torch.distributed.all_reduce(amax.view(torch.int32), op=torch.distributed.ReduceOp.MAX)
        host = torch.cat([sums, amax.double()[:, None, :]], dim=1).cpu().numpy()
        col = {MEANGRAD_METRIC: 0, GAINGRAD_METRIC: 1, SALIENCY_METRIC: 2, ABSMAXGRAD_METRIC: 3}
        for metric, values in metric_data.items():
            for i, v in enumerate(values):
                if isinstance(v, _ChanGrad):
                    values[i] = host[rows[id(v)], col[metric]].astype(np.float32)

    def _to_host(self, values: list) -> list:
        """device vectors of the fused path -> list of np.float32 arrays with ONE transfer."""
        if values and all(isinstance(v, torch.Tensor) and v.is_cuda for v in values):
            host = self._rank_average(torch.stack(values)).cpu().numpy()
            return [host[i] for i in range(host.shape[0])]
        return values

    def _device_to_host(self, metric_data: Dict[str, list]):
        """a device-served layer's buffer -> the host values the hook path would have buffered, in place: ONE transfer of
        the stacked moments vectors (mean |A| part averaged across ranks like the fused vectors, mean / std rank-local
        like the hook path's), one of the full-map snapshot (NCHW view with the channels_last strides of the hook's clone)"""
        moms: Dict[int, int] = {}  # id of a buffered moments vector -> its row
        stack = []
        for values in metric_data.values():
            for v in values:
                if isinstance(v, _Moments) and id(v.t) not in moms:
                    moms[id(v.t)] = len(stack)
                    stack.append(v.t)
        host = None
        if stack:
            stacked = torch.stack(stack)
            if FUSED_METRIC in metric_data:
                part = stacked[:, :-2].contiguous()
                avg = self._rank_average(part)
                if avg is not part:
                    stacked = torch.cat([avg, stacked[:, -2:]], dim=1)
            host = stacked.cpu().numpy()
        for metric, values in metric_data.items():
            for i, v in enumerate(values):
                if isinstance(v, _Moments):
                    row = host[moms[id(v.t)]]
                    if metric == FUSED_METRIC:
                        values[i] = row[:-2]
                    else:
                        values[i] = np.asarray(row[-2] if metric == "mean_activation" else row[-1], dtype=np.float32)
                elif isinstance(v, torch.Tensor) and v.is_cuda:
                    values[i] = v.cpu().permute(0, 3, 1, 2)

    def step(self, global_step: int) -> Dict[str, Any]:
        if not self.config.get("enabled", False):
            return {}
        if global_step % self.config.get("track_interval", 100) != 0:
            return {}
        log: Dict[str, Any] = {}
        processed: Dict[str, Dict[str, Any]] = {}
        for metric_data in self.hook_collected_buffer.values():
            if any(isinstance(v, _Moments) or (m == "full_activation_map" and isinstance(v, torch.Tensor) and v.is_cuda)
                   for m, values in metric_data.items() for v in values):
                self._device_to_host(metric_data)
            self._chanhist_to_host(metric_data)
            self._chancov_to_host(metric_data)
            self._changroup_to_host(metric_data)
            self._changrad_to_host(metric_data)
        for layer_id, metric_data in self.hook_collected_buffer.items():
            processed[layer_id] = {}
            for metric, values in metric_data.items():
                if not values:
                    continue
                agg = None
                key = f"tracking/{layer_id}/{metric}"
                try:
                    if metric == "full_activation_map":
                        agg = values[0]
                        arr = agg.numpy() if isinstance(agg, torch.Tensor) else agg
                        if isinstance(arr, np.ndarray):
                            log[key + "_mean"] = np.mean(arr.astype(np.float32))
                            log[key + "_std"] = np.std(arr.astype(np.float32))
                    elif metric in CHANCOV_METRICS:  # one value, of the covariance averaged over the buffered forwards
                        agg = values[0]
                        if metric == CORR_METRIC:
                            log[key + "_mean_abs_offdiag"] = correlation_summary(agg)["cov_mean_abs_offdiag"]
                        elif metric == MAXCORR_METRIC:
                            log[key + "_overall_max"] = np.max(agg)
                        elif metric == RANK_METRIC:
                            log[key] = agg
                    elif metric in CHANGROUP_METRICS:  # one value, of the sums over every sample since the last step()
                        agg = values[0]
                        if metric == SHARE_METRIC:
                            G = self._groups.get(layer_id, (None,))[0] or 1  # uniform share 1 / cg = G / C
                            log[key + "_squashed_channels"] = int(np.sum(agg < SQUASHED_SHARE * G / max(len(agg), 1)))
                            log[key + "_overall_max"] = np.max(agg)
                        elif metric == DOMINANCE_METRIC:
                            log[key + "_overall_max"] = np.max(agg)
                            log[key + "_most_dominated_group"] = int(np.argmax(agg))
                        elif metric == NRMS_METRIC:
                            log[key + "_overall_min"] = np.min(agg)
                        elif metric == ACTIVE_METRIC:
                            log[key + "_overall_min"] = np.min(agg)
                        else:
                            log[key + "_overall_max"] = np.max(agg)
                    elif metric == HIST_METRIC:  # summed over the buffered forwards
                        agg = np.sum(np.stack([np.asarray(v, dtype=np.int64) for v in values]), axis=0)
                        log[key + "_top_bin_share"] = float(agg[..., -1].sum()) / max(float(agg.sum()), 1.0)
                    elif metric == ABSMAX_METRIC:  # the maximum over them (a NaN stays)
                        agg = np.max(np.stack(values), axis=0)
                        log[key + "_overall_max"] = np.max(agg)
                    elif metric == NEARZERO_METRIC:  # the unweighted mean, like every other metric
                        agg = np.mean(np.stack(values), axis=0)
                        log[key + "_overall_mean"] = np.mean(agg)
                        log[key + "_overall_max"] = np.max(agg)
                    elif metric == ABSMAXGRAD_METRIC:  # the maximum over the buffered backward passes (a NaN stays)
                        agg = np.max(np.stack(values), axis=0)
                        log[key + "_overall_max"] = np.max(agg)
                    elif metric in CHANGRAD_METRICS:  # the unweighted mean over them
                        agg = np.mean(np.stack(values), axis=0)
                        log[key + "_overall_mean"] = np.mean(agg)
                        if metric != GAINGRAD_METRIC:
                            log[key + "_overall_max"] = np.max(agg)
                    elif FUSED_METRIC in metric:
                        vals = self._to_host(values)
                        if all(isinstance(v, np.ndarray) for v in vals):
                            agg = np.mean(np.stack(vals), axis=0)
                            log[key + "_overall_mean"] = np.mean(agg)
                            log[key + "_overall_std"] = np.std(agg)
                        else:
                            agg = vals[0]
                            if isinstance(agg, np.ndarray):
                                log[key + "_overall_mean"] = np.mean(agg)
                                log[key + "_overall_std"] = np.std(agg)
                            elif agg is not None:
                                log[key + "_overall_mean"] = float(agg)
                    else:
                        agg = np.mean([v.item() if hasattr(v, "item") else float(v) for v in values])
                        log[key] = agg
                except Exception as e:
                    logger.error(f"Error aggregating metric {metric} for {layer_id} in step(): {e}", exc_info=True)
                    agg = values[0]
                if agg is not None:
                    processed[layer_id][metric] = agg
        if processed:
            self.processed_data_by_step[global_step] = processed
            logger.info(f"ActivityMonitor collected and processed data for step {global_step}.")
        self.hook_collected_buffer.clear()
        return log

    def get_data_for_step(self, global_step: int) -> Dict[str, Any]:
        return self.processed_data_by_step.get(global_step, {})

    def export_all_processed_data_to_records(self) -> List[Dict[str, Any]]:
        recs: List[Dict[str, Any]] = []
        for gs, step_data in self.processed_data_by_step.items():
            for layer_id, metrics in step_data.items():
                for metric, value in metrics.items():
                    base = {"global_step": gs, "layer_identifier": layer_id, "original_metric_name": metric}

                    def add(kind, val):
                        recs.append({**base, "metric_type": kind, "metric_value": val})

                    if isinstance(value, torch.Tensor):
                        arr = value.numpy()
                    elif isinstance(value, np.ndarray):
                        arr = value
                    else:
                        add("scalar", float(value))
                        continue
                    if arr.ndim == 0:
                        add("scalar", float(arr.item()))
                    elif metric == "full_activation_map":
                        a32 = arr.astype(np.float32)
                        add("full_map_shape", str(arr.shape))
                        add("full_map_mean", float(np.mean(a32)))
                        add("full_map_std", float(np.std(a32)))
                        add("full_map_min", float(np.min(a32)))
                        add("full_map_max", float(np.max(a32)))
                    elif metric in (COV_METRIC, CORR_METRIC):
                        # (a correlation matrix is its own covariance: the cov_* figures of its summary are its own)
                        summ = correlation_summary(arr, self.redundancy_threshold)
                        kind = "covariance" if metric == COV_METRIC else "correlation"
                        add(kind + "_shape", str(arr.shape))
                        add(kind + "_mean_abs_offdiag", summ["cov_mean_abs_offdiag"])
                        add(kind + "_max_abs_offdiag", summ["cov_max_abs_offdiag"])
                        add(kind + "_redundant_pairs", summ["redundant_pairs"])  # pairs c < c' with |rho| above the threshold
                    elif metric == MAXCORR_METRIC:
                        add("max_abs_correlation_overall_mean", float(np.mean(arr)))
                        add("max_abs_correlation_overall_max", float(np.max(arr)))
                        add("max_abs_correlation_redundant_channels", int(np.sum(arr > self.redundancy_threshold)))
                    elif metric in CHANGROUP_METRICS:
                        kind = metric[:-len("_per_channel")] if metric != DOMINANCE_METRIC else "group_dominance"
                        add(kind + "_overall_mean", float(np.mean(arr)))
                        add(kind + "_overall_min", float(np.min(arr)))
                        add(kind + "_overall_max", float(np.max(arr)))
                        if metric == SHARE_METRIC:  # channels below a tenth of the uniform share 1 / cg: squashed by a neighbour
                            G = self._groups.get(layer_id, (None,))[0] or 1
                            add(kind + "_squashed_channels", int(np.sum(arr < SQUASHED_SHARE * G / max(len(arr), 1))))
                        elif metric == DOMINANCE_METRIC:
                            add(kind + "_argmax_group", int(np.argmax(arr)))
                        elif metric == ACTIVE_METRIC:  # channels no sample activates
                            add(kind + "_silent_channels", int(np.sum(arr == 0.0)))
                    elif metric == HIST_METRIC:
                        total = arr.reshape(-1, arr.shape[-1]).sum(axis=0)  # the tensor's histogram: all channels together
                        rows = arr.reshape(-1, arr.shape[-1]).sum(axis=1)
                        add("histogram_shape", str(arr.shape))
                        # forwards x B*H*W: every channel's row sums to it (-1 if the rows disagree, which no path produces)
                        add("histogram_row_total", int(rows[0]) if (rows == rows[0]).all() else -1)
                        add("histogram_top_bin_count", int(total[-1]))
                        add("histogram_zero_bin_count", int(total[0]))
                        # the bin that holds the tensor's median magnitude (the lower median)
                        add("histogram_median_bin", int(np.searchsorted(np.cumsum(total), (int(total.sum()) + 1) // 2)))
                    elif metric == ABSMAX_METRIC:
                        add("abs_max_overall_max", float(np.max(arr)))
                        add("abs_max_overall_mean", float(np.mean(arr)))
                        add("abs_max_argmax_channel", int(np.argmax(arr)))
                    elif metric in CHANGRAD_METRICS:
                        kind = metric[:-len("_per_channel")]
                        add(kind + "_overall_mean", float(np.mean(arr)))
                        add(kind + "_overall_min", float(np.min(arr)))
                        add(kind + "_overall_max", float(np.max(arr)))
                        if metric == SALIENCY_METRIC:
                            add(kind + "_argmax_channel", int(np.argmax(arr)))
                        elif metric == MEANGRAD_METRIC:  # channels that received (next to) no gradient
                            add(kind + "_zero_channels", int(np.sum(arr <= self.zero_gradient_threshold)))
                    elif metric == NEARZERO_METRIC:
                        add("near_zero_overall_mean", float(np.mean(arr)))
                        add("near_zero_overall_max", float(np.max(arr)))
                        add("near_zero_dead_channels", int(np.sum(arr >= DEAD_FRACTION)))
                    elif FUSED_METRIC in metric:
                        add("per_channel_overall_mean", float(np.mean(arr)))
                        add("per_channel_overall_std", float(np.std(arr)))
                        add("per_channel_overall_min", float(np.min(arr)))
                        add("per_channel_overall_max", float(np.max(arr)))
                    else:
                        a32 = arr.astype(np.float32)
                        add("array_mean", float(np.mean(a32)))
                        add("array_std", float(np.std(a32)))
        return recs

    def __del__(self):
        try:
            self.remove_hooks()
        except Exception:
            pass
