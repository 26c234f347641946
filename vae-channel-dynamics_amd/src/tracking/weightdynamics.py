"""WeightDynamicsTracker: per-channel norms, gradients and updates of the WEIGHTS that write and read a channel (YAML section
`weight_dynamics:`), the weight-side twin of ActivityMonitor's per-channel activation metrics.

For a parameter stored as [O][K][I] (OHWI conv weight: K = kh kw; linear [out][in]: K = 1; vector: K = I = 1) the `out` view has
one slice per output channel o (all k, i: the filter that writes the channel, or one element of a GroupNorm gamma) and the `in`
view one slice per input channel i (all o, k: what the layer reads of the channel; only when I > 1).  Per slice, six raw sums
and a maximum over its elements:
    S_ww = sum w^2, S_gg = sum g^2, S_wg = sum w g, S_mm = sum m^2, S_gm = sum g m, S_uu = sum u^2, A = max |w|
with g the gradient, m / v the Adam moments and u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps) the Adam direction, so that
lr * u is the Adam part of the update just applied.  The metrics, on the host in float64 (derive()):
    weight_norm_per_channel           sqrt(S_ww)
    weight_abs_max_per_channel        A
    grad_norm_per_channel             sqrt(S_gg)
    scale_gradient_per_channel        S_wg: dL/ds of a gain s on the slice at s = 1 (the twin of gain_gradient_per_channel)
    update_ratio_per_channel          last_lr * sqrt(S_uu) / max(sqrt(S_ww), 1e-30)
    grad_momentum_cosine_per_channel  S_gm / sqrt(S_gg * S_mm), 0 where a factor is 0
A parameter with requires_grad == False reports the two weight metrics and NaN for the other four; before the first optimizer
step the update ratio and the cosine are NaN.

With the parameters in the HIP arena on a GPU, track() is ONE ops.weight_dynamics pass over the four flat arenas (parameters,
gradients, both moments of FusedAdamW) and one read-back of the result vectors; any other model (plain torch parameters, CPU)
gets the same definitions as float64 torch formulas (raw_sums_torch).  Nothing is exchanged between ranks: after the gradient
all-reduce every rank holds the same arenas, so train.py calls track() on the main rank only.
"""
from __future__ import annotations

import json
import logging
from collections import defaultdict
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

logger = logging.getLogger(__name__)

METRICS = ("weight_norm_per_channel", "weight_abs_max_per_channel", "grad_norm_per_channel", "scale_gradient_per_channel",
           "update_ratio_per_channel", "grad_momentum_cosine_per_channel")
WEIGHT_METRICS = METRICS[:2]  # what a frozen parameter still reports
VIEWS = ("out", "in")
DEFAULT_CLASSES = (nn.Conv2d, nn.Linear, nn.GroupNorm)
S_WW, S_GG, S_WG, S_MM, S_GM, S_UU = range(6)


def adam_constants(beta1: float, beta2: float, eps: float, step: int) -> Tuple[float, float, float]:
    """(bc1, bc2_sqrt, eps) rounded to float once, as the fused optimizer and csrc/wdyn.hip hold them"""
    return (float(np.float32(1.0 - beta1 ** step)), float(np.float32(np.sqrt(1.0 - beta2 ** step))), float(np.float32(eps)))


def as_okI(t: torch.Tensor) -> torch.Tensor:
    """a parameter-shaped tensor as [O][K][I]: the arena's memory order of a conv weight, whatever its strides"""
    if t.dim() == 4:
        return t.permute(0, 2, 3, 1).reshape(t.shape[0], t.shape[2] * t.shape[3], t.shape[1])
    if t.dim() == 2:
        return t.reshape(t.shape[0], 1, t.shape[1])
    if t.dim() == 1:
        return t.reshape(-1, 1, 1)
    raise ValueError(f"weight dynamics: a parameter of shape {tuple(t.shape)} is no conv weight, linear weight or vector")


def raw_sums_torch(w: torch.Tensor, g: Optional[torch.Tensor], m: Optional[torch.Tensor], v: Optional[torch.Tensor],
                   consts: Optional[Tuple[float, float, float]]):
    """what ops.weight_dynamics computes for one parameter, as float64 torch formulas on the tensors' device:
    {view: (sums float64 [n, 6], absmax fp32 [n])}; the sums a missing operand cannot form are NaN.  No `in` view when I == 1."""
    w3 = as_okI(w.detach())
    d = lambda t: None if t is None else as_okI(t.detach()).double()  # noqa: E731
    wd, gd, md, vd = d(w), d(g), d(m), d(v)
    terms: List[Optional[torch.Tensor]] = [wd * wd, None, None, None, None, None]
    if gd is not None:
        terms[S_GG], terms[S_WG] = gd * gd, wd * gd
    if gd is not None and md is not None and vd is not None:
        bc1, bc2_sqrt, eps = consts
        u = (md / bc1) / (vd.sqrt() / bc2_sqrt + eps)
        terms[S_MM], terms[S_GM], terms[S_UU] = md * md, gd * md, u * u
    out = {}
    for view, dims in (("out", (1, 2)), ("in", (0, 1))):
        if view == "in" and w3.shape[2] == 1:
            continue
        n = w3.shape[0] if view == "out" else w3.shape[2]
        cols = [t.sum(dim=dims) if t is not None else torch.full((n,), float("nan"), dtype=torch.float64, device=w3.device)
                for t in terms]
        out[view] = (torch.stack(cols, dim=1), w3.abs().amax(dim=dims).float())  # amax hands a NaN on
    return out


def derive(sums: np.ndarray, absmax: np.ndarray, last_lr: Optional[float]) -> Dict[str, np.ndarray]:
    """the six metrics of a view from its raw sums [n, 6] and max |w| [n], float64; NaN sums give NaN metrics"""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        wn = np.sqrt(s[:, S_WW])
        gn = np.sqrt(s[:, S_GG])
        den = np.sqrt(s[:, S_GG] * s[:, S_MM])
        cos = np.where(den > 0, s[:, S_GM] / np.where(den > 0, den, 1.0), np.where(np.isnan(den), np.nan, 0.0))
        ratio = (float("nan") if last_lr is None else float(last_lr)) * np.sqrt(s[:, S_UU]) / np.maximum(wn, 1e-30)
    return {"weight_norm_per_channel": wn, "weight_abs_max_per_channel": np.asarray(absmax, dtype=np.float64),
            "grad_norm_per_channel": gn, "scale_gradient_per_channel": s[:, S_WG].copy(),
            "update_ratio_per_channel": ratio, "grad_momentum_cosine_per_channel": cos}


def _subset(name: str, given, allowed: Sequence[str]) -> Tuple[str, ...]:
    if given is None:
        return tuple(allowed)
    given = [given] if isinstance(given, str) else list(given)
    bad = [x for x in given if x not in allowed]
    if bad:
        raise ValueError(f"weight_dynamics.{name}: unknown {bad}; choose from {list(allowed)}")
    if not given:
        raise ValueError(f"weight_dynamics.{name}: empty; choose from {list(allowed)}")
    return tuple(x for x in allowed if x in given)


class WeightDynamicsTracker:
    def __init__(self, config: Optional[Dict[str, Any]] = None):
        cfg = dict(config or {})
        known = {"enabled", "track_interval", "target_parameters", "views", "metrics"}
        unknown = sorted(set(cfg) - known)
        if unknown:
            raise ValueError(f"weight_dynamics: unknown keys {unknown}; the section knows {sorted(known)}")
        self.enabled = bool(cfg.get("enabled", False))
        self.track_interval = int(cfg.get("track_interval", 100))
        if self.track_interval < 1:
            raise ValueError(f"weight_dynamics.track_interval must be at least 1, got {self.track_interval}")
        tp = cfg.get("target_parameters")
        self.target_parameters: Optional[List[str]] = None if tp is None else [str(t) for t in ([tp] if isinstance(tp, str) else tp)]
        self.views = _subset("views", cfg.get("views"), VIEWS)
        self.metrics = _subset("metrics", cfg.get("metrics"), METRICS)
        # (parameter, view, metric) -> [(global_step, float64 vector)]
        self.history: Dict[Tuple[str, str, str], List[Tuple[int, np.ndarray]]] = defaultdict(list)
        self._table = None  # (key, WeightTable)
        self.last_raw: Dict[str, Dict[str, Tuple[np.ndarray, np.ndarray]]] = {}
        self.last_lr: Optional[float] = None

    # ------------------------------------------------------------------ selection
    def targets(self, model: nn.Module) -> List[Tuple[str, nn.Parameter]]:
        """[(name, parameter)] in the model's order.  Default: every weight / bias of Conv2d, Linear and GroupNorm; else the
        parameters whose name equals an entry of target_parameters or starts with `entry.` (a leading `vae.` is the wrapper's)."""
        named = list(model.named_parameters())
        if self.target_parameters is None:
            out = []
            for name, p in named:
                mod_name, _, leaf = name.rpartition(".")
                if leaf in ("weight", "bias") and isinstance(model.get_submodule(mod_name), DEFAULT_CLASSES) and p.dim() in (1, 2, 4):
                    out.append((name, p))
            return out
        chosen: List[Tuple[str, nn.Parameter]] = []
        for pre in self.target_parameters:
            hit = []
            for cand in (pre, pre[4:] if pre.startswith("vae.") else pre):
                hit = hit or [(n, p) for n, p in named if n == cand or n.startswith(cand + ".")]
            if not hit:
                raise ValueError(f"weight_dynamics.target_parameters: {pre!r} matches no parameter of the model")
            chosen += [h for h in hit if all(h[0] != c[0] for c in chosen)]
        order = {n: i for i, (n, _) in enumerate(named)}
        return sorted(chosen, key=lambda np_: order[np_[0]])

    # ------------------------------------------------------------------ the pass
    @torch.no_grad()
    def track(self, model_or_wrapper, optimizer, global_step: int) -> Dict[str, float]:
        """record every target's vectors at `global_step`; returns {`weight_dynamics/<parameter>/<view>/<metric>_max`: value}"""
        model = getattr(model_or_wrapper, "vae", None)
        model = model_or_wrapper if model is None else model
        if not isinstance(model, nn.Module):
            raise TypeError("WeightDynamicsTracker.track: expected an nn.Module or a wrapper with .vae")
        items = self.targets(model)
        if not items:
            return {}
        arena = getattr(model, "arena", None)
        if arena is not None and arena.flat.is_cuda and all(id(p) in arena.offset_of for _, p in items):
            raw, last_lr = self._raw_arena(arena, items, optimizer)
        else:
            raw, last_lr = self._raw_torch(items, optimizer)
        self.last_raw, self.last_lr = raw, last_lr  # of this call: {parameter: {view: (sums [n, 6], max |w| [n])}}
        logs: Dict[str, float] = {}
        for name, p in items:
            for view in self.views:
                if view not in raw[name]:
                    continue
                vals = derive(*raw[name][view], last_lr)
                for metric in self.metrics:
                    vec = vals[metric]
                    if not p.requires_grad and metric not in WEIGHT_METRICS:
                        vec = np.full_like(vec, np.nan)  # its gradient slot may hold anything
                    self.history[(name, view, metric)].append((int(global_step), vec))
                    logs[f"weight_dynamics/{name}/{view}/{metric}_max"] = _nan_stat(np.nanmax, vec)
        return logs

    @staticmethod
    def _adam_state(optimizer):
        """(beta1, beta2, eps, step, last_lr) of an optimizer that has taken a step, else None"""
        if optimizer is None or not getattr(optimizer, "param_groups", None):
            return None
        g = optimizer.param_groups[0]
        if "betas" not in g:
            return None
        step = getattr(optimizer, "step_count", None)
        if step is None:  # torch.optim.Adam / AdamW keep it per parameter
            steps = [int(st["step"]) for st in optimizer.state.values() if "step" in st]
            step = max(steps) if steps else 0
        if int(step) < 1:
            return None
        last_lr = getattr(optimizer, "last_lr", None)
        return float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), int(step), float(g["lr"] if last_lr is None else last_lr)

    def _raw_arena(self, arena, items, optimizer):
        from vaehip import ops
        from vaehip.weight_table import WeightTable
        key = (id(arena), arena.flat.data_ptr(), tuple(n for n, _ in items))
        if self._table is None or self._table[0] != key:
            self._table = (key, WeightTable(arena, items))
        table = self._table[1]
        st = self._adam_state(optimizer)
        m = getattr(optimizer, "exp_avg", None) if st else None
        v = getattr(optimizer, "exp_avg_sq", None) if st else None
        if m is None or v is None or m.numel() != arena.flat.numel():
            st, m, v = None, None, None
        b1, b2, eps, step, last_lr = st if st else (0.9, 0.999, 1e-8, 1, None)
        res = ops.weight_dynamics(arena.flat, arena.grad, m, v, table, b1, b2, eps, step)
        # one read-back: the four vectors as one float64 buffer (max |w| is exact in float64)
        host = torch.cat([res[0].reshape(-1), res[1].reshape(-1), res[2].double(), res[3].double()]).cpu().numpy()
        n_o, n_i = table.n_out, table.n_in
        out_sums, in_sums = host[:6 * n_o].reshape(n_o, 6), host[6 * n_o:6 * (n_o + n_i)].reshape(n_i, 6)
        out_amax, in_amax = host[6 * (n_o + n_i):6 * (n_o + n_i) + n_o], host[6 * (n_o + n_i) + n_o:]
        raw = {}
        for s in table.slots:
            raw[s.name] = {"out": (out_sums[table.out_slice(s)], out_amax[table.out_slice(s)])}
            if s.I > 1:
                raw[s.name]["in"] = (in_sums[table.in_slice(s)], in_amax[table.in_slice(s)])
        return raw, last_lr

    def _raw_torch(self, items, optimizer):
        st = self._adam_state(optimizer)
        consts = adam_constants(*st[:4]) if st else None
        raw = {}
        for name, p in items:
            g = p.grad if p.requires_grad else None
            m = v = None
            if st and g is not None:
                state = optimizer.state.get(p, {}) if hasattr(optimizer, "state") else {}
                m, v = state.get("exp_avg"), state.get("exp_avg_sq")
            res = raw_sums_torch(p, g, m, v, consts)
            raw[name] = {view: (s.cpu().numpy(), a.cpu().numpy()) for view, (s, a) in res.items()}
        return raw, (st[4] if st else None)

    # ------------------------------------------------------------------ export
    def export_records(self) -> List[Dict[str, Any]]:
        """one record per (step, parameter, view, metric): the vector as a JSON list in metric_value, beside its length and
        its min / median / max over the channels (NaN entries skipped; NaN when all are)"""
        recs = []
        for (name, view, metric), hist in self.history.items():
            for step, vec in hist:
                recs.append({"global_step": step, "parameter": name, "view": view, "metric": metric,
                             "metric_type": metric[:-len("_per_channel")] + "_vector", "num_channels": int(vec.shape[0]),
                             "min": _nan_stat(np.nanmin, vec), "median": _nan_stat(np.nanmedian, vec), "max": _nan_stat(np.nanmax, vec),
                             "metric_value": json.dumps([float(x) for x in vec])})
        recs.sort(key=lambda r: r["global_step"])
        return recs


CSV_FIELDS = ("global_step", "parameter", "view", "metric", "metric_type", "num_channels", "min", "median", "max", "metric_value")


def _nan_stat(fn, vec: np.ndarray) -> float:
    return float("nan") if vec.size == 0 or np.isnan(vec).all() else float(fn(vec))
