"""Train / validate / evaluate loop with the reference's API, one process per GPU.

Reference: /root/reference/src/engine.py -- `Engine.run_epoch(data, gpu_id, epoch, mode)` (:40),
`Trainer(model, loss_delta, out_dir).fit((train, val), gpu_id)` (:104-133), `.save/.load(ckpt)`
(:135-157), `Evaluator(model, delta, out_dir, ckpt).eval(loader, gpu_id)` (:160-168);
src/loss.py:51-52 (Huber), :55-95 (Gauss), src/metrics.py:20-35 (MAE / MAPE / RMSE).

Differences that are the point of this build:
  * fp32 end to end (the reference wraps the forward in CUDA AMP, engine.py:54; the parity bar of
    the hot path is fp32).  No loss scaling is needed, but checkpoints carry the state dict of a
    default `GradScaler` under the reference's key so that either side loads the other's files.
  * the step tail runs in the library: ONE pass over the prediction gives the
    Huber loss and the metric sums (`ops.huber_metrics`), which stay on the device -- the host reads them
    once per epoch instead of four `.item()` syncs per batch (engine.py:66, metrics.py:24,30,34) -- and
    Adam updates every parameter in one launch over flat state buffers (`FlatAdam`).
  * under `torch.distributed` every rank runs its batch shard and the gradients are averaged with ONE
    flat all-reduce of the buffer Adam reads (`nn.DataParallel`, main.py:52-55, is not used).
  * `null_value` (off by default) treats entries of the truth that are NaN or equal to it as missing readings: they
    drop out of the loss, its gradient and the metrics, which are then kept per forecast horizon
    (`ops.masked_huber_metrics`; the batch's valid count stays on the device, also as the rank's weight).
  * `loss=GaussLoss(sigma, delta)` (off by default: Huber) trains and evaluates with the reference's other loss, in the same
    library tail -- one pass with metrics, masked or not, the valid count on the device, captured steps.
  * `loss=QuantileLoss(quantiles)` trains a quantile forecast -- a head of `Q * T_out` outputs against `T_out`-step truths --
    with the pinball loss in the same tail (`ops.quantile_metrics`): the point metrics from the level nearest 0.5, and per
    horizon what makes such a forecast checkable, coverage per level, interval width, crossing rate (`last_stats["quantiles"]`).
  * `max_grad_norm` / `skip_nonfinite` (both off by default) put a guard on the optimizer step: the global gradient norm is
    taken on the device, the gradient is clipped to `max_grad_norm` as `torch.nn.utils.clip_grad_norm_` would, and a step
    whose norm is Inf or NaN is left out whole, as the reference's `GradScaler.step` leaves it out (engine.py:61-63) --
    inside a captured step and after the one all-reduce of a multi-rank step, with nothing read back (`FlatAdam`).
  * `ema_decay` (off by default) keeps an exponential moving average of the parameters inside the same update launch
    (`msgat_adam_step_averaged`): one more flat buffer, warmed up by each tensor's own step count, untouched by a step the
    guard leaves out, bit-identical across ranks.  `fit` validates -- and so picks its best checkpoint -- on the averaged
    weights, exchanged with the parameters in place by one launch (`msgat_param_swap`), so captured validation graphs read
    them at the addresses they hold; checkpoints gain an `ema` key and `Evaluator(weights=...)` chooses which set to load.
  * `accumulate_steps=k` (1, off, by default) takes one optimizer step per window of k batches: every micro-batch is added
    into the flat gradient buffer with the weight a rank would have (`msgat_gather_accumulate`), the last one's step
    divides by the summed weight -- one step on the union of the window, one collective per window under a process group.
  * `hip_graph="auto"` (the default on the GPU) captures a step in a HIP graph once its batch shape recurs and replays it.
CPU tensors (the host-logic tests run a small CPU `nn.Module` through this loop) take plain PyTorch
ops for loss and optimizer; the library has no CPU path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from pathlib import Path
from time import localtime, strftime
from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist
from torch import nn, optim
from torch.optim import lr_scheduler

from . import parallel


def huber_loss(output: torch.Tensor, target: torch.Tensor, delta: float = 1.0) -> torch.Tensor:
    """Mean Huber loss (loss.py:51-52): quadratic within `delta`, linear beyond."""
    err = (output - target).abs()
    return torch.where(err <= delta, 0.5 * err * err, delta * err - 0.5 * delta * delta).mean()


def valid_entries(target: torch.Tensor, null_value: float) -> torch.Tensor:
    """The entries of the truth that are measurements: not NaN and not `null_value` (PEMS files store 0 for a sensor
    that was down).  `null_value = nan` masks the NaN entries only."""
    return ~torch.isnan(target) & (target != null_value)


def masked_huber_loss(output: torch.Tensor, target: torch.Tensor, delta: float, null_value: float) -> torch.Tensor:
    """Huber loss summed over the valid entries of `target` and divided by max(valid count, 1): 0 for a batch without a
    valid entry.  The torch restatement of `ops.masked_huber_metrics` (what CPU tensors run)."""
    valid = valid_entries(target, null_value)
    zero = torch.zeros((), dtype=output.dtype, device=output.device)
    err = torch.where(valid, output - target, zero).abs()
    huber = torch.where(err <= delta, 0.5 * err * err, delta * err - 0.5 * delta * delta)
    return torch.where(valid, huber, zero).sum() / valid.sum().clamp(min=1)


def gauss_entry(err: torch.Tensor, sigma: float, delta: float) -> torch.Tensor:
    """The Gauss loss of every entry at the absolute errors `err`: sigma^2 (1 - exp(-err^2 / 2 sigma^2)) + delta err,
    written as the reference writes it (loss.py:94-95).  In fp32 the VALUE carries the reference's cancellation for
    err << sigma (3.5e-3 relative at err = 1e-3 sigma, delta = 0; the library's kernels take -expm1f instead); its
    gradient err exp(-err^2 / 2 sigma^2) + delta does not, which torch.expm1's backward (out + 1) would lose in the tail."""
    return sigma ** 2 * (1 - torch.exp(-(err * err) / (2 * sigma ** 2))) + delta * err


def gauss_loss(output: torch.Tensor, target: torch.Tensor, sigma: float = 1.0, delta: float = 5e-2) -> torch.Tensor:
    """Mean Gauss loss (loss.py:94-95): sigma^2 mean(1 - exp(-e^2 / 2 sigma^2)) + delta mean |e|, a robust loss whose
    weight on an entry saturates where Huber's grows without bound."""
    return gauss_entry((output - target).abs(), sigma, delta).mean()


def masked_gauss_loss(output: torch.Tensor, target: torch.Tensor, sigma: float, delta: float,
                      null_value: float) -> torch.Tensor:
    """Gauss loss summed over the valid entries of `target` and divided by max(valid count, 1).  The torch restatement
    of `ops.masked_gauss_metrics` (what CPU tensors run)."""
    valid = valid_entries(target, null_value)
    zero = torch.zeros((), dtype=output.dtype, device=output.device)
    err = torch.where(valid, output - target, zero).abs()
    return torch.where(valid, gauss_entry(err, sigma, delta), zero).sum() / valid.sum().clamp(min=1)


def quantile_entries(output: torch.Tensor, target: torch.Tensor, levels, null_value: Optional[float]):
    """-> (p [..., Q, T_out], y [..., 1, T_out] with 0 at the entries that are not valid, valid [..., T_out],
    rho [..., Q, T_out]): the pinball loss max(tau_q u, (tau_q - 1) u), u = y - p_q, of every level at every valid entry
    and 0 elsewhere.  `output` is [..., Q * T_out], level-major (or [..., Q, T_out])."""
    from . import ops
    t_out = ops.quantile_widths(output, target, len(levels))
    p = output.reshape(*target.shape[:-1], len(levels), t_out)
    valid = valid_entries(target, float("nan") if null_value is None else null_value)
    zero = torch.zeros((), dtype=output.dtype, device=output.device)
    y = torch.where(valid, target.to(output.dtype), zero).unsqueeze(-2)
    tau = torch.tensor(levels, dtype=output.dtype, device=output.device).reshape(-1, 1)
    u = y - p
    rho = torch.where(valid.unsqueeze(-2), torch.maximum(tau * u, (tau - 1) * u), zero)
    return p, y, valid, rho


def quantile_loss(output: torch.Tensor, target: torch.Tensor, levels, null_value: Optional[float] = None) -> torch.Tensor:
    """Pinball loss averaged over the Q levels, summed over the valid entries of `target` and divided by max(valid count,
    1): 0 for a batch without a valid entry.  Its autograd is the rule the kernels state: -tau_q / 1 - tau_q either side
    of p_q and, `torch.maximum` splitting a tie evenly, 1/2 - tau_q at y == p_q.  The torch restatement of
    `ops.quantile_metrics` (what CPU tensors run)."""
    _, _, valid, rho = quantile_entries(output, target, levels, null_value)
    return rho.sum() / (len(levels) * valid.sum().clamp(min=1))


class HuberLoss(nn.Module):
    """Mean Huber loss.  `null_value` (default None: every entry counts, the reference's loss) drops the entries of the
    target that are NaN or equal to it from the sum AND from the divisor."""

    def __init__(self, delta: float = 1.0, null_value: Optional[float] = None):
        super().__init__()
        self.delta = delta
        self.null_value = null_value

    def forward(self, output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if output.is_cuda:
            return self.fused(output, target, 0.0, None)
        if self.null_value is not None:
            return masked_huber_loss(output, target, self.delta, self.null_value)
        return huber_loss(output, target, self.delta)

    def entry(self, err: torch.Tensor) -> torch.Tensor:
        """The loss of every entry at the absolute errors `err` (what `Metrics` sums on CPU tensors)."""
        return torch.where(err <= self.delta, 0.5 * err * err, self.delta * err - 0.5 * self.delta * self.delta)

    def fused(self, pred, truth, mask_value, sums, loss_weight=1.0, valid=None) -> torch.Tensor:
        """The library's one pass over device tensors: the loss, and `sums` fed (`valid`: the masked form's count)."""
        from . import ops
        if self.null_value is not None:
            return ops.masked_huber_metrics(pred, truth, self.delta, self.null_value, mask_value, sums, valid)
        return ops.huber_metrics(pred, truth, self.delta, mask_value, sums, loss_weight)


class GaussLoss(nn.Module):
    """Mean Gauss loss (loss.py:55-95), sigma^2 (1 - exp(-e^2 / 2 sigma^2)) + delta |e| per entry.  `null_value` as in
    `HuberLoss`.  On device tensors it is `ops.gauss_metrics` / `ops.masked_gauss_metrics`."""

    def __init__(self, sigma: float = 1.0, delta: float = 5e-2, null_value: Optional[float] = None):
        super().__init__()
        from . import ops
        ops.gauss_params(sigma, delta)      # ValueError for what the kernels refuse
        self.sigma, self.delta = sigma, delta
        self.null_value = null_value

    def forward(self, output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if output.is_cuda:
            return self.fused(output, target, 0.0, None)
        if self.null_value is not None:
            return masked_gauss_loss(output, target, self.sigma, self.delta, self.null_value)
        return gauss_loss(output, target, self.sigma, self.delta)

    def extra_repr(self) -> str:
        return f"sigma={self.sigma}, delta={self.delta}"

    def entry(self, err: torch.Tensor) -> torch.Tensor:
        return gauss_entry(err, self.sigma, self.delta)

    def fused(self, pred, truth, mask_value, sums, loss_weight=1.0, valid=None) -> torch.Tensor:
        from . import ops
        if self.null_value is not None:
            return ops.masked_gauss_metrics(pred, truth, self.sigma, self.delta, self.null_value, mask_value, sums, valid)
        return ops.gauss_metrics(pred, truth, self.sigma, self.delta, mask_value, sums, loss_weight)


class QuantileLoss(nn.Module):
    """Pinball loss of a quantile forecast: the model's `Q * T_out` outputs per node are, level-major, the `quantiles`
    of the next `T_out` steps (`out_timesteps = Q * T_out`), compared with ONE truth per step.  `levels` are the
    quantiles, `point` the index of the level nearest 0.5 (the lower one on a tie): the level whose forecast feeds MAE /
    MAPE / RMSE.  Entries of the target that are NaN or equal to `null_value` (None: NaN only) drop out, as in the masked
    forms of the other two losses -- there is no unmasked form.  On device tensors it is `ops.quantile_metrics`."""

    def __init__(self, quantiles=(0.1, 0.5, 0.9), null_value: Optional[float] = None):
        super().__init__()
        from . import ops
        self.levels = ops.quantile_levels(quantiles)      # ValueError for what the kernels refuse
        self.point = ops.quantile_point(self.levels)
        self.null_value = null_value

    def split(self, pred: torch.Tensor) -> torch.Tensor:
        """[B, N, Q * T_out] -> [B, N, Q, T_out] (a view where `pred` allows one)."""
        q = len(self.levels)
        if pred.dim() == 0 or pred.shape[-1] % q:
            raise ValueError(f"{tuple(pred.shape)}: the last axis must hold {q} levels times T_out steps")
        return pred.reshape(*pred.shape[:-1], q, pred.shape[-1] // q)

    def point_forecast(self, pred: torch.Tensor) -> torch.Tensor:
        """[B, N, Q * T_out] -> [B, N, T_out]: the forecast of level `point`."""
        return self.split(pred)[..., self.point, :]

    def forward(self, output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if output.is_cuda:
            return self.fused(output, target, 0.0, None)
        return quantile_loss(output, target, self.levels, self.null_value)

    def extra_repr(self) -> str:
        return f"quantiles={self.levels}"

    def fused(self, pred, truth, mask_value, sums, loss_weight=1.0, valid=None) -> torch.Tensor:
        """The library's one pass (`loss_weight` is not used: a rank's weight is its valid count, as in every masked form)."""
        from . import ops
        return ops.quantile_metrics(pred, truth, self.levels, self.null_value, mask_value, sums, valid, self.point)


class Metrics:
    """Running MAE / MAPE / RMSE with the reference's definitions (metrics.py:11-38): MAPE sums
    |err/y| over entries with y > mask_value but divides by ALL entries, like the reference.
    Totals [AE, APE, SE, sum of batch losses] accumulate on the device in float64; properties synchronise
    when read.  Under a process group a rank adds its share n_r / n_b of every global batch's loss
    (`loss_weight`), so the all-reduced total is the sum of the reference's per-batch mean losses
    (engine.py:66-67) -- also for uneven shards -- and `batches` counts GLOBAL batches (every rank sees them all).

    With `null_value` set, only the VALID entries of the truth count (not NaN, != null_value) and the totals are kept per
    forecast horizon: a float64 [T_out + 1, 5] buffer whose row t < T_out holds, for horizon step t + 1,
    {valid count, sum |e|, 100 sum_{y > mask_value} |e / y|, sum e^2, sum loss(e)} and whose last row holds the same
    over all horizons (the layout `ops.masked_huber_metrics` / `ops.masked_gauss_metrics` add to; `loss` is whichever
    loss ran).  It is allocated on first use, zeroed by `reset()` and reduced in place by `all_reduce()`.  MAE / MAPE / RMSE divide by the valid count read from the
    buffer, and `loss` is the epoch's total loss sum over its total valid count -- a ratio of totals, the same number
    for any number of ranks and any sharding of the batches, which a mean of per-batch means is not once the batches'
    valid counts differ.  `per_horizon()` / `at(steps)` give the metrics per horizon; a Metrics that was told its loss
    (`loss_fn`, here or in `update`) also gives a "loss" list there, column 4 over the valid count.

    With a `QuantileLoss` as `loss_fn` (given HERE: it sizes the buffer) the totals are always per horizon
    (`null_value=None` runs as NaN) and the buffer is [T_out + 1, 7 + 2Q], the layout `ops.quantile_metrics` adds to:
    columns 0-4 as above with e = p_point - y and the pinball loss averaged over the levels, 5 the number of entries whose
    levels cross (any p_q > p_{q+1}), 6 the sum of p_{Q-1} - p_0, 7 + q the number of entries with y <= p_q and
    7 + Q + q the sum of level q's pinball loss.  `per_horizon()` then also has "coverage" and "pinball" (Q lists of length
    T_out) and "crossing" and "width" (lists); `quantile_summary()` gives the same over all horizons."""

    def __init__(self, mask_value: float = 0.0, null_value: Optional[float] = None, loss_fn: Optional[nn.Module] = None):
        self.mask_value = mask_value
        if isinstance(loss_fn, QuantileLoss) and null_value is None:
            null_value = float("nan") if loss_fn.null_value is None else loss_fn.null_value
        self.null_value = null_value
        self.loss_fn = loss_fn
        self.n = 0
        self.batches = 0
        self._sums: Optional[torch.Tensor] = None

    def reset(self) -> None:
        """Start a new epoch on the SAME totals buffer (captured loss kernels hold its address)."""
        if self._sums is not None:
            self._sums.zero_()
        self.n = self.batches = 0

    def totals(self, device, t_out: Optional[int] = None) -> torch.Tensor:
        """The totals buffer; with `null_value` set the first call must name the number of horizons `t_out`."""
        if self.null_value is not None:
            if self._sums is None:
                if t_out is None:
                    raise ValueError("Metrics(null_value=...): the first totals() call needs t_out")
                self._sums = torch.zeros(int(t_out) + 1, self._columns(), device=device, dtype=torch.float64)
            elif t_out is not None and self._sums.shape[0] != int(t_out) + 1:
                raise ValueError(f"Metrics holds totals for {self._sums.shape[0] - 1} horizons, got a batch with {t_out}")
            return self._sums
        if self._sums is None:
            self._sums = torch.zeros(4, device=device, dtype=torch.float64)
        return self._sums

    def _quantile(self) -> Optional["QuantileLoss"]:
        return self.loss_fn if isinstance(self.loss_fn, QuantileLoss) else None

    def _columns(self) -> int:
        ql = self._quantile()
        return 5 if ql is None else 7 + 2 * len(ql.levels)

    def count(self, y_true: torch.Tensor) -> None:
        """A batch whose sums went into `totals` inside the fused loss kernel."""
        self.n += y_true.numel()
        self.batches += 1

    def update(self, y_pred: torch.Tensor, y_true: torch.Tensor, loss: Optional[torch.Tensor] = None,
               count: bool = True, loss_weight: float = 1.0, delta: Optional[float] = None,
               loss_fn: Optional[nn.Module] = None) -> None:
        """Add a batch with torch ops (CPU tensors; the GPU path adds inside the fused loss kernel).  With `null_value`
        set the loss column is computed here: with `loss_fn` (a `HuberLoss` or `GaussLoss`; it is kept) or this Metrics'
        own from that loss, otherwise as the Huber loss of `delta` (`loss` and `loss_weight` are not used; without any of
        them the column, and with it `loss`, stays 0)."""
        if loss_fn is not None:
            self.loss_fn = loss_fn
            if isinstance(loss_fn, QuantileLoss) and self.null_value is None and self._sums is None:
                self.null_value = float("nan") if loss_fn.null_value is None else loss_fn.null_value
        if self._quantile() is not None:
            self._update_quantile(y_pred, y_true, self.loss_fn)
            if count:
                self.count(y_true)
            return
        if self.null_value is not None:
            self._update_masked(y_pred, y_true, delta, self.loss_fn)
            if count:
                self.count(y_true)
            return
        err = (y_pred.detach() - y_true).double()
        truth = y_true.double()
        mask = truth > self.mask_value
        ape = torch.where(mask, (err / torch.where(mask, truth, torch.ones_like(truth))).abs(), torch.zeros_like(err))
        zero = err.new_zeros(())
        s = torch.stack([err.abs().sum(), 100.0 * ape.sum(), (err * err).sum(),
                         zero if loss is None else loss.detach().double() * loss_weight])
        self.totals(y_pred.device).add_(s)
        if count:
            self.count(y_true)

    def _update_masked(self, y_pred: torch.Tensor, y_true: torch.Tensor, delta: Optional[float],
                       loss_fn: Optional[nn.Module] = None) -> None:
        """What `ops.masked_huber_metrics` / `ops.masked_gauss_metrics` add to the buffer, in float64 torch ops."""
        t_out = y_true.shape[-1]
        truth = y_true.double().reshape(-1, t_out)
        valid = valid_entries(truth, self.null_value)
        zero = torch.zeros_like(truth)
        err = torch.where(valid, y_pred.detach().double().reshape(-1, t_out) - truth, zero)
        mask = valid & (truth > self.mask_value)
        ape = torch.where(mask, (err / torch.where(mask, truth, torch.ones_like(truth))).abs(), zero)
        a = err.abs()
        if loss_fn is not None:
            entry = loss_fn.entry(a)          # 0 at a = 0, where the entries that are not valid sit
        else:
            entry = zero if delta is None else torch.where(a <= delta, 0.5 * a * a, delta * a - 0.5 * delta * delta)
        rows = torch.stack([valid.double().sum(0), a.sum(0), 100.0 * ape.sum(0), (err * err).sum(0), entry.sum(0)], dim=1)
        sums = self.totals(y_pred.device, t_out)
        sums[:t_out].add_(rows)
        sums[t_out].add_(rows.sum(0))

    def _update_quantile(self, y_pred: torch.Tensor, y_true: torch.Tensor, loss_fn: "QuantileLoss") -> None:
        """What `ops.quantile_metrics` adds to the buffer, in float64 torch ops."""
        p, y, valid, rho = quantile_entries(y_pred.detach().double(), y_true.double(), loss_fn.levels, self.null_value)
        t_out, q = y_true.shape[-1], len(loss_fn.levels)
        p, y, rho = p.reshape(-1, q, t_out), y.reshape(-1, 1, t_out), rho.reshape(-1, q, t_out)
        valid = valid.reshape(-1, t_out)
        zero = torch.zeros_like(y[:, 0])
        err = torch.where(valid, p[:, loss_fn.point] - y[:, 0], zero)
        mask = valid & (y[:, 0] > self.mask_value)
        ape = torch.where(mask, (err / torch.where(mask, y[:, 0], torch.ones_like(zero))).abs(), zero)
        crossing = valid & (p[:, :-1] > p[:, 1:]).any(dim=1)
        width = torch.where(valid, p[:, -1] - p[:, 0], zero)
        hits = valid.unsqueeze(1) & (y <= p)
        cols = [valid.double().sum(0), err.abs().sum(0), 100.0 * ape.sum(0), (err * err).sum(0), rho.sum((0, 1)) / q,
                crossing.double().sum(0), width.sum(0), *hits.double().sum(0), *rho.sum(0)]
        rows = torch.stack(cols, dim=1)
        sums = self.totals(y_pred.device, t_out)
        sums[:t_out].add_(rows)
        sums[t_out].add_(rows.sum(0))

    def _get(self, i: int) -> float:
        return 0.0 if self._sums is None else float(self._sums[i].item())

    def _masked_total(self, column: int) -> float:
        """Column `column` of the all-horizon row over the epoch's valid count (at least 1)."""
        if self._sums is None:
            return 0.0
        last = self._sums[-1].tolist()
        return last[column] / max(last[0], 1.0)

    def per_horizon(self) -> Dict[str, List[float]]:
        """MAE / MAPE / RMSE and the valid count of every forecast horizon: lists of length T_out (needs `null_value`).
        With `loss_fn` known also "loss": the horizon's loss sum over its valid count, for whichever loss ran."""
        if self.null_value is None:
            raise ValueError("per-horizon metrics need Metrics(null_value=...): the unmasked totals are kept over all horizons")
        named = {} if self.loss_fn is None else {"loss": []}
        ql = self._quantile()
        if ql is not None:
            named.update(coverage=[[] for _ in ql.levels], pinball=[[] for _ in ql.levels], crossing=[], width=[])
        if self._sums is None:
            return {"MAE": [], "MAPE": [], "RMSE": [], "valid": [], **named}
        rows = self._sums[:-1].cpu()
        n = rows[:, 0].clamp(min=1.0)
        if named:
            named["loss"] = (rows[:, 4] / n).tolist()
        if ql is not None:
            named.update(self._quantile_columns(rows, n, len(ql.levels)))
        return {"MAE": (rows[:, 1] / n).tolist(), "MAPE": (rows[:, 2] / n).tolist(),
                "RMSE": (rows[:, 3] / n).sqrt().tolist(), "valid": rows[:, 0].tolist(), **named}

    @staticmethod
    def _quantile_columns(rows: torch.Tensor, n: torch.Tensor, q: int) -> dict:
        """Coverage (hits over the valid count) and mean pinball loss per level, crossing rate and mean width of the rows
        of a quantile totals buffer: [Q][len(rows)] and [len(rows)] lists."""
        return {"coverage": (rows[:, 7:7 + q] / n[:, None]).t().tolist(),
                "pinball": (rows[:, 7 + q:7 + 2 * q] / n[:, None]).t().tolist(),
                "crossing": (rows[:, 5] / n).tolist(), "width": (rows[:, 6] / n).tolist()}

    def quantile_summary(self) -> dict:
        """Over all horizons: {"levels", "coverage" (per level, the share of valid entries with y <= p_q: a calibrated
        forecast has coverage = level), "pinball" (per level), "crossing" (share of entries whose levels cross), "width"
        (mean p_{Q-1} - p_0)}.  Needs a `QuantileLoss` as `loss_fn`."""
        ql = self._quantile()
        if ql is None:
            raise ValueError("quantile_summary() needs Metrics(loss_fn=QuantileLoss(...))")
        q = len(ql.levels)
        if self._sums is None:
            return {"levels": list(ql.levels), "coverage": [0.0] * q, "pinball": [0.0] * q, "crossing": 0.0, "width": 0.0}
        last = self._sums[-1:].cpu()
        got = self._quantile_columns(last, last[:, 0].clamp(min=1.0), q)
        return {"levels": list(ql.levels), "coverage": [c[0] for c in got["coverage"]],
                "pinball": [c[0] for c in got["pinball"]], "crossing": got["crossing"][0], "width": got["width"][0]}

    def at(self, steps) -> Dict[str, List[float]]:
        """`per_horizon()` at the 1-based horizon steps `steps`, e.g. `at([3, 6, 12])`."""
        every = self.per_horizon()
        t_out = len(every["valid"])
        for step in steps:
            if not 1 <= int(step) <= t_out:
                raise IndexError(f"horizon step {step} outside 1..{t_out}")
        pick = lambda v: [v[int(step) - 1] for step in steps]  # noqa: E731
        return {k: [pick(level) for level in v] if k in ("coverage", "pinball") else pick(v) for k, v in every.items()}

    def all_reduce(self) -> None:
        if self.null_value is not None:
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and self._sums is not None:
                dist.all_reduce(self._sums)    # the whole buffer, in place: captured kernels keep adding to it
            return
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and self._sums is not None:
            buf = torch.cat([self._sums, self._sums.new_tensor([float(self.n)])])
            dist.all_reduce(buf)
            self._sums.copy_(buf[:4])      # in place: the kernels of a captured step keep adding to THIS buffer
            self.n = int(buf[4].item())

    @property
    def MAE(self) -> float:
        if self.null_value is not None:
            return self._masked_total(1)
        return self._get(0) / max(self.n, 1)

    @property
    def MAPE(self) -> float:
        if self.null_value is not None:
            return self._masked_total(2)
        return self._get(1) / max(self.n, 1)

    @property
    def RMSE(self) -> float:
        if self.null_value is not None:
            return self._masked_total(3) ** 0.5
        return (self._get(2) / max(self.n, 1)) ** 0.5

    @property
    def loss(self) -> float:
        """Mean over the (global) batches of the batch-mean loss, the reference's `loss_ave` (engine.py:66-67).
        With `null_value` set: the epoch's total loss sum divided by its total valid count (a ratio of totals, see
        the class docstring)."""
        if self.null_value is not None:
            return self._masked_total(4)
        return self._get(3) / max(self.batches, 1)

    def todict(self):
        return {"MAE": self.MAE, "MAPE": self.MAPE, "RMSE": self.RMSE}


def check_max_grad_norm(max_grad_norm) -> None:
    if max_grad_norm is not None and not float(max_grad_norm) > 0.0:      # also refuses NaN
        raise ValueError(f"max_grad_norm must be a positive number or None, not {max_grad_norm!r}")


def check_ema_decay(ema_decay) -> None:
    if ema_decay is None:
        return
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= float(ema_decay) < 1.0:   # also NaN
        raise ValueError(f"ema_decay must be a float in [0, 1) or None, not {ema_decay!r}")


def check_accumulate_steps(accumulate_steps) -> None:
    if isinstance(accumulate_steps, bool) or not isinstance(accumulate_steps, int) or accumulate_steps < 1:
        raise ValueError(f"accumulate_steps must be an int >= 1, not {accumulate_steps!r}")


def average_rate(decay: float, step) -> torch.Tensor:
    """1 - d of the averaged weights, d = min(decay, (1 + t) / (10 + t)) at the (already advanced) step count t: three
    separately rounded fp32 operations, as `k_adam` takes them (csrc/tail.hip)."""
    t = torch.as_tensor(float(step), dtype=torch.float32)
    d = torch.minimum(torch.tensor(float(decay), dtype=torch.float32), (1.0 + t) / (10.0 + t))
    return 1.0 - d


class FlatAdam(optim.Optimizer):
    """`torch.optim.Adam` (engine.py:106; L2 weight decay on the gradient, bias correction, eps outside the
    square root) as ONE launch over flat state buffers (`msgat_adam_step`, csrc/tail.hip).

    The gradients are gathered into one flat fp32 buffer (the buffer a multi-rank step all-reduces, so the
    collective and the update share it), both moments are flat, and the parameters stay where they are -- views
    of the parameter bank (`stacked.ParamBank`) -- reached through a device table of 2048-element chunks.  The
    step count and the learning rate live in device memory: a captured launch follows `StepLR`.
    `state_dict()` / `load_state_dict()` speak torch.optim.Adam's format (per-parameter `step`, `exp_avg`,
    `exp_avg_sq`), so checkpoints interchange with the reference's optimizer.

    Who writes a parameter: the update kernels (`msgat_adam_step` and its guarded and averaged forms) and
    `msgat_param_swap` write it through its device address.  No tensor's version counter moves, and inside a captured
    step no Python runs at all, so nothing derived from a trained parameter may be cached on its identity or version.
    The library's own caches follow that: a dense adjacency that requires grad has its values re-read from the tensor at
    every call (`graph.graph_of`, `graph.batched_graph_of`), a sparse one's are read where they sit.  Anything a caller
    derives from a parameter on the host must be derived again after a step, a replay or a swap.

    The guard (`max_grad_norm`, `skip_nonfinite`; off unless one is set, and then nothing here changes): two more launches
    (`msgat_grad_guard`) take the global L2 norm of the flat gradient -- on one GPU after the copy into the flat views, with
    several ranks after the all-reduce and the clamp of the divisor, so every rank decides from the same bits and the norm
    is that of the global-batch mean gradient -- and leave `coef = min(1, max_grad_norm / (norm + 1e-6))` (1 without
    `max_grad_norm`) and a finite flag in device memory, where the update (`msgat_adam_step_guarded`) reads them:
    `g = weight_decay * w + coef * grad`, i.e. `clip_grad_norm_` followed by `optim.Adam`.  While the guard is active a
    step whose norm is Inf or NaN writes nothing -- no parameter, no moment, no step count; only the skipped counter
    moves -- which is `GradScaler.step`'s behaviour and on purpose NOT `clip_grad_norm_`'s (it would scale every gradient
    by NaN).  Nothing is read back: `guard_stats()` is the only call that synchronises.  The host cannot know which
    steps were left out, so with the guard on the step counts in device memory are the truth and `state_dict()` reads
    them back.

    The average (`ema_decay`, a float in [0, 1); None, the default, changes nothing here): `shadow`, one more flat buffer
    next to the moments, starts as a copy of the parameters and is moved by the update launch itself
    (`msgat_adam_step_averaged`, guarded or not): `e += (1 - d) * (w_new - e)` with `d = min(ema_decay, (1 + t) / (10 + t))`
    and t the tensor's own step count -- so a tensor without a gradient keeps its shadow, a step the guard leaves out moves
    none, and after the all-reduce every rank holds the same bits.  `swap_averaged()` exchanges parameters and shadow in
    place (one launch, `msgat_param_swap`; twice = the identity) and `averaged_parameters()` does so around a block: whoever
    holds the parameters' addresses -- a captured validation graph -- then reads the averaged weights.  While they are
    swapped in, `step()`, `state_dict()` and `averaged_state()` raise: the parameters are not the trained ones.
    `averaged_state()` / `load_averaged_state()` carry the shadow to and from checkpoints, in place.

    Gradient accumulation (`accumulate(weight)`; never called: nothing here changes): a window of k micro-batches is ONE
    step on their union.  `accumulate(w)` adds `w * p.grad` into the flat buffer and `w` into its last element -- the first
    micro-batch of a window through the overwriting gather, later ones through `msgat_gather_accumulate{,_dev}` (product
    and sum rounded one after the other: the bits of an all-reduce sum over as many ranks) -- and `step(rank_weight=w)`
    adds the last one and closes the window: the all-reduce (several ranks: one collective per window), the clamp of the
    summed weight (device counts), then guard, update and average as the data-parallel step has them, dividing by the
    summed weight on the way in.  Step counts, the average and the guard move once per window; the guard sees the norm of
    the window's mean gradient, so one non-finite micro-batch leaves the whole window out.  `pending` counts the open
    window's micro-batches; while it is not 0, `state_dict()`, `swap_averaged()` and `averaged_state()` raise."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, ema_decay: Optional[float] = None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) != 1:
            raise ValueError("FlatAdam takes one parameter group (the reference trains with one, engine.py:106)")
        check_max_grad_norm(max_grad_norm)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self._guard = None            # [GUARD_FLOATS] fp32 on the device: norm, coef, skipped steps, largest norm, finite
        self._guard_partials = None   # one double per chunk of the whole layout
        check_ema_decay(ema_decay)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.shadow = None            # [numel] fp32: the averaged weights (with ema_decay), in the layout of the moments
        self.swapped = False          # True while the parameters hold the averaged weights and `shadow` the trained ones
        self._params: List[nn.Parameter] = []
        self._loaded_steps: Dict[int, float] = {}    # steps that arrived through load_state_dict, by id(param)
        self._host_steps: List[int] = []             # host mirror of the per-parameter step counts
        self._captured_active: Optional[tuple] = None
        self._tables: Dict[tuple, tuple] = {}
        self._gather_tables: dict = {}
        self._lr_on_device = None
        self._last_active: Optional[tuple] = None
        self.flat_grad = None
        self.numel = -1
        self._pending = 0                            # micro-batches in the open accumulation window
        self._window_active: Optional[tuple] = None  # the active set of the window's first micro-batch
        self._window_on_device = False               # the window's weights are device counts (clamped when it closes)
        self.param_names: Dict[int, str] = {}        # id(param) -> name, for messages (Trainer fills it in)

    # -- flat buffers ----------------------------------------------------------------------------------------
    def _build(self) -> None:
        self._params = [p for p in self.param_groups[0]["params"] if p.requires_grad]
        if not self._params:
            raise ValueError("no trainable parameters")
        dev = self._params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FlatAdam runs in libmsgat_hip.so on the GPU; use torch.optim.Adam for CPU parameters")
        self._offsets, off = [], 0
        for p in self._params:
            self._offsets.append(off)
            off += p.numel()
        # A rebuild with the same layout (load_state_dict on a live optimizer) keeps every device buffer and writes
        # into it: step graphs captured earlier hold these addresses (and those of the chunk tables).
        reuse = (self.flat_grad is not None and self.numel == off and self.flat_grad.device == dev
                 and len(self._host_steps) == len(self._params))
        self.numel = off
        self._host_steps = [int(self._loaded_steps.get(id(p), 0)) for p in self._params]
        steps = torch.tensor([float(t) for t in self._host_steps])
        if reuse:
            self._dev_steps.copy_(steps)
            self._dev_lr.fill_(float(self.param_groups[0]["lr"]))
        else:
            self.flat_grad = torch.zeros(off + 1, device=dev, dtype=torch.float32)   # + the rank's weight (all-reduce)
            self.exp_avg = torch.zeros(off, device=dev, dtype=torch.float32)
            self.exp_avg_sq = torch.zeros(off, device=dev, dtype=torch.float32)
            self._dev_steps = steps.to(dev)
            self._dev_lr = torch.tensor([float(self.param_groups[0]["lr"])], device=dev)
            if self.ema_decay is not None:
                self.shadow = torch.empty(off, device=dev, dtype=torch.float32)
                self.reset_average()
            self._tables.clear()
            self._gather_tables.clear()
            if self.guarded:          # here, not at the first guarded step: they exist before any capture
                from . import _lib
                chunk = int(_lib.checked().msgat_adam_chunk_elems())
                n_chunks = sum(-(-p.numel() // chunk) for p in self._params)
                old_guard = self._guard
                self._guard = torch.zeros(_lib.GUARD_FLOATS, device=dev, dtype=torch.float32)
                if old_guard is not None:     # new buffers (another layout or device): the counts so far go along
                    self._guard.copy_(old_guard)
                self._guard_partials = torch.zeros(int(_lib.checked().msgat_grad_guard_partial_doubles(n_chunks)), device=dev,
                                                   dtype=torch.float64)
        self._grad_views = [self.flat_grad[o:o + p.numel()].view_as(p) for p, o in zip(self._params, self._offsets)]
        self._lr_on_device = float(self.param_groups[0]["lr"])
        for i, (p, o) in enumerate(zip(self._params, self._offsets)):
            old = self.state.get(p, {})
            m, v = self.exp_avg[o:o + p.numel()].view_as(p), self.exp_avg_sq[o:o + p.numel()].view_as(p)
            if "exp_avg" in old:      # state that arrived through load_state_dict: move it into the flat buffers
                if old["exp_avg"].data_ptr() != m.data_ptr():
                    m.copy_(old["exp_avg"])
                    v.copy_(old["exp_avg_sq"])
            elif reuse:               # no state for this parameter in what was loaded: fresh moments
                m.zero_()
                v.zero_()
            self.state[p] = {"step": torch.tensor(float(self._host_steps[i])), "exp_avg": m, "exp_avg_sq": v}

    def buffer_token(self) -> tuple:
        """Addresses a captured step graph depends on; a change means such graphs must be dropped."""
        if self.flat_grad is None:
            return ()
        token = (self.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                 self._dev_steps.data_ptr(), self._dev_lr.data_ptr())
        if self.guarded:
            token += (self._guard.data_ptr(), self._guard_partials.data_ptr())
        if self.shadow is not None:
            token += (self.shadow.data_ptr(),)
        return token

    def _table(self, active: tuple):
        """Device chunk table of the parameters that have a gradient (torch's Adam skips the others)."""
        key = (active, tuple(p.data_ptr() for p in self._params))
        hit = self._tables.get(key)
        if hit is None:
            from . import _lib
            chunk = int(_lib.checked().msgat_adam_chunk_elems())
            ptrs, offs, lens, tens, act = [], [], [], [], []
            for i, (p, o, on) in enumerate(zip(self._params, self._offsets, active)):
                if not on:
                    continue
                if not p.is_contiguous():
                    raise RuntimeError("FlatAdam needs contiguous parameters")
                act.append(i)
                for s in range(0, p.numel(), chunk):
                    ptrs.append(p.data_ptr() + 4 * s)
                    offs.append(o + s)
                    lens.append(min(chunk, p.numel() - s))
                    tens.append(i)
            dev = self.flat_grad.device
            hit = (torch.tensor(ptrs, dtype=torch.int64).to(dev), torch.tensor(offs, dtype=torch.int64).to(dev),
                   torch.tensor(lens, dtype=torch.int32).to(dev), torch.tensor(tens, dtype=torch.int32).to(dev),
                   torch.tensor(act, dtype=torch.int32).to(dev), len(ptrs), len(act))
            self._tables[key] = hit       # never evicted: a captured step may hold the addresses of an older table
        return hit

    def _gather(self, grads: List[torch.Tensor], active: tuple, weight, accumulate: bool = False) -> None:
        """flat = weight * gradients, flat[-1] = weight, in ONE launch (`parallel.gather_scaled`); `accumulate`: added to
        what the buffer holds instead (a later micro-batch of a window)."""
        offsets = [o for o, on in zip(self._offsets, active) if on]
        parallel.gather_scaled(self.flat_grad, grads, offsets, weight, self.numel, self._gather_tables, accumulate=accumulate)

    # -- gradient accumulation ---------------------------------------------------------------------------------
    @property
    def pending(self) -> int:
        """The number of micro-batches in the open accumulation window (0: none is open)."""
        return self._pending

    def _refuse_while_pending(self, what: str) -> None:
        if self._pending:
            raise RuntimeError(f"FlatAdam.{what} while an accumulation window is open ({self._pending} micro-batch(es) "
                               f"pending): close it with step() first")

    def _name(self, i: int) -> str:
        p = self._params[i]
        return self.param_names.get(id(p), f"parameter {i} of shape {tuple(p.shape)}")

    def _add_micro_batch(self, weight, several_ranks: bool) -> None:
        """The current gradients, times `weight`, into the window: the first micro-batch through the overwriting gather
        (no zeroing pass), a later one through the accumulating gather, the weight into the buffer's last element."""
        active = tuple(p.grad is not None for p in self._params)
        grads = [p.grad for p in self._params if p.grad is not None]
        on_device = torch.is_tensor(weight)
        first = self._pending == 0
        if first:
            if several_ranks and active != self._last_active:
                self.flat_grad.zero_()           # parameters without a gradient contribute zeros on every rank
            self._window_active, self._window_on_device = active, on_device
        else:
            if active != self._window_active:
                i = next(j for j, (a, b) in enumerate(zip(active, self._window_active)) if a != b)
                raise RuntimeError(
                    f"gradient accumulation: {self._name(i)} {'has a' if active[i] else 'has no'} gradient in micro-batch "
                    f"{self._pending + 1} of the window but {'had none' if active[i] else 'had one'} in its first: a window's "
                    f"set of parameters with a gradient is that of its first micro-batch")
            if on_device != self._window_on_device:
                raise ValueError("gradient accumulation: the weights of one window are all floats (sample counts) or all "
                                 "one-element device tensors (valid counts)")
        if grads:
            self._gather(grads, active, weight if on_device else float(weight), accumulate=not first)
        else:
            slot = self.flat_grad[self.numel:]       # no gradient anywhere: the weight alone
            if not first:
                slot.add_(weight.reshape(1) if on_device else float(weight))
            elif on_device:
                slot.copy_(weight.reshape(1))
            else:
                slot.fill_(float(weight))
        self._pending += 1

    @torch.no_grad()
    def accumulate(self, weight) -> None:
        """Add the current `p.grad` of every trained parameter, times `weight`, into the open accumulation window (opening
        one if none is).  `weight`: this micro-batch's sample count (a float) or its valid count (a one-element float32
        device tensor, read where it lives).  Nothing is updated: `step()` closes the window."""
        self._refuse_while_swapped("accumulate()")
        if not self._params or self.flat_grad is None or self._params[0].device != self.flat_grad.device:
            self._build()
        self._add_micro_batch(weight, dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)

    def drop_window(self) -> None:
        """Forget the open window (after an error inside it): the next micro-batch opens a new one, which overwrites."""
        self._pending, self._window_active = 0, None

    def sync_lr(self) -> None:
        """Write the group's learning rate (a host float the scheduler edits) into device memory when it changed."""
        lr = float(self.param_groups[0]["lr"])
        if self._lr_on_device is not None and lr != self._lr_on_device:
            self._dev_lr.fill_(lr)
            self._lr_on_device = lr

    def note_replayed_step(self) -> None:
        """A HIP-graph replay ran the captured update: advance the host-side mirror of the step counts."""
        for i, on in enumerate(self._captured_active or ()):
            self._host_steps[i] += int(on)

    @torch.no_grad()
    def step(self, closure=None, rank_weight=None):
        """One update.  `rank_weight` (this rank's sample count) makes it a data-parallel step: the flat gradient
        buffer is all-reduced as sum(w g) / sum(w) -- the gradient of the mean loss over the global batch, also for
        uneven shards -- before the update, in the one collective of the step.
        A one-element float32 device tensor is accepted too (the valid count of a masked batch): the gather reads it on
        the device, and the summed weight is clamped to at least 1 before it divides -- counts are integers, so the
        clamp is exact whenever anything was valid, and a global batch without a valid entry gives a zero gradient.
        With an accumulation window open (`accumulate`) the current gradients are its last micro-batch, weighted by
        `rank_weight`, and the window closes: one step on the union of its micro-batches.  `rank_weight=None` then
        closes the window as it stands, without adding anything."""
        from . import _lib
        self._refuse_while_swapped("step()")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._params or self.flat_grad is None or self._params[0].device != self.flat_grad.device:
            self._build()
        active = tuple(p.grad is not None for p in self._params)
        divisor = 0
        several_ranks = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if rank_weight is not None and (self._pending or several_ranks):
            # the current gradients are the last micro-batch of the open window, or -- a data-parallel step -- a window of
            # their own: one launch before the collective (the gather, scaled by the weight, which also rides in the
            # buffer's last element).  Without a weight an open window closes as it stands (the shorter last one of an epoch)
            self._add_micro_batch(rank_weight, several_ranks)
        if self._pending:
            # the window closes: flat = sum(w g), last = sum(w) over its micro-batches and, after the collective, over the
            # ranks; the update divides by the summed weight on the way in (device counts: clamped to at least 1)
            active = self._window_active
            if several_ranks:
                parallel.all_reduce_flat(self.flat_grad)
            if self._window_on_device:
                self.flat_grad[self.numel:].clamp_(min=1.0)
            divisor = self.flat_grad.data_ptr() + 4 * self.numel
            self._pending, self._window_active = 0, None
        elif any(active):
            torch._foreach_copy_([v for v, on in zip(self._grad_views, active) if on],
                                 [p.grad for p in self._params if p.grad is not None])
        self._last_active = active
        self.sync_lr()
        ptrs, offs, lens, tens, act, n, n_act = self._table(active)
        g = self.param_groups[0]
        stream = torch.cuda.current_stream(self.flat_grad.device).cuda_stream
        adam = (ptrs.data_ptr(), offs.data_ptr(), lens.data_ptr(), tens.data_ptr(), n, act.data_ptr(), n_act,
                self.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self._dev_steps.data_ptr(),
                self._dev_lr.data_ptr(), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                divisor)
        if self.guarded:
            # the norm of what the update is about to consume: the flat views (one GPU) or the all-reduced sum over
            # its clamped divisor (several ranks: the same bits, hence the same decision, on every rank)
            max_norm = float("inf") if self.max_grad_norm is None else self.max_grad_norm
            _lib.checked().msgat_grad_guard(offs.data_ptr(), lens.data_ptr(), n, self.flat_grad.data_ptr(), divisor, max_norm,
                                            self._guard_partials.data_ptr(), self._guard.data_ptr(), stream)
        if self.shadow is not None:       # the guarded or the plain update, and the average, in the same launch
            _lib.checked().msgat_adam_step_averaged(*adam, self._guard.data_ptr() if self.guarded else 0,
                                                    self.shadow.data_ptr(), self.ema_decay, stream)
        elif self.guarded:
            _lib.checked().msgat_adam_step_guarded(*adam, self._guard.data_ptr(), stream)
        else:
            _lib.checked().msgat_adam_step(*adam, stream)
        if torch.cuda.is_current_stream_capturing():
            self._captured_active = active
        else:
            for i, on in enumerate(active):
                self._host_steps[i] += int(on)
        return loss

    @property
    def allreduce_bytes(self) -> int:
        if not self._params:
            self._build()
        return self.flat_grad.numel() * 4

    # -- torch.optim.Adam's checkpoint format ------------------------------------------------------------------
    def state_dict(self):
        self._refuse_while_swapped("state_dict()")
        self._refuse_while_pending("state_dict()")
        if self.guarded and self._params and self.flat_grad is not None:
            # the host mirror counted every launch, the device only the steps that were not left out
            self._host_steps = [int(t) for t in self._dev_steps.tolist()]
        for p, t in zip(self._params, self._host_steps):
            self.state[p]["step"] = torch.tensor(float(t))
        sd = super().state_dict()
        for group in sd["param_groups"]:            # the keys torch.optim.Adam writes, so the reference's loader accepts it
            group.setdefault("amsgrad", False)
            group.setdefault("maximize", False)
            group.setdefault("foreach", None)
            group.setdefault("capturable", False)
            group.setdefault("differentiable", False)
            group.setdefault("fused", None)
            group["lr"] = float(group["lr"])
        return sd

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._loaded_steps = {id(p): float(st["step"]) for p, st in self.state.items() if "step" in st}
        if self.param_groups[0]["params"] and self.param_groups[0]["params"][0].is_cuda:
            self._build()                             # moves the loaded moments and step counts into the flat buffers

    def set_steps(self, steps: List[int]) -> None:
        """Put the step counts (host mirror and device) back, e.g. after the warm-up iterations of a graph capture."""
        self._host_steps = list(steps)
        self._dev_steps.copy_(torch.tensor([float(t) for t in steps]))

    # -- the averaged weights ------------------------------------------------------------------------------------
    def _refuse_while_swapped(self, what: str) -> None:
        if self.swapped:
            raise RuntimeError(f"FlatAdam.{what} while the averaged weights are swapped in: the parameters are not the trained "
                               f"ones (leave averaged_parameters(), or call swap_averaged() again)")

    def _need_average(self) -> None:
        if self.ema_decay is None:
            raise RuntimeError("FlatAdam was built without ema_decay: there are no averaged weights")
        if not self._params or self.flat_grad is None:
            self._build()

    def _shadow_views(self) -> List[torch.Tensor]:
        return [self.shadow[o:o + p.numel()].view_as(p) for p, o in zip(self._params, self._offsets)]

    @torch.no_grad()
    def reset_average(self) -> None:
        """Start the average at the current parameters, in place."""
        torch._foreach_copy_(self._shadow_views(), [p.detach() for p in self._params])

    def swap_averaged(self) -> None:
        """Exchange parameters and shadow in place, bit for bit: one launch over the table of all trainable parameters."""
        from . import _lib
        self._need_average()
        self._refuse_while_pending("swap_averaged()")
        ptrs, offs, lens, _, _, n, _ = self._table((True,) * len(self._params))
        stream = torch.cuda.current_stream(self.flat_grad.device).cuda_stream
        _lib.checked().msgat_param_swap(ptrs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, self.shadow.data_ptr(), stream)
        self.swapped = not self.swapped

    @contextlib.contextmanager
    def averaged_parameters(self):
        """`with opt.averaged_parameters():` the model computes with the averaged weights; the trained ones come back
        when the block ends, also when it raises."""
        self.swap_averaged()
        try:
            yield
        finally:
            self.swap_averaged()

    def averaged_state(self) -> dict:
        """{"decay": ema_decay, "shadow": {index: tensor}}: a copy of the shadow of every trainable parameter, by its index
        in the parameter group (the indices of `state_dict()["state"]`)."""
        self._need_average()
        self._refuse_while_swapped("averaged_state()")
        self._refuse_while_pending("averaged_state()")
        index = {id(p): i for i, p in enumerate(self.param_groups[0]["params"])}
        return {"decay": self.ema_decay,
                "shadow": {index[id(p)]: e.clone() for p, e in zip(self._params, self._shadow_views())}}

    @torch.no_grad()
    def load_averaged_state(self, state: dict) -> None:
        """Write the shadows of `state` (from `averaged_state()`) into the flat buffer, in place: captured steps keep
        reading the same words.  Parameters that `state` does not name keep their shadow; the decay stays this optimizer's."""
        self._need_average()
        self._refuse_while_swapped("load_averaged_state()")
        views = {id(p): e for p, e in zip(self._params, self._shadow_views())}
        group = self.param_groups[0]["params"]
        for i, tensor in state["shadow"].items():
            views[id(group[int(i)])].copy_(tensor)

    def shadow_snapshot(self):
        """A copy of the shadow, for `shadow_restore` (None: no average, or nothing built yet)."""
        return None if self.shadow is None else self.shadow.clone()

    def shadow_restore(self, snapshot) -> None:
        """Undo what the warm-up of a graph capture did to the shadow; without a snapshot (the warm-up built the buffers)
        the average starts at the parameters, which the caller has put back."""
        if self.shadow is None:
            return
        if snapshot is None:
            self.reset_average()
        else:
            self.shadow.copy_(snapshot)

    # -- the guard ---------------------------------------------------------------------------------------------
    def guard_stats(self) -> Dict[str, float]:
        """What the guard saw: the last step's pre-clip norm and coefficient, the steps left out so far and the largest
        finite norm since `reset_guard_stats()`.  Reads device memory: the one call of the guard that synchronises."""
        if not self.guarded:
            raise RuntimeError("FlatAdam was built without max_grad_norm / skip_nonfinite: there is no guard to report")
        norm, coef, skipped, largest = (0.0, 1.0, 0.0, 0.0) if self._guard is None else self._guard[:4].tolist()
        return {"grad_norm": norm, "clip_coef": coef, "skipped_steps": int(skipped), "grad_norm_max": largest}

    def reset_guard_stats(self) -> None:
        """Start the running maximum of the norm afresh (the skipped count is cumulative and stays)."""
        if self._guard is not None:
            self._guard[3:4].zero_()

    def guard_snapshot(self):
        """Device step counts and guard state, for `guard_restore` (None: guard off, or nothing built yet)."""
        if self._guard is None:
            return None
        return self._dev_steps.clone(), self._guard.clone()

    def guard_restore(self, snapshot) -> None:
        """Undo guarded steps that must not count (the warm-up of a graph capture): a poisoned warm-up batch was left
        out on the device, so neither the host's step counts nor a second skipped count may survive it."""
        if self._guard is None:
            return
        if snapshot is None:
            self._guard.zero_()
            return
        self._dev_steps.copy_(snapshot[0])
        self._guard.copy_(snapshot[1])
        self._host_steps = [int(t) for t in snapshot[0].tolist()]


def _edge_dropout_streams(model: nn.Module) -> List[torch.Tensor]:
    """The {seed, step} buffers of every edge-dropout mask stream under `model` (`MSGAT(edge_dropout=p)`,
    `model.EdgeDropout`): device memory that a training forward advances."""
    return [m.edge_drop_state for m in model.modules() if isinstance(getattr(m, "edge_drop_state", None), torch.Tensor)]


def _edge_dropout_owner(model: nn.Module):
    """The module under `model` (itself, or what a data-parallel wrapper holds) that draws edge-dropout masks, or None."""
    inner = getattr(model, "module", model)
    return inner if getattr(inner, "edge_dropout", 0) and hasattr(inner, "edge_dropout_state") else None


class _GraphedStep:
    """One captured step for one batch shape: static input buffers, `replay()` per batch.

    Training steps are captured whole (forward, loss, backward and, on a single GPU, the optimizer
    step); with several ranks the graph ends after backward and the all-reduce and the optimizer run
    eagerly.  Capture follows PyTorch's whole-network recipe: warm-up iterations on a side stream
    (they initialise the optimizer's lazy state), then capture -- with parameters and optimizer state put back
    afterwards, so the captured run starts from exactly the state an eager run would."""

    def __init__(self, engine: "Engine", batch, training: bool, step_in_graph: bool, loss_weight: float = 1.0):
        model, opt = engine.model, engine.optimizer
        self.static = [t.clone() for t in batch]
        *inputs, truth = self.static
        self.training = training
        self.grads = None
        trained = saved_params = saved_state = None
        if training:
            trained = [p for group in opt.param_groups for p in group["params"] if p.requires_grad]
            saved_params = [p.detach().clone() for p in trained]
            saved_state = {p: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state.get(p, {}).items()}
                           for group in opt.param_groups for p in group["params"]}
            saved_steps = list(getattr(opt, "_host_steps", []))
            saved_guard = opt.guard_snapshot() if isinstance(opt, FlatAdam) else None
            saved_shadow = opt.shadow_snapshot() if isinstance(opt, FlatAdam) else None
            # the warm-up forwards draw edge-dropout masks and move their stream on: put it back with the parameters, so
            # that the first replay (the capture itself executes nothing) draws the step an eager run would have drawn
            saved_drop = [(s, s.clone()) for s in _edge_dropout_streams(model)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                if training:
                    opt.zero_grad(set_to_none=True)
                    engine._loss(model(*inputs), truth, None).backward()
                    if step_in_graph:
                        opt.step()
                else:
                    with torch.no_grad():
                        model(*inputs)
        torch.cuda.current_stream().wait_stream(side)
        if training:   # undo the warm-up: parameters and optimizer state as before it (fresh state = zeros)
            with torch.no_grad():
                for p, old in zip(trained, saved_params):   # not the frozen adjacency: its version keys the CSR cache
                    p.copy_(old)
                for p, st in opt.state.items():
                    for k, v in st.items():
                        if torch.is_tensor(v) and v.is_cuda:
                            old = saved_state.get(p, {}).get(k)
                            v.copy_(old) if old is not None else v.zero_()
                if isinstance(opt, FlatAdam) and step_in_graph:
                    opt.set_steps(saved_steps if saved_steps else [0] * len(opt._host_steps))
                    opt.guard_restore(saved_guard)   # a warm-up batch the guard left out counts once: at its replay
                    opt.shadow_restore(saved_shadow)  # the parameters are back: the average the warm-up moved goes back too
                for s, old in saved_drop:
                    s.copy_(old)
            opt.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            if training:
                self.pred = model(*inputs)
                self.loss = engine._loss(self.pred, truth, engine._graph_metrics, loss_weight)
                self.loss.backward()
                if step_in_graph:
                    opt.step()
            else:
                with torch.no_grad():
                    self.pred = model(*inputs)
                    self.loss = engine._loss(self.pred, truth, engine._graph_metrics, loss_weight)
        if training:
            # the gradients of THIS capture live in its private pool: whoever reads p.grad after a replay (the eager
            # all-reduce + optimizer of a multi-rank step) must see these tensors, not those of a later capture
            self.grads = [(p, p.grad) for p in trained]

    def replay(self, batch):
        for dst, src in zip(self.static, batch):
            dst.copy_(src, non_blocking=True)
        self.graph.replay()
        if self.grads is not None:
            for p, g in self.grads:
                p.grad = g
        return self.pred, self.loss, self.static[-1]


class Engine:
    __labels__ = {"train": "[Train   ]", "validate": "[Validate]", "evaluate": "[Evaluate]"}

    def __init__(self, model: nn.Module, loss_delta: float, out_dir: str, null_value: Optional[float] = None,
                 loss: Optional[nn.Module] = None):
        self.model = model
        self._loss_given = loss is not None     # then the per-horizon statistics carry the loss too
        if loss is None:
            loss = HuberLoss(loss_delta, null_value)
        elif not isinstance(loss, (HuberLoss, GaussLoss, QuantileLoss)):
            raise TypeError(f"loss must be a HuberLoss, a GaussLoss or a QuantileLoss (the fused step tail runs the losses "
                            f"it knows), not {type(loss).__name__}")
        else:
            theirs = loss.null_value
            if null_value is not None and theirs is not None and not (
                    float(theirs) == float(null_value) or (math.isnan(theirs) and math.isnan(null_value))):
                raise ValueError(f"null_value = {null_value!r} but the loss was built with null_value = {theirs!r}")
            null_value = theirs if null_value is None else null_value
            loss.null_value = null_value         # one switch: the engine's, or the loss's own where the engine got none
            if isinstance(loss, QuantileLoss) and null_value is None:
                null_value = float("nan")        # a quantile forecast has the masked tail only: NaN masks the NaN entries
        self.null_value = null_value     # None: every entry of the truth counts (the reference's loss and metrics)
        self._valid_count = None         # [1] fp32: the valid count of the last batch (device memory on the GPU)
        self.loss_fn, self.out_dir = loss, Path(out_dir)
        self.out_dir.mkdir(parents=True, exist_ok=True)
        self.log_file = self.out_dir / "run.log"
        self.optimizer = None
        self._grad_sync = None
        self.hip_graph = False       # False | True | "auto" (see Trainer)
        self.graph_after = 3         # "auto": a batch shape is captured once it has been seen more often than this
        self._graph_seen = {}
        self._graphs = {}
        self._graph_metrics = None   # the Metrics whose device totals the captured loss kernels add to
        self.max_grad_norm: Optional[float] = None   # the guard on the optimizer step (see Trainer); off by default
        self.skip_nonfinite = False
        self._cpu_guard = {"grad_norm": 0.0, "clip_coef": 1.0, "skipped_steps": 0, "grad_norm_max": 0.0}
        self._skipped_reported = 0   # the cumulative skipped count at the last end of a training epoch
        self.ema_decay: Optional[float] = None       # the averaged weights (see Trainer); off by default
        self._cpu_shadow: Optional[List[torch.Tensor]] = None   # the average of CPU parameters under torch.optim.Adam
        self._cpu_swapped = False
        self.accumulate_steps = 1    # micro-batches per optimizer step (see Trainer); 1: every batch is a step
        self._cpu_window: Optional[list] = None      # [accumulators sum(w g) per trained parameter, sum(w), count]

    # -- helpers -------------------------------------------------------------------------
    def _device(self, gpu_id):
        if gpu_id is not None:
            return torch.device("cuda", gpu_id)
        return next(self.model.parameters()).device

    @staticmethod
    def _world() -> Tuple[int, int]:
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def _loss(self, pred: torch.Tensor, truth: torch.Tensor, metrics: Optional[Metrics],
              loss_weight: float = 1.0) -> torch.Tensor:
        """The loss of a batch (`loss_fn`: Huber or Gauss); feeds `metrics` (engine.py:56,66-70).  On the GPU one library
        pass does both.
        `loss_weight` = this rank's share of the global batch (1 without a process group).
        With `null_value` set: the masked loss and the per-horizon totals; the batch's valid count stays in
        `_valid_count` (one buffer for every step, so captured kernels and the rank weight of a replay find it)."""
        mask_value = 0.0 if metrics is None else metrics.mask_value
        if isinstance(self.loss_fn, QuantileLoss):
            from . import ops
            ops.quantile_widths(pred, truth, len(self.loss_fn.levels))      # ValueError that names both sizes
        if self.null_value is not None:
            if pred.is_cuda:
                sums = None if metrics is None else metrics.totals(pred.device, truth.shape[-1])
                return self.loss_fn.fused(pred, truth, mask_value, sums, valid=self._valid_buffer(pred.device))
            self._valid_count = valid_entries(truth, self.null_value).sum().to(torch.float32).reshape(1)
            if metrics is not None:
                self._update_masked_on_cpu(metrics, pred, truth)
            return self.loss_fn(pred, truth)
        if pred.is_cuda:
            sums = None if metrics is None else metrics.totals(pred.device)
            return self.loss_fn.fused(pred, truth, mask_value, sums, loss_weight)
        loss = self.loss_fn(pred, truth)
        if metrics is not None:
            metrics.update(pred, truth, loss, count=False, loss_weight=loss_weight)   # counted by the caller
        return loss

    def _update_masked_on_cpu(self, metrics: Metrics, pred: torch.Tensor, truth: torch.Tensor) -> None:
        """The masked totals of a CPU batch (counted by the caller): the loss column from the loss itself; for the default
        loss through `delta=`, as before there was a choice."""
        if self._loss_given:
            metrics.update(pred, truth, count=False, loss_fn=self.loss_fn)
        else:
            metrics.update(pred, truth, count=False, delta=self.loss_fn.delta)

    def _new_metrics(self) -> Metrics:
        return Metrics(null_value=self.null_value, loss_fn=self.loss_fn if self._loss_given else None)

    def _valid_buffer(self, device) -> torch.Tensor:
        if self._valid_count is None or self._valid_count.device != device:
            self._valid_count = torch.zeros(1, device=device, dtype=torch.float32)
        return self._valid_count

    def _step_weight(self, n_samples: int):
        # a rank's weight in the gradient mean: its sample count, or -- entries dropping out of a masked loss -- its
        # batch's valid count, which is in device memory: sum_r v_r g_r / sum_r v_r is the gradient of the global
        # masked mean for any split
        return float(n_samples) if self.null_value is None else self._valid_count

    # -- a learned dense adjacency under captured steps (graph._learned_graph_of) ----------------------------------
    # A captured step refills the adjacency's values on the pattern it was captured with.  Where the optimizer runs
    # inside the step, the warm-up's eager steps grow the pattern before the capture.  Where it runs outside (several
    # ranks, gradient accumulation), the first update after a capture fills every zero of a sparse-start graph: the
    # pattern is rebuilt right after that update and the captured steps are dropped, so the next batch captures anew.
    # Whatever still slips through -- a step captured before the pattern grew and replayed after -- is counted on the
    # device and raised at the end of the epoch, since no eager call on the tensor may ever come.
    def _recapture_outgrown(self) -> None:
        from . import graph
        if graph._CAPTURED and graph.learned_patterns_grew(list(self.model.parameters())):     # empty: no such adjacency
            self._graphs.clear()

    def _check_captured_patterns(self) -> None:
        from . import _lib, graph
        if not graph._CAPTURED:
            return
        try:
            graph.check_captured_patterns(list(self.model.parameters()))
        except _lib.MsgatError:
            self._graphs.clear()      # they hold the outgrown pattern: the next epoch captures anew
            raise

    def _optimizer_step(self, n_samples: int, world: int) -> None:
        weight = self._step_weight(n_samples)
        if isinstance(self.optimizer, FlatAdam):
            self.optimizer.step(rank_weight=weight if world > 1 else None)
            return
        self._cpu_step(weight, world)

    def _window_step(self, n_samples: Optional[int], world: int, close: bool) -> None:
        """One micro-batch of an accumulation window (`accumulate_steps` > 1), weighted like a rank of a data-parallel
        step; `close`: it is the window's last, the optimizer steps.  `n_samples` None: no micro-batch, only the closing
        of the shorter window an epoch ends with."""
        weight = None if n_samples is None else self._step_weight(n_samples)
        if isinstance(self.optimizer, FlatAdam):
            if close:
                self.optimizer.step(rank_weight=weight)
            else:
                self.optimizer.accumulate(weight)
            return
        if weight is not None:
            self._cpu_accumulate(weight)
        if close:
            total = self._cpu_close_window()
            self._cpu_step(total, world)

    @torch.no_grad()
    def _cpu_accumulate(self, weight) -> None:
        """The window in torch fp32 ops (CPU parameters under torch.optim.Adam): one accumulator per trained parameter,
        acc = acc + w * g with the product and the sum rounded one after the other, as the library's gather does."""
        params = self._trained()
        if self._cpu_window is None:
            self._cpu_window = [[None if p.grad is None else weight * p.grad for p in params], weight, 1]
            return
        accs = self._cpu_window[0]
        names = {id(p): name for name, p in self.model.named_parameters()}
        for i, p in enumerate(params):
            if (p.grad is None) != (accs[i] is None):
                raise RuntimeError(
                    f"gradient accumulation: {names.get(id(p), i)} {'has no' if p.grad is None else 'has a'} gradient in "
                    f"micro-batch {self._cpu_window[2] + 1} of the window, unlike in its first: a window's set of parameters "
                    f"with a gradient is that of its first micro-batch")
        for i, p in enumerate(params):
            if accs[i] is not None:
                accs[i] = accs[i] + weight * p.grad
        self._cpu_window[1] = self._cpu_window[1] + weight
        self._cpu_window[2] += 1

    @torch.no_grad()
    def _cpu_close_window(self):
        """p.grad = sum(w g) / max(sum w, 1): the window's mean gradient, in front of the all-reduce, the guard and
        `optimizer.step()`.  Returns sum w, this rank's weight in the gradient mean over ranks."""
        accs, total, _ = self._cpu_window
        self._cpu_window = None
        divisor = total.clamp(min=1.0) if torch.is_tensor(total) else max(total, 1.0)
        for p, a in zip(self._trained(), accs):
            p.grad = None if a is None else a / divisor
        return total

    def _cpu_step(self, weight, world: int) -> None:
        if world > 1:
            if self._grad_sync is None:
                self._grad_sync = parallel.FlatGradAllReduce(self.model.parameters())
            self._grad_sync(weight=weight)
        if self._cpu_swapped:
            raise RuntimeError("an optimizer step while the averaged weights are swapped in: the parameters are not the trained ones")
        if self._guarded() and not self._cpu_guard_passes():
            return                      # left out whole: the average does not move either
        self.optimizer.step()
        if self._cpu_shadow is not None:
            self._cpu_average()

    def _trained(self) -> List[nn.Parameter]:
        return [p for group in self.optimizer.param_groups for p in group["params"] if p.requires_grad]

    @torch.no_grad()
    def _cpu_average(self) -> None:
        """The average in torch fp32 ops (CPU parameters under torch.optim.Adam), after the step: what `k_adam` does on the
        GPU -- every operation rounded on its own, the clock each parameter's own step count, a parameter without a
        gradient (which Adam skipped) left alone."""
        for p, e in zip(self._trained(), self._cpu_shadow):
            if p.grad is None:
                continue
            omd = average_rate(self.ema_decay, self.optimizer.state[p]["step"])
            diff = p.detach() - e
            e.copy_(e + omd * diff)

    def _guarded(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _cpu_guard_passes(self) -> bool:
        """The guard in torch ops (CPU parameters under torch.optim.Adam; after the gradient all-reduce, so every rank sees
        the same norm): False = a non-finite norm, the step is left out; otherwise the gradients are clipped in place."""
        params = [p for group in self.optimizer.param_groups for p in group["params"] if p.grad is not None]
        g = self._cpu_guard
        if not params:
            g.update(grad_norm=0.0, clip_coef=1.0)
            return True
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))
        g["grad_norm"] = float(norm)
        if not bool(torch.isfinite(norm)):
            g["clip_coef"] = 0.0
            g["skipped_steps"] += 1
            return False
        g["grad_norm_max"] = max(g["grad_norm_max"], g["grad_norm"])
        g["clip_coef"] = 1.0
        if self.max_grad_norm is not None:
            nn.utils.clip_grad_norm_(params, self.max_grad_norm)
            g["clip_coef"] = min(1.0, self.max_grad_norm / (g["grad_norm"] + 1e-6))
        return True

    def guard_stats(self) -> Dict[str, float]:
        """`FlatAdam.guard_stats()`, or the same figures of the torch path: synchronises on the GPU."""
        if isinstance(self.optimizer, FlatAdam):
            return self.optimizer.guard_stats()
        return dict(self._cpu_guard)

    def _reset_guard_max(self) -> None:
        if isinstance(self.optimizer, FlatAdam):
            self.optimizer.reset_guard_stats()
        else:
            self._cpu_guard["grad_norm_max"] = 0.0

    def run_epoch(self, data, gpu_id=None, epoch=None, mode: str = "train") -> float:
        """One pass over `data` (an iterable of (X, H, D, Y) batches).  Returns the mean batch loss.

        Under torch.distributed every rank must see the SAME sequence of global batches and takes its dim-0 shard
        (`parallel.shard_batch`) -- loaders built by `data.make_loaders` under a process group are already sharded
        (`msgat_sharded`), each rank loading only its own samples of a shared per-epoch permutation.  Global batches
        with fewer samples than ranks are skipped on every rank alike."""
        training = mode == "train"
        self.model.train(training)
        device = self._device(gpu_id)
        rank, world = self._world()
        presharded = bool(getattr(data, "msgat_sharded", False))
        sampler = getattr(data, "batch_sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(0 if epoch is None else int(epoch))
        if self._graph_metrics is None or not self.hip_graph or device.type != "cuda":
            metrics = self._new_metrics()
        else:
            metrics = self._graph_metrics       # captured kernels hold its totals buffer: re-use it, zeroed
            metrics.reset()
        if self.hip_graph and device.type == "cuda":
            self._graph_metrics = metrics
            if self.null_value is None:
                metrics.totals(device)
        # sizes of the GLOBAL batches behind pre-sharded ones (the sampler knows them); without a sampler the
        # shards are taken to be even
        global_sizes = iter(sampler.global_batch_sizes()) if presharded and hasattr(sampler, "global_batch_sizes") else None
        guard = torch.cuda.device(device) if device.type == "cuda" else _NullContext()
        pred = loss = None
        guarded = training and self._guarded()
        if guarded:
            self._reset_guard_max()
        dropper = _edge_dropout_owner(self.model) if training and world > 1 else None
        # gradient accumulation: micro-batches 1 .. k-1 of a window are accumulated, the k-th steps; the update then stays
        # outside a captured step, as with several ranks (the graph ends after backward)
        window = self.accumulate_steps if training else 1
        step_in_graph = world == 1 and window == 1
        in_window = optimizer_steps = 0
        with guard, torch.set_grad_enabled(training):
            for batch in data:
                n_global = batch[0].shape[0]
                if world > 1 and not presharded:
                    if n_global < world:
                        continue
                    batch = parallel.shard_batch(batch, rank, world)
                elif world > 1:
                    n_global = next(global_sizes) if global_sizes is not None else n_global * world
                if dropper is not None:
                    # this rank's samples draw the masks they have in the global batch (shard_batch and the sharded
                    # sampler cut by the same bounds); n_global keys the captured graphs, so the offset is a constant of each
                    dropper.edge_dropout_sample_offset = parallel.shard_bounds(n_global, rank, world)[0]
                loss_weight = batch[0].shape[0] / n_global
                batch = [t.to(device, non_blocking=True) for t in batch]
                *inputs, truth = batch
                graphed = None
                if self.null_value is not None and device.type == "cuda":
                    metrics.totals(device, truth.shape[-1])     # both exist before a capture can begin
                    self._valid_buffer(device)
                if self.hip_graph and device.type == "cuda":
                    key = (training, tuple(tuple(t.shape) for t in batch), n_global)
                    graphed = self._graphs.get(key)
                    capture = graphed is None
                    if capture and self.hip_graph == "auto":
                        # a shape earns its graph by recurring: the ragged last batch of an epoch (or a one-off evaluation)
                        # is launched eagerly instead of paying two warm-up steps and a capture for a single replay
                        seen = self._graph_seen[key] = self._graph_seen.get(key, 0) + 1
                        capture = seen > self.graph_after
                    if capture:
                        # nothing may keep the autograd graph of an eager step alive across a capture: its AccumulateGrad nodes
                        # belong to the default stream, and a backward that meets them on the capturing stream breaks the
                        # capture (hipStreamEndCapture crashes) -- the previous iteration's `loss` / `pred` do exactly that
                        pred = loss = None
                        with torch.enable_grad():
                            graphed = self._graphs[key] = _GraphedStep(self, batch, training, step_in_graph=step_in_graph,
                                                                       loss_weight=loss_weight)
                if graphed is not None:
                    pred, loss, truth = graphed.replay(batch)
                    if training and step_in_graph and isinstance(self.optimizer, FlatAdam):
                        self.optimizer.note_replayed_step()
                else:
                    pred = self.model(*inputs)
                    loss = self._loss(pred, truth, metrics, loss_weight)
                    if training:
                        self.optimizer.zero_grad(set_to_none=True)
                        loss.backward()
                if training and window > 1:
                    in_window += 1
                    self._window_step(truth.shape[0], world, close=in_window == window)
                    if in_window == window:
                        in_window, optimizer_steps = 0, optimizer_steps + 1
                elif training and (not step_in_graph or graphed is None):
                    self._optimizer_step(truth.shape[0], world)
                if training and graphed is not None and not step_in_graph:
                    self._recapture_outgrown()
                metrics.count(truth)
            if in_window:       # the batch count was no multiple of the window: no gradient outlives the epoch
                self._window_step(None, world, close=True)
                optimizer_steps += 1
        if self._graphs:
            self._check_captured_patterns()
        if world > 1:
            if metrics._sums is None and self.null_value is None:
                metrics.totals(device)
            metrics.all_reduce()
        loss_ave = metrics.loss
        stats = {"loss": loss_ave, **metrics.todict()}
        if window > 1:
            stats["optimizer_steps"] = optimizer_steps
        horizons = None if self.null_value is None else metrics.per_horizon()
        quantiles = metrics.quantile_summary() if isinstance(self.loss_fn, QuantileLoss) else None
        if rank == 0:
            if mode == "evaluate":
                self.log_to_file(self.__labels__[mode], **stats)
            else:
                self.log_to_file(self.__labels__[mode], epoch=epoch, **stats)
            if horizons is not None and mode != "train":
                per = {k: "/".join(f"{v:.6g}" for v in horizons[k]) for k in ("MAE", "MAPE", "RMSE")}
                self.log_to_file(self.__labels__[mode], "per horizon", **({} if mode == "evaluate" else {"epoch": epoch}), **per)
            if quantiles is not None and mode != "train":
                per = {k: "/".join(f"{v:.6g}" for v in quantiles[k]) for k in ("levels", "coverage", "pinball")}
                self.log_to_file(self.__labels__[mode], "quantiles", **({} if mode == "evaluate" else {"epoch": epoch}), **per,
                                 crossing=f"{quantiles['crossing']:.6g}", width=f"{quantiles['width']:.6g}")
        if horizons is not None:
            stats["horizons"] = horizons
        if quantiles is not None:
            stats["quantiles"] = quantiles
        if guarded:      # the epoch's one read of the guard state; every rank took the same decisions
            seen = self.guard_stats()
            stats["skipped_steps"] = seen["skipped_steps"] - self._skipped_reported
            stats["grad_norm_max"] = seen["grad_norm_max"]
            self._skipped_reported = seen["skipped_steps"]
            if rank == 0:
                self.log_to_file(self.__labels__[mode], "guard", epoch=epoch, skipped_steps=stats["skipped_steps"],
                                 grad_norm_max=stats["grad_norm_max"])
        self.last_stats = stats
        return loss_ave

    def log_to_file(self, *args, **kwargs) -> None:
        """`date - label - k=v,...` lines appended to run.log (engine.py:85-92)."""
        with open(self.log_file, "a") as f:
            f.write(strftime("%Y/%m/%d %H:%M:%S", localtime()))
            f.write(" - " + " - ".join(f"{a}" for a in args))
            f.write(" - " + ",".join(f"{k}={v}" for k, v in kwargs.items()) + "\n")


class _NullContext:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class Trainer(Engine):
    """Adam(lr 1e-3, wd 5e-4), StepLR(30, 0.1), early stopping after 20 stale epochs, best-val checkpoints
    after epoch 20 (engine.py:104-133).  GPU parameters train with `FlatAdam` (one launch), CPU parameters (host-logic
    tests) with torch.optim.Adam -- same update, same checkpoint format."""

    def __init__(self, model: nn.Module, loss_delta: float, out_dir: str, hip_graph="auto",
                 null_value: Optional[float] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, loss: Optional[nn.Module] = None, ema_decay: Optional[float] = None,
                 accumulate_steps: int = 1):
        """`loss` (default None: `HuberLoss(loss_delta, null_value)`, the reference's training loss): a `HuberLoss` or a
        `GaussLoss` instance to train with instead; `loss_delta` is then not read.  It runs in the same step tail -- one
        library pass with the metrics, masked or not, captured or not -- and takes the engine's `null_value` (or gives the
        engine its own where the engine got none; two different ones: ValueError).  `last_stats["horizons"]` then also has
        a "loss" list.  A `QuantileLoss(quantiles)` trains a quantile forecast: the model has `out_timesteps = Q * T_out`
        outputs against `T_out`-step truths (another width: ValueError), the totals are always per horizon (without a
        `null_value` only NaN truths are masked, and `self.null_value` reads NaN), `last_stats["horizons"]` gains
        "coverage", "pinball", "crossing" and "width", and `last_stats["quantiles"]` holds `Metrics.quantile_summary()`.
        Anything else is a TypeError: the fused tail runs the losses it knows.
        `max_grad_norm`, `skip_nonfinite` (default None / False: the step as the reference's optimizer takes it): a guard on
        the optimizer step, active when either is set.  The global L2 norm of the gradient -- of the global batch's mean
        gradient under a process group -- is taken before the update; the gradient is scaled by
        `min(1, max_grad_norm / (norm + 1e-6))` like `torch.nn.utils.clip_grad_norm_` (`skip_nonfinite` alone: never
        scaled), and a step whose norm is Inf or NaN (one NaN in X is enough) is left out whole -- parameters, moments and
        step counts untouched -- as `GradScaler.step` of the reference leaves it out; `clip_grad_norm_` would have scaled
        every gradient by NaN instead.  On the GPU all of it happens in the library, inside a captured step too
        (`FlatAdam`).  A training epoch then adds `skipped_steps` (this epoch's) and `grad_norm_max` to `last_stats` and one
        `guard` line to run.log.
        `ema_decay` (default None: off, and then no launch, bit, key or checkpoint changes; a float in [0, 1), e.g. 0.999):
        an exponential moving average of every trainable parameter, kept by the update itself: after a parameter's step,
        `e += (1 - d) (w - e)`, `d = min(ema_decay, (1 + t) / (10 + t))` with t that parameter's step count.  A parameter
        without a gradient, and every parameter in a step the guard leaves out, keeps its average.  `fit` validates on the
        averaged weights (`averaged_parameters()`), so the best checkpoint and the logged validation loss are theirs, with
        one more `average` log line per validation epoch; `save` adds the key `ema` = {"decay", "shadow": {name: tensor}}
        beside the raw weights under `model`, `load` restores it in place (a checkpoint without it: the average starts at the
        loaded parameters) and `Evaluator(weights="auto" | "raw" | "averaged")` picks the set to evaluate.
        `accumulate_steps` (default 1: every batch is a step, and no launch, bit, key or log line changes; an int >= 1):
        gradient accumulation -- k consecutive batches of a training epoch are the micro-batches of one window and ONE
        optimizer step on their union: each is weighted like a rank of a data-parallel step (its sample count, or its valid
        count under `null_value`), micro-batches 1 to k-1 are added into the optimizer's flat buffer
        (`FlatAdam.accumulate`), the k-th steps (`FlatAdam.step`), which divides by the summed weight.  The model has no
        batch statistics, so this is the step of a k times larger batch at the activation memory of one.  Step counts, the
        guard (one non-finite micro-batch leaves the whole window out) and the averaged weights move once per window, and
        under a process group the collective runs once per window.  An epoch whose batch count is no multiple of k closes
        its last, shorter window at its end: no gradient crosses validation, an epoch boundary or `save`.  Captured steps end
        after backward, as with several ranks, and the window's tail is launched eagerly.  `last_stats` and the train log
        line gain `optimizer_steps`.  CPU parameters get the same semantics in torch ops.
        `null_value` (default None: the reference's loss and metrics over every entry): entries of the truth that are
        NaN or equal to it are missing readings -- they drop out of the loss, its gradient and the metrics, the metrics are
        kept per forecast horizon (`last_stats["horizons"]`, one more log line per validation epoch), and under a process
        group a rank's weight in the gradient mean is its batch's valid count.
        `hip_graph`: "auto" (default) -- on the GPU a training / validation step is captured in a HIP graph once its batch
        shape has recurred `graph_after` (3) times and replayed from then on, other shapes are launched eagerly (a step of
        ~120 launches is host-bound wherever it is under ~3 ms of GPU work: msgat48 3.3 -> 2.8 ms, PEMSD4 2.7 -> 1.5 ms);
        True -- capture every shape at first sight; False -- eager launches only.  Graphs are keyed by (grad mode, batch
        shape, global batch size) and dropped when `load()` moves the optimizer's buffers."""
        super().__init__(model, loss_delta=loss_delta, out_dir=out_dir, null_value=null_value, loss=loss)
        on_gpu = next(model.parameters()).is_cuda
        if hip_graph is True and not on_gpu:
            raise ValueError("hip_graph=True needs the model on the GPU")
        if hip_graph not in (True, False, "auto"):
            raise ValueError(f"hip_graph must be True, False or 'auto', not {hip_graph!r}")
        self.hip_graph = hip_graph if on_gpu else False
        parallel.sync_parameters(model)     # data-parallel replicas start from rank 0's weights (no-op for one process)
        check_max_grad_norm(max_grad_norm)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        check_ema_decay(ema_decay)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        check_accumulate_steps(accumulate_steps)
        self.accumulate_steps = accumulate_steps
        if on_gpu:
            self.optimizer = FlatAdam(model.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=self.max_grad_norm,
                                      skip_nonfinite=self.skip_nonfinite, ema_decay=self.ema_decay)
            self.optimizer.param_names = {id(p): name for name, p in model.named_parameters()}
        else:
            self.optimizer = optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
            if self.ema_decay is not None:
                self._cpu_shadow = [p.detach().clone() for p in self._trained()]
        self.scheduler = lr_scheduler.StepLR(self.optimizer, step_size=30, gamma=0.1)
        self.best = {"epoch": 0, "loss": float("inf"), "ckpt": ""}
        self.epoch = 1
        self.patience, self.min_delta = 20, 1e-4
        self.max_epochs, self.min_epochs = 100, 20

    def fit(self, data_loaders, gpu_id=None) -> None:
        train, val = data_loaders
        while self.epoch <= self.max_epochs:
            self.run_epoch(train, gpu_id=gpu_id, epoch=self.epoch, mode="train")
            if self.ema_decay is None:
                loss = self.run_epoch(val, gpu_id=gpu_id, epoch=self.epoch, mode="validate")
            else:       # the validation loss, and with it the best checkpoint, are those of the averaged weights
                with self.averaged_parameters():
                    loss = self.run_epoch(val, gpu_id=gpu_id, epoch=self.epoch, mode="validate")
                if self._world()[0] == 0:
                    self.log_to_file(self.__labels__["validate"], "average", epoch=self.epoch, decay=self.ema_decay)
            self.scheduler.step()
            self._sync_lr()
            if self.epoch > self.min_epochs:
                if loss < (1 - self.min_delta) * self.best["loss"]:
                    self.best = dict(epoch=self.epoch, loss=loss, ckpt=self.out_dir / f"{self.epoch}_{loss:.2f}.pkl")
                    if self._world()[0] == 0:
                        self.save(ckpt=self.best["ckpt"])
                elif self.epoch > self.best["epoch"] + self.patience:
                    break
            self.epoch += 1

    def _sync_lr(self) -> None:
        if isinstance(self.optimizer, FlatAdam):
            self.optimizer.sync_lr()   # a captured update reads the rate from device memory

    # -- the averaged weights ------------------------------------------------------------------------------------
    def _need_average(self) -> None:
        if self.ema_decay is None:
            raise RuntimeError("Trainer was built without ema_decay: there are no averaged weights")

    @contextlib.contextmanager
    def averaged_parameters(self):
        """`with trainer.averaged_parameters():` the model holds the averaged weights, exchanged with the trained ones in
        place -- on the GPU by `FlatAdam.swap_averaged()`, so captured validation graphs need no recapture -- and gets the
        trained ones back when the block ends, also when it raises.  No optimizer step inside."""
        self._need_average()
        if isinstance(self.optimizer, FlatAdam):
            with self.optimizer.averaged_parameters():
                yield
            return
        self._cpu_swap()
        try:
            yield
        finally:
            self._cpu_swap()

    @torch.no_grad()
    def _cpu_swap(self) -> None:
        for p, e in zip(self._trained(), self._cpu_shadow):
            kept = p.detach().clone()
            p.copy_(e)
            e.copy_(kept)
        self._cpu_swapped = not self._cpu_swapped

    def _named_trained(self) -> List[Tuple[str, int]]:
        """(name in the model, index in the optimizer's group) of every trainable parameter, in the optimizer's order."""
        names = {id(p): name for name, p in self.model.named_parameters()}
        group = self.optimizer.param_groups[0]["params"]
        return [(names[id(p)], i) for i, p in enumerate(group) if p.requires_grad]

    def averaged_state(self) -> dict:
        """{"decay": ema_decay, "shadow": {parameter name: tensor}}: what `save` writes under `ema`."""
        self._need_average()
        if isinstance(self.optimizer, FlatAdam):
            shadow = self.optimizer.averaged_state()["shadow"]
            return {"decay": self.ema_decay, "shadow": {name: shadow[i] for name, i in self._named_trained()}}
        if self._cpu_swapped:
            raise RuntimeError("averaged_state() while the averaged weights are swapped in")
        return {"decay": self.ema_decay,
                "shadow": {name: e.clone() for (name, _), e in zip(self._named_trained(), self._cpu_shadow)}}

    @torch.no_grad()
    def _load_average(self, state: Optional[dict]) -> None:
        """The shadow from a checkpoint's `ema` entry, in place; None (a checkpoint of a run without the average): the
        average starts at the parameters just loaded."""
        named = self._named_trained()
        if isinstance(self.optimizer, FlatAdam):
            if state is None:
                self.optimizer._need_average()
                self.optimizer.reset_average()
            else:
                shadow = strip_data_parallel_prefix(state["shadow"])
                self.optimizer.load_averaged_state({"shadow": {i: shadow[strip_prefix(name)] for name, i in named}})
            return
        for (name, _), p, e in zip(named, self._trained(), self._cpu_shadow):
            e.copy_(p.detach() if state is None else strip_data_parallel_prefix(state["shadow"])[strip_prefix(name)])

    def save(self, ckpt) -> None:
        """The reference's five keys (engine.py:135-146).  `grad_scaler` holds the state of a default-constructed,
        enabled GradScaler -- this build trains in fp32 and never scales, but the reference's `load` feeds that entry
        to `GradScaler.load_state_dict`, which rejects an empty dict (engine.py:155).  A model that drops edges
        (`MSGAT(edge_dropout=p)`) adds a sixth key, `edge_dropout` = {seed, step} of its mask stream, which is no
        `state_dict` entry; every other model's checkpoint keeps the five.  With `ema_decay` set one more key, `ema` =
        {"decay", "shadow": {parameter name: tensor}}, holds the averaged weights; `model` stays the raw ones, which
        resuming needs and the reference's loader reads."""
        states = dict(best=self.best, epoch=self.epoch, model=self.model.state_dict(),
                      optimizer=self.optimizer.state_dict(), scheduler=self.scheduler.state_dict(),
                      grad_scaler=default_grad_scaler_state())
        dropper = _edge_dropout_owner(self.model)
        if dropper is not None:
            states["edge_dropout"] = dropper.edge_dropout_state()
        if self.ema_decay is not None:
            states["ema"] = self.averaged_state()
        torch.save(states, ckpt)

    def load(self, ckpt) -> None:
        states = torch.load(ckpt, map_location=next(self.model.parameters()).device, weights_only=False)
        self.best = states["best"]
        self.epoch = states["epoch"] + 1
        token = self.optimizer.buffer_token() if isinstance(self.optimizer, FlatAdam) else ()
        self.model.load_state_dict(strip_data_parallel_prefix(states["model"]))
        self.optimizer.load_state_dict(states["optimizer"])
        self.scheduler.load_state_dict(states["scheduler"])
        dropper = _edge_dropout_owner(self.model)
        if dropper is not None and states.get("edge_dropout") is not None:
            dropper.set_edge_dropout_state(states["edge_dropout"])      # in place: captured steps read the same words
        if self.ema_decay is not None:
            self._load_average(states.get("ema"))
        self._sync_lr()
        if isinstance(self.optimizer, FlatAdam) and token and token != self.optimizer.buffer_token():
            self._graphs.clear()            # the optimizer's buffers moved: captured steps point at the old ones
            self._graph_metrics = None


def default_grad_scaler_state() -> dict:
    """`torch.cuda.amp.GradScaler().state_dict()` of an enabled, never-stepped scaler (its constructor defaults)."""
    return {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 0}


class Evaluator(Engine):
    def __init__(self, model: nn.Module, delta: float, out_dir: str, ckpt, hip_graph="auto",
                 null_value: Optional[float] = None, loss: Optional[nn.Module] = None, weights: str = "auto"):
        # null_value, loss: see Trainer (with `loss` given, `delta` is not read)
        # weights: "auto" -- the averaged weights where the checkpoint has them (its `ema` key, Trainer(ema_decay=...)),
        # else the raw ones; "raw" -- always `model`; "averaged" -- KeyError without the `ema` key
        if weights not in ("auto", "raw", "averaged"):
            raise ValueError(f"weights must be 'auto', 'raw' or 'averaged', not {weights!r}")
        super().__init__(model, loss_delta=delta, out_dir=out_dir, null_value=null_value, loss=loss)
        states = torch.load(ckpt, map_location=next(model.parameters()).device, weights_only=False)
        if weights == "averaged" and states.get("ema") is None:
            raise KeyError(f"{ckpt}: no 'ema' key -- the checkpoint was written without averaged weights (Trainer(ema_decay=...))")
        state = dict(states["model"])
        self.weights = "raw"
        if weights != "raw" and states.get("ema") is not None:
            state.update(states["ema"]["shadow"])       # the trainable parameters; buffers and frozen ones stay
            self.weights = "averaged"
        model.load_state_dict(strip_data_parallel_prefix(state))
        self.hip_graph = hip_graph if next(model.parameters()).is_cuda else False   # see Trainer

    def eval(self, data_loader, gpu_id=None) -> float:
        return self.run_epoch(data_loader, gpu_id=gpu_id, mode="evaluate")


def strip_prefix(name: str) -> str:
    return name[len("module."):] if name.startswith("module.") else name


def strip_data_parallel_prefix(state_dict):
    """Checkpoints written through `nn.DataParallel` (main.py:54,60) prefix every key with `module.`."""
    if state_dict and all(k.startswith("module.") for k in state_dict):
        return {k[len("module."):]: v for k, v in state_dict.items()}
    return state_dict
