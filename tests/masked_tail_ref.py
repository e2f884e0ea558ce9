"""The yardstick of the masked step tail: a float64 torch restatement of its definitions, and the seeded inputs the
host and GPU tests share.

An entry of the truth is VALID when it is not NaN and != null_value.  Over the valid entries only:
  loss            sum huber(e) / max(valid count, 1),  e = pred - truth,
                  huber(e) = e^2 / 2 where |e| <= delta, delta |e| - delta^2 / 2 beyond
  sums[t, :]      {valid count, sum |e|, 100 sum_{truth > mask_value} |e / truth|, sum e^2, sum huber(e)} of horizon t
                  (the last axis of the tensors), t < T_out; sums[T_out, :] the same over all horizons
  dpred           dloss * clamp(e, -delta, delta) / max(valid count, 1) at valid entries, 0 elsewhere
"""
import torch


def valid_mask(truth, null_value):
    t = truth.double()
    return ~torch.isnan(t) & (t != null_value)


def restate(pred, truth, delta, null_value, mask_value=0.0, dloss=1.0):
    """-> dict(loss, valid, sums [T_out + 1, 5], dpred), everything float64 on the CPU."""
    t_out = pred.shape[-1]
    p, y = pred.detach().double().cpu().reshape(-1, t_out), truth.detach().double().cpu().reshape(-1, t_out)
    v = valid_mask(y, null_value)
    zero = torch.zeros_like(p)
    e = torch.where(v, p - y, zero)
    a = e.abs()
    huber = torch.where(v, torch.where(a <= delta, 0.5 * a * a, delta * a - 0.5 * delta * delta), zero)
    rel = v & (y > mask_value)
    ape = torch.where(rel, (e / torch.where(rel, y, torch.ones_like(y))).abs(), zero)
    rows = torch.stack([v.double().sum(0), a.sum(0), 100.0 * ape.sum(0), (e * e).sum(0), huber.sum(0)], dim=1)
    sums = torch.cat([rows, rows.sum(0, keepdim=True)])
    count = float(v.sum())
    dpred = torch.where(v, e.clamp(-delta, delta), zero) * (dloss / max(count, 1.0))
    return dict(loss=float(huber.sum()) / max(count, 1.0), valid=count, sums=sums, dpred=dpred.reshape(pred.shape))


def metrics_of(sums):
    """MAE / MAPE / RMSE / valid per row of a [T_out + 1, 5] totals buffer (rows 0..T_out-1: horizons, last: all)."""
    n = sums[:, 0].clamp(min=1.0)
    return dict(MAE=(sums[:, 1] / n).tolist(), MAPE=(sums[:, 2] / n).tolist(), RMSE=(sums[:, 3] / n).sqrt().tolist(),
                valid=sums[:, 0].tolist(), loss=(sums[:, 4] / n).tolist())


def make_inputs(shape, seed, delta, null_value=0.0, null_fraction=0.2, n_nan=0):
    """Seeded (pred, truth) fp32 CPU tensors: truth is positive and flow-like (20 .. 400) with `null_fraction` of its
    entries set to `null_value` and `n_nan` further entries set to NaN; |e| lies on both sides of delta -- in
    [0.05, 0.9] delta or [1.1, 2] delta, so that no entry sits within 1e-4 relative of the clamp boundary |e| = delta,
    which is asserted on the fp32 values the kernels see."""
    g = torch.Generator().manual_seed(seed)
    truth = 20.0 + 380.0 * torch.rand(shape, generator=g)
    inside = torch.rand(shape, generator=g) < 0.5
    mag = torch.where(inside, 0.05 + 0.85 * torch.rand(shape, generator=g), 1.1 + 0.9 * torch.rand(shape, generator=g))
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    pred = (truth + sign * mag * delta).float()
    truth = truth.float()
    e = (pred.double() - truth.double()).abs()
    assert bool(((e - delta).abs() > 1e-4 * delta).all()), "an entry within 1e-4 relative of the clamp boundary"
    assert bool((e < delta).any()) and bool((e > delta).any())
    n = truth.numel()
    order = torch.randperm(n, generator=g)
    n_null = int(round(null_fraction * n))
    flat = truth.reshape(-1)
    flat[order[:n_null]] = null_value
    flat[order[n_null:n_null + n_nan]] = float("nan")
    return pred, truth


def sharded_truth(truth, fractions, seed, null_value=0.0):
    """A copy of `truth` [B, ...] whose dim-0 halves (the shards of two ranks) have the given VALID fractions, the other
    entries set to `null_value`: shards of one global batch with clearly different valid counts."""
    g = torch.Generator().manual_seed(seed)
    out = truth.clone()
    half = (truth.shape[0] + 1) // 2
    for sl, keep in zip((slice(0, half), slice(half, None)), fractions):
        part = out[sl]
        part[torch.rand(part.shape, generator=g) >= keep] = null_value
    return out
