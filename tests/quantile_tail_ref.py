"""The yardstick of the quantile step tail: a float64 torch restatement of its definitions, and the seeded inputs the
host and GPU tests share.

pred [..., Q * T_out] holds, level-major, Q quantile forecasts p_q of truth [..., T_out]; the levels tau_q are the fp32
values the C ABI receives.  An entry of the truth is VALID when it is not NaN and != null_value (None: NaN only).  Over
the valid entries, with u = truth - p_q and e = p_point - truth:
  rho_q           max(tau_q u, (tau_q - 1) u)
  loss            sum (1/Q) sum_q rho_q / max(valid count, 1)
  sums[t, :]      {valid count, sum |e|, 100 sum_{truth > mask_value} |e / truth|, sum e^2, sum (1/Q) sum_q rho_q,
                  entries with any p_q > p_{q+1}, sum p_{Q-1} - p_0, Q counts of truth <= p_q, Q sums of rho_q} of
                  horizon t, t < T_out; sums[T_out, :] the same over all horizons          ([T_out + 1, 7 + 2Q])
  dpred           c_q * (dloss / max(valid count, 1)) at valid entries, 0 elsewhere; c_q = -tau_q / Q where truth > p_q,
                  (1 - tau_q) / Q where truth < p_q, (1/2 - tau_q) / Q at a tie -- formed in float64, rounded to fp32 once,
                  and the product taken in fp32: the arithmetic the kernel states, so the comparison is bit for bit
"""
import torch


def fp32_levels(levels):
    return torch.tensor(list(levels), dtype=torch.float32).double()


def point_of(levels):
    return min(range(len(levels)), key=lambda i: (abs(levels[i] - 0.5), i))


def valid_mask(truth, null_value):
    t = truth.double()
    if null_value is None:
        return ~torch.isnan(t)
    return ~torch.isnan(t) & (t != null_value)


def slopes(levels):
    """[3, Q] fp32: c_q for truth > p_q, truth < p_q, truth == p_q."""
    tau, q = fp32_levels(levels), float(len(levels))
    return torch.stack([-tau / q, (1.0 - tau) / q, (0.5 - tau) / q]).float()


def restate(pred, truth, levels, null_value=None, mask_value=0.0, point=None):
    """-> dict(loss, valid, sums [T_out + 1, 7 + 2Q], width_abs [T_out + 1]: sum |p_{Q-1} - p_0|, the scale of the signed
    width column), everything float64 on the CPU."""
    q, t_out = len(levels), truth.shape[-1]
    point = point_of(levels) if point is None else point
    p = pred.detach().double().cpu().reshape(-1, q, t_out)
    y = truth.detach().double().cpu().reshape(-1, t_out)
    v = valid_mask(y, null_value)
    zero = torch.zeros_like(y)
    ys = torch.where(v, y, zero)
    tau = fp32_levels(levels).reshape(1, q, 1)
    u = ys.unsqueeze(1) - p
    rho = torch.where(v.unsqueeze(1), torch.maximum(tau * u, (tau - 1.0) * u), torch.zeros_like(u))
    e = torch.where(v, p[:, point] - ys, zero)
    rel = v & (ys > mask_value)
    ape = torch.where(rel, (e / torch.where(rel, ys, torch.ones_like(ys))).abs(), zero)
    crossing = v & (p[:, :-1] > p[:, 1:]).any(dim=1)
    width = torch.where(v, p[:, -1] - p[:, 0], zero)
    hits = v.unsqueeze(1) & (ys.unsqueeze(1) <= p)
    cols = [v.double().sum(0), e.abs().sum(0), 100.0 * ape.sum(0), (e * e).sum(0), rho.sum((0, 1)) / q,
            crossing.double().sum(0), width.sum(0), *hits.double().sum(0), *rho.sum(0)]
    rows = torch.stack(cols, dim=1)
    count = float(v.sum())
    width_abs = width.abs().sum(0)
    return dict(loss=float(rho.sum()) / q / max(count, 1.0), valid=count, sums=torch.cat([rows, rows.sum(0, keepdim=True)]),
                width_abs=torch.cat([width_abs, width_abs.sum().reshape(1)]))


def dpred_fp32(pred, truth, levels, null_value, valid_count, dloss=1.0):
    """The fp32 torch expression of the gradient, shaped like pred [..., Q * T_out]: bit for bit what the kernel writes."""
    q, t_out = len(levels), truth.shape[-1]
    p = pred.detach().float().cpu().reshape(-1, q, t_out)
    y = truth.detach().float().cpu().reshape(-1, 1, t_out)
    v = valid_mask(y, null_value)
    c = slopes(levels).reshape(3, 1, q, 1)
    scale = torch.tensor(dloss, dtype=torch.float32) / torch.tensor(max(valid_count, 1.0), dtype=torch.float32)
    each = torch.where(y > p, c[0], torch.where(y < p, c[1], c[2])) * scale
    return torch.where(v, each, torch.zeros_like(each)).reshape(pred.shape)


def make_inputs(rows, t_out, levels, seed, null_value=0.0, nan_fraction=0.1, null_fraction=0.1, dead_horizon=None,
                n_ties=4, n_crossings=5):
    """Seeded (pred [rows, Q * T_out], truth [rows, T_out]) fp32 CPU tensors: truth flow-like (20 .. 400); the level
    forecasts are the truth plus noise plus an offset that grows with the level (mostly ordered, some crossing on their
    own), then `n_crossings` entries get p_0 and p_{Q-1} swapped, `n_ties` (entry, level) pairs get p_q == truth exactly;
    `nan_fraction` of the truth is set to NaN, `null_fraction` to `null_value`, and horizon `dead_horizon` wholly to
    `null_value`.  Ties and crossings are planted at entries that stay valid."""
    q = len(levels)
    g = torch.Generator().manual_seed(seed)
    truth = (20.0 + 380.0 * torch.rand(rows, t_out, generator=g)).float()
    offset = (torch.tensor(list(levels)) - 0.5).reshape(1, q, 1) * 60.0
    pred = (truth.unsqueeze(1) + offset + 15.0 * torch.randn(rows, q, t_out, generator=g)).float()
    n = rows * t_out
    order = torch.randperm(n, generator=g)
    n_nan, n_null = int(round(nan_fraction * n)), int(round(null_fraction * n))
    flat = truth.reshape(-1)
    keep = order[n_nan + n_null:]
    if dead_horizon is not None:
        keep = keep[keep % t_out != dead_horizon]
    for k, i in enumerate(keep[:n_ties].tolist()):
        pred[i // t_out, k % q, i % t_out] = flat[i]
    if q > 1:
        for i in keep[n_ties:n_ties + n_crossings].tolist():
            r, t = i // t_out, i % t_out
            lo, hi = float(pred[r, 0, t]), float(pred[r, q - 1, t])
            pred[r, 0, t], pred[r, q - 1, t] = max(lo, hi) + 1.0, min(lo, hi) - 1.0
    flat[order[:n_nan]] = float("nan")
    flat[order[n_nan:n_nan + n_null]] = null_value
    if dead_horizon is not None:
        truth[:, dead_horizon] = null_value
    return pred.reshape(rows, q * t_out), truth
