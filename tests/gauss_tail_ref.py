"""The yardstick of the Gauss loss in the step tail: a float64 torch restatement of its definitions (the reference's
`gauss_loss`, loss.py:94-95, and its autograd), plain and masked, and the seeded inputs the host and GPU tests share.
tests/test_gauss_tail_cpu.py pins it to what the reference itself computed (tests/golden/gauss_loss_ref.npz).

With e = pred - truth, over the VALID entries (all of them when null_value is None; otherwise truth not NaN and
!= null_value):
  g(e)            sigma^2 (1 - exp(-e^2 / (2 sigma^2))) + delta |e|
  g'(e)           e exp(-e^2 / (2 sigma^2)) + delta sgn(e),  sgn(0) = 0
  loss            sum g(e) / max(valid count, 1)
  sums[t, :]      {valid count, sum |e|, 100 sum_{truth > mask_value} |e / truth|, sum e^2, sum g(e)} of horizon t (the
                  last axis of the tensors), t < T_out; sums[T_out, :] the same over all horizons
  dpred           dloss * g'(e) / max(valid count, 1) at valid entries, 0 elsewhere
In float64 the 1 - exp(-t) of the smallest errors used here (t ~ 5e-7) is good to 1e-10 relative: five orders below the
bars it serves.
"""
import torch


def valid_mask(truth, null_value):
    t = truth.double()
    if null_value is None:
        return torch.ones_like(t, dtype=torch.bool)
    return ~torch.isnan(t) & (t != null_value)


def restate(pred, truth, sigma, delta, null_value=None, mask_value=0.0, dloss=1.0):
    """-> dict(loss, valid, sums [T_out + 1, 5], dpred), everything float64 on the CPU."""
    t_out = pred.shape[-1]
    p, y = pred.detach().double().cpu().reshape(-1, t_out), truth.detach().double().cpu().reshape(-1, t_out)
    v = valid_mask(y, null_value)
    zero = torch.zeros_like(p)
    e = torch.where(v, p - y, zero)
    a = e.abs()
    w = torch.exp(-(a * a) / (2 * sigma ** 2))
    g = torch.where(v, sigma ** 2 * (1 - w) + delta * a, zero)
    rel = v & (y > mask_value)
    ape = torch.where(rel, (e / torch.where(rel, y, torch.ones_like(y))).abs(), zero)
    rows = torch.stack([v.double().sum(0), a.sum(0), 100.0 * ape.sum(0), (e * e).sum(0), g.sum(0)], dim=1)
    sums = torch.cat([rows, rows.sum(0, keepdim=True)])
    count = float(v.sum())
    slope = torch.where(v, e * w + delta * torch.sign(e), zero)
    return dict(loss=float(g.sum()) / max(count, 1.0), valid=count, sums=sums,
                dpred=(slope * (dloss / max(count, 1.0))).reshape(pred.shape))


def plain_sums(want, loss_weight=1.0):
    """The [4] totals of the unmasked tail {sum |e|, 100 sum |e / y|, sum e^2, loss_weight * loss} from a restatement
    with null_value=None."""
    last = want["sums"][-1]
    return torch.stack([last[1], last[2], last[3], torch.tensor(want["loss"] * loss_weight, dtype=torch.float64)])


def make_inputs(shape, seed, scale, null_value=0.0, null_fraction=0.0, n_nan=0, n_equal=0):
    """Seeded (pred, truth) fp32 CPU tensors: truth positive and flow-like (20 .. 400), pred = truth + errors of size
    ~`scale` (normal) with `n_equal` entries set to pred == truth; then `null_fraction` of the truth's entries set to
    `null_value` and `n_nan` further ones to NaN."""
    g = torch.Generator().manual_seed(seed)
    truth = (20.0 + 380.0 * torch.rand(shape, generator=g)).float()
    pred = (truth + scale * torch.randn(shape, generator=g)).float()
    n = truth.numel()
    order = torch.randperm(n, generator=g)
    pred.reshape(-1)[order[:n_equal]] = truth.reshape(-1)[order[:n_equal]]
    order = torch.randperm(n, generator=g)
    n_null = int(round(null_fraction * n))
    flat = truth.reshape(-1)
    flat[order[:n_null]] = null_value
    flat[order[n_null:n_null + n_nan]] = float("nan")
    return pred, truth


def grad_violations(got, want):
    """How many entries of the gradient `got` lie outside |a - b| <= 1e-5 |b| + 1e-7 max|b| of the yardstick's `want`
    (the floor: with delta = 0, fp32 exp underflows where float64 still holds 1e-50), and the worst error over max|b|."""
    a, b = got.detach().double().cpu(), want.double()
    top = float(b.abs().max())
    bad = (a - b).abs() > 1e-5 * b.abs() + 1e-7 * top
    return int(bad.sum()), float((a - b).abs().max()) / max(top, 1e-300)
