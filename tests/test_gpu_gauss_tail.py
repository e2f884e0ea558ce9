"""GPU: the Gauss loss in the step tail -- `msgat_gauss_{metrics,grad}` and `msgat_masked_gauss_{metrics,grad}` through
`ops.gauss_metrics` / `ops.masked_gauss_metrics`, `GaussLoss`, and the engine on top of them (eager and captured steps,
Evaluator).  Yardstick: the float64 restatement of tests/gauss_tail_ref.py, pinned to the reference's own numbers by
tests/test_gauss_tail_cpu.py.  Bars: loss and every totals entry 1e-5 relative, counts exact, dpred per entry
|a - b| <= 1e-5 |b| + 1e-7 max|b| and exactly 0 where the yardstick's is 0."""
import copy

import pytest
import torch

from conftest import record_err, rel_err
from gauss_tail_ref import grad_violations, make_inputs, plain_sums, restate

pytestmark = pytest.mark.gpu

MASK = 30.0
# one block, T_out no power of two; T_out = 1; T_out at the limit (256 lanes, none idle); several blocks with a T_out that
# does not divide 256 (240 lanes, 16 idle)
SHAPES = [(2, 23, 12), (3, 7, 1), (1, 5, 64), (2, 130, 40)]
PARAMS = [(1.0, 0.05), (20.0, 0.5), (1.0, 0.0)]


def _dev():
    return torch.device("cuda:0")


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 3 else f"s{v[0]:g}d{v[1]:g}"


def _plain(pred, truth, sigma, delta, sums=None, dloss=None, loss_weight=1.0):
    """-> loss (0-dim), sums [4], dpred, all on the device."""
    from ms_gat_amd import ops
    p = pred.to(_dev()).requires_grad_(True)
    if sums is None:
        sums = torch.zeros(4, device=_dev(), dtype=torch.float64)
    loss = ops.gauss_metrics(p, truth.to(_dev()), sigma, delta, MASK, sums, loss_weight)
    (loss if dloss is None else loss * dloss).backward()
    return loss.detach(), sums, p.grad


def _masked(pred, truth, sigma, delta, null_value=0.0, sums=None, dloss=None):
    """-> loss (0-dim), valid [1], sums [T_out + 1, 5], dpred, all on the device."""
    from ms_gat_amd import ops
    p = pred.to(_dev()).requires_grad_(True)
    if sums is None:
        sums = torch.zeros(p.shape[-1] + 1, 5, device=_dev(), dtype=torch.float64)
    valid = torch.full((1,), -1.0, device=_dev())
    loss = ops.masked_gauss_metrics(p, truth.to(_dev()), sigma, delta, null_value, MASK, sums, valid)
    (loss if dloss is None else loss * dloss).backward()
    return loss.detach(), valid, sums, p.grad


def _check(what, loss, sums, dpred, want_loss, want_sums, want_dpred):
    e_loss = abs(float(loss) - want_loss) / max(abs(want_loss), 1e-300)
    e_sums = float(((sums.cpu() - want_sums).abs() / want_sums.abs().clamp(min=1e-300)).max())
    n_bad, e_grad = grad_violations(dpred, want_dpred)
    print(f"{what}: loss {e_loss:.2e} sums {e_sums:.2e} dpred {e_grad:.2e} of the maximum, {n_bad} entries outside the bound")
    for key, err, bar in (("loss", e_loss, 1e-5), ("sums", e_sums, 1e-5), ("dpred / max", e_grad, 1e-5)):
        record_err(f"gauss tail {what}", key, err, bar)
    assert e_loss < 1e-5 and e_sums < 1e-5 and n_bad == 0
    d = dpred.double().cpu()
    assert bool((d[want_dpred == 0] == 0).all()) and not torch.isnan(d).any() and not torch.isnan(sums).any()


def _scale(sigma):
    return 4.0 * sigma if sigma == 1.0 else 30.0      # |e| / sigma from 0 to beyond 10: both regimes in every case


@pytest.mark.parametrize("params", PARAMS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_plain_loss_sums_and_gradient_match_the_yardstick(shape, params):
    sigma, delta = params
    pred, truth = make_inputs(shape, seed=sum(shape), scale=_scale(sigma), n_equal=3)
    want = restate(pred, truth, sigma, delta, None, MASK, dloss=0.75)
    loss, sums, dpred = _plain(pred, truth, sigma, delta, dloss=0.75, loss_weight=0.5)
    _check(f"plain {shape} {params}", loss, sums, dpred, want["loss"], plain_sums(want, 0.5), want["dpred"])
    assert int((want["dpred"] == 0).sum()) == 3


@pytest.mark.parametrize("params", PARAMS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_masked_loss_valid_sums_and_gradient_match_the_yardstick(shape, params):
    sigma, delta = params
    pred, truth = make_inputs(shape, seed=sum(shape) + 1, scale=_scale(sigma), null_fraction=0.2, n_nan=2, n_equal=3)
    assert int(torch.isnan(truth).sum()) == 2
    want = restate(pred, truth, sigma, delta, 0.0, MASK, dloss=0.75)
    assert 0 < want["valid"] < truth.numel() - 2
    loss, valid, sums, dpred = _masked(pred, truth, sigma, delta, dloss=0.75)
    assert float(valid) == want["valid"] and torch.equal(sums[:, 0].cpu(), want["sums"][:, 0])       # counts: exact
    _check(f"masked {shape} {params}", loss, sums, dpred, want["loss"], want["sums"], want["dpred"])
    assert bool((dpred[torch.isnan(truth).to(_dev())] == 0).all())


@pytest.mark.parametrize("sigma", [1.0, 20.0])
def test_errors_far_below_sigma_keep_their_loss(sigma):
    """|e| ~ 1e-3 sigma, delta = 0: 1 - exp(-t) with t ~ 5e-7.  `1.f - expf(-t)` is off by 3.5e-3 relative here; the bar
    is the tail's 1e-5."""
    pred, truth = make_inputs((2, 23, 12), seed=21, scale=1e-3 * sigma)
    assert float((pred.double() - truth.double()).abs().max()) < 1e-2 * sigma
    want = restate(pred, truth, sigma, 0.0, None, MASK)
    loss, sums, dpred = _plain(pred, truth, sigma, 0.0)
    _check(f"cancellation plain sigma {sigma}", loss, sums, dpred, want["loss"], plain_sums(want), want["dpred"])
    pred, truth = make_inputs((2, 23, 12), seed=21, scale=1e-3 * sigma, null_fraction=0.2)      # the nulls drop out
    want = restate(pred, truth, sigma, 0.0, 0.0, MASK)
    loss, valid, sums, dpred = _masked(pred, truth, sigma, 0.0)
    assert float(valid) == want["valid"] < truth.numel()
    _check(f"cancellation masked sigma {sigma}", loss, sums, dpred, want["loss"], want["sums"], want["dpred"])


def test_entries_without_an_error_give_exactly_zero_and_add_nothing():
    _, truth = make_inputs((2, 23, 12), seed=22, scale=1.0)
    loss, sums, dpred = _plain(truth.clone(), truth, 1.0, 0.05)       # delta > 0: sgn(0) = 0 is what is at stake
    assert float(loss) == 0.0 and not sums.any() and not dpred.any() and not torch.isnan(dpred).any()
    loss, valid, sums, dpred = _masked(truth.clone(), truth, 1.0, 0.05)
    assert float(loss) == 0.0 and float(valid) == truth.numel() and not dpred.any()
    assert not sums[:, 1:].any() and float(sums[-1, 0]) == truth.numel()
    # among entries with an error: the yardstick's zeros are zeros, and the sums are those of the others
    pred, truth = make_inputs((2, 23, 12), seed=23, scale=4.0, n_equal=50)
    want = restate(pred, truth, 1.0, 0.05, None, MASK)
    loss, sums, dpred = _plain(pred, truth, 1.0, 0.05)
    assert int((want["dpred"] == 0).sum()) == 50 and bool((dpred.cpu()[want["dpred"] == 0] == 0).all())
    _check("50 entries without an error", loss, sums, dpred, want["loss"], plain_sums(want), want["dpred"])


@pytest.mark.parametrize("sigma", [1.0, 20.0])
def test_saturated_entries_keep_the_linear_term(sigma):
    """|e| = 50 sigma exactly (integer truths), delta = 0.05: exp(-1250) underflows, the value of an entry is sigma^2 +
    delta |e| and the gradient delta sgn(e) / n."""
    delta = 0.05
    g = torch.Generator().manual_seed(24)
    truth = torch.randint(1100, 2000, (2, 23, 12), generator=g).float()
    sign = torch.where(torch.rand(truth.shape, generator=g) < 0.5, -1.0, 1.0)
    pred = truth + sign * 50.0 * sigma
    assert bool(((pred - truth).abs() == 50.0 * sigma).all()) and bool((sign < 0).any()) and bool((sign > 0).any())
    n = truth.numel()
    loss, sums, dpred = _plain(pred, truth, sigma, delta)
    want = sigma ** 2 + delta * 50.0 * sigma
    assert abs(float(loss) - want) < 1e-6 * want
    ref = delta * sign.double() / n
    assert bool(((dpred.double().cpu() - ref).abs() <= 1e-6 * ref.abs()).all())
    loss, valid, sums, dpred = _masked(pred, truth, sigma, delta)
    assert float(valid) == n and abs(float(loss) - want) < 1e-6 * want
    assert bool(((dpred.double().cpu() - ref).abs() <= 1e-6 * ref.abs()).all())
    assert abs(float(sums[-1, 4]) - n * want) < 1e-6 * n * want


def test_a_batch_without_a_valid_entry_gives_zero_loss_and_a_positive_zero_gradient():
    pred, truth = make_inputs((2, 130, 40), seed=25, scale=4.0, null_fraction=1.0)
    truth[0, 0, :5] = float("nan")
    loss, valid, sums, dpred = _masked(pred, truth, 1.0, 0.05)
    assert float(loss) == 0.0 and float(valid) == 0.0 and not sums.any() and not dpred.any()
    assert not torch.signbit(dpred).any() and not torch.isnan(loss) and not torch.isnan(sums).any()


def test_a_batch_with_one_valid_entry_beside_a_nan():
    pred, truth = make_inputs((2, 23, 12), seed=26, scale=4.0, null_fraction=1.0)
    truth[1, 20, 7] = 123.0
    truth[1, 20, 8] = float("nan")
    want = restate(pred, truth, 1.0, 0.05, 0.0, MASK)
    assert want["valid"] == 1.0 and want["sums"][7, 0] == 1.0
    loss, valid, sums, dpred = _masked(pred, truth, 1.0, 0.05)
    assert float(valid) == 1.0
    _check("one valid entry", loss, sums, dpred, want["loss"], want["sums"], want["dpred"])
    assert float(dpred[1, 20, 8]) == 0.0 and int((dpred != 0).sum()) == 1 and not torch.isnan(dpred).any()


def test_two_calls_on_the_same_input_give_the_same_bits():
    pred, truth = make_inputs((2, 130, 40), seed=27, scale=30.0, null_fraction=0.2, n_nan=2)
    for run in (lambda: _plain(pred, truth.nan_to_num(1.0), 20.0, 0.5), lambda: _masked(pred, truth, 20.0, 0.5)):
        for x, y in zip(run(), run()):
            assert torch.equal(x, y)


def test_two_batches_accumulate_into_one_totals_buffer():
    pred, truth = make_inputs((6, 23, 12), seed=28, scale=30.0, null_fraction=0.2)
    sums = torch.zeros(13, 5, device=_dev(), dtype=torch.float64)
    plain = torch.zeros(4, device=_dev(), dtype=torch.float64)
    halves = (slice(0, 4), slice(4, 6))
    for sl in halves:
        _masked(pred[sl], truth[sl], 20.0, 0.5, sums=sums)
        _plain(pred[sl], truth[sl], 20.0, 0.5, sums=plain)
    want = restate(pred, truth, 20.0, 0.5, 0.0, MASK)["sums"]
    assert torch.equal(sums[:, 0].cpu(), want[:, 0])
    assert float(((sums.cpu() - want).abs() / want.abs()).max()) < 1e-5
    whole = restate(pred, truth, 20.0, 0.5, None, MASK)["sums"][-1]
    means = sum(restate(pred[sl], truth[sl], 20.0, 0.5, None, MASK)["loss"] for sl in halves)      # sums[3]: batch means
    ref = torch.stack([whole[1], whole[2], whole[3], torch.tensor(means, dtype=torch.float64)])
    assert float(((plain.cpu() - ref).abs() / ref.abs()).max()) < 1e-5


def test_the_huber_ops_are_unchanged_by_the_gauss_ones_running_in_the_same_process():
    from ms_gat_amd import ops
    pred, truth = make_inputs((2, 130, 40), seed=29, scale=60.0, null_fraction=0.2)

    def huber():
        out = []
        p = pred.to(_dev()).requires_grad_(True)
        sums = torch.zeros(4, device=_dev(), dtype=torch.float64)
        loss = ops.huber_metrics(p, truth.to(_dev()), 50.0, MASK, sums)
        loss.backward()
        out += [loss.detach(), sums, p.grad]
        p = pred.to(_dev()).requires_grad_(True)
        sums = torch.zeros(41, 5, device=_dev(), dtype=torch.float64)
        valid = torch.zeros(1, device=_dev())
        loss = ops.masked_huber_metrics(p, truth.to(_dev()), 50.0, 0.0, MASK, sums, valid)
        loss.backward()
        return out + [loss.detach(), sums, valid, p.grad]

    before = huber()
    _plain(pred, truth, 20.0, 0.5)
    _masked(pred, truth, 20.0, 0.5)
    for x, y in zip(before, huber()):
        assert torch.equal(x, y)
    # and they are the Huber definitions still
    err = (pred.double() - truth.double()).abs()
    want = torch.where(err <= 50.0, 0.5 * err * err, 50.0 * err - 0.5 * 50.0 * 50.0).mean()
    assert abs(float(before[0]) - float(want)) < 1e-6 * float(want)
    assert float(before[5]) == float((truth != 0).sum())


def test_gauss_loss_on_device_tensors_is_the_op():
    from ms_gat_amd import GaussLoss, ops
    pred, truth = make_inputs((2, 23, 12), seed=30, scale=30.0, null_fraction=0.2, n_nan=2)
    y = truth.to(_dev())
    for null_value, op in ((None, lambda p: ops.gauss_metrics(p, y, 20.0, 0.5)),
                           (0.0, lambda p: ops.masked_gauss_metrics(p, y, 20.0, 0.5, 0.0))):
        if null_value is None:
            y = truth.nan_to_num(1.0).to(_dev())
        else:
            y = truth.to(_dev())
        a, b = (pred.to(_dev()).requires_grad_(True) for _ in range(2))
        la, lb = GaussLoss(20.0, 0.5, null_value=null_value)(a, y), op(b)
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(a.grad, b.grad) and float(la) > 0


# ---- engine -----------------------------------------------------------------------------------------------------------------
def _tiny_model_and_batches(n_batches, seed=0, nulls=True):
    """A small msgat48 (N = 32, B = 4) and batches whose truth has zeros -- a different share in every batch, so the
    valid counts of replayed batches differ."""
    from ms_gat_amd import data, model
    torch.manual_seed(seed)
    ds = data.SyntheticPEMS(n_nodes=32, n_edges=40, n_channels=1, in_hours=[1, 2], batch_size=4, days=2)
    net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj)
    g = torch.Generator().manual_seed(seed + 1)
    batches = []
    for i, b in zip(range(n_batches), ds.training):
        *inputs, y = b
        y = y.clone()
        if nulls:
            y[torch.rand(y.shape, generator=g) < (0.1, 0.5, 0.3, 0.7)[i % 4]] = 0.0
        batches.append([*inputs, y])
    assert len(batches) == n_batches
    return net.to(_dev()), batches


@pytest.mark.parametrize("null_value", [None, 0.0], ids=["plain", "masked"])
def test_training_steps_with_a_gauss_loss_in_a_hip_graph_match_the_eager_steps(tmp_path, null_value):
    """Six training steps eager against six with hip_graph=True (captured at the first batch, replayed on five others).
    Bars of test_masked_training_steps_in_a_hip_graph_match_the_eager_steps: losses 1e-4, parameters 2e-2."""
    from ms_gat_amd import GaussLoss, engine
    net, batches = _tiny_model_and_batches(6, nulls=null_value is not None)
    twin = copy.deepcopy(net)
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False, null_value=null_value, loss=GaussLoss(20.0, 0.5))
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True, null_value=null_value, loss=GaussLoss(20.0, 0.5))
    for i, b in enumerate(batches):
        le = eager.run_epoch([b], gpu_id=0, epoch=i + 1, mode="train")
        lg = graphed.run_epoch([b], gpu_id=0, epoch=i + 1, mode="train")
        ge, gg = (t.optimizer.flat_grad[: t.optimizer.numel] for t in (eager, graphed))
        print(f"step {i}: loss {le:.6f} / {lg:.6f} gradient rel err {rel_err(gg, ge):.2e}")
        assert le > 0 and abs(le - lg) < 1e-4 * abs(le), (i, le, lg)
        assert rel_err(gg, ge) < 5e-2, (i, rel_err(gg, ge))     # a stale valid count would be off by the counts' ratio
        if null_value is not None:
            assert eager.last_stats["horizons"]["valid"] == graphed.last_stats["horizons"]["valid"]
            assert sum(graphed.last_stats["horizons"]["valid"]) == int((b[-1] != 0).sum())
            assert graphed.last_stats["horizons"]["loss"] == pytest.approx(eager.last_stats["horizons"]["loss"], rel=1e-4)
    assert len(graphed._graphs) == 1
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name
    assert set(graphed.optimizer._host_steps) == set(eager.optimizer._host_steps) == {6}


def test_evaluator_with_a_gauss_loss_reports_it_per_horizon(tmp_path):
    from ms_gat_amd import GaussLoss, engine
    net, batches = _tiny_model_and_batches(3, seed=1)
    ckpt = tmp_path / "net.pkl"
    torch.save(dict(model=net.state_dict()), ckpt)
    ev = engine.Evaluator(net, 50.0, str(tmp_path / "masked"), ckpt, hip_graph=False, null_value=0.0, loss=GaussLoss(20.0, 0.5))
    loss = ev.eval(batches, gpu_id=0)
    net.eval()
    with torch.no_grad():
        pred = torch.cat([net(*[t.to(_dev()) for t in b[:-1]]) for b in batches])
    want = restate(pred, torch.cat([b[-1] for b in batches]), 20.0, 0.5, 0.0)
    n = want["sums"][:, 0].clamp(min=1.0)
    ref = dict(MAE=want["sums"][:, 1] / n, MAPE=want["sums"][:, 2] / n, RMSE=(want["sums"][:, 3] / n).sqrt(),
               loss=want["sums"][:, 4] / n)
    got = ev.last_stats["horizons"]
    assert sorted(got) == ["MAE", "MAPE", "RMSE", "loss", "valid"] and got["valid"] == want["sums"][:12, 0].tolist()
    for k, r in ref.items():
        assert len(got[k]) == 12
        for a, b in zip(got[k], r[:12].tolist()):
            assert abs(a - b) < 1e-5 * abs(b), (k, got[k], r)
    assert abs(loss - want["loss"]) < 1e-5 * want["loss"] and ev.last_stats["loss"] == loss
    assert abs(loss - float(ref["loss"][-1])) < 1e-5 * loss
    # unmasked: the reference's mean over every entry, batch by batch
    plain = engine.Evaluator(net, 50.0, str(tmp_path / "plain"), ckpt, hip_graph=False, loss=GaussLoss(20.0, 0.5))
    got_plain = plain.eval(batches, gpu_id=0)
    whole = restate(pred, torch.cat([b[-1] for b in batches]), 20.0, 0.5, None)
    assert abs(got_plain - whole["loss"]) < 1e-5 * whole["loss"] and "horizons" not in plain.last_stats
