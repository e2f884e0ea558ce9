"""GPU: the masked step tail -- Huber loss and per-horizon metric sums over the valid entries of the truth
(`msgat_masked_huber_metrics`), its gradient with the valid count read from device memory (`msgat_masked_huber_grad`),
and the engine on top of them (eager and captured steps, Evaluator).  Yardstick: the float64 restatement of
tests/masked_tail_ref.py.  Bars: sums and loss 1e-5 relative (fp32 terms of one sign added in fp64), dpred 1e-5 relative
per entry, counts exact, dpred exactly 0 at invalid entries."""
import copy

import pytest
import torch

from conftest import record_err, rel_err
from masked_tail_ref import make_inputs, metrics_of, restate

pytestmark = pytest.mark.gpu

DELTA = 50.0
MASK = 30.0
# the issue's shapes: one block with T_out no power of two; two blocks with a ragged last one; T_out = 1; one block whose
# 252 lanes leave four idle; T_out = 64.  Then: 17 blocks; 67 blocks (the finish kernel's lanes take a second block
# each); 589 blocks' worth of entries on the 512-block ceiling (blocks take a second trip)
SHAPES = [(2, 5, 3), (3, 47, 24), (2, 33, 1), (2, 19, 36), (1, 7, 64), (4, 700, 12), (8, 1400, 12), (32, 883, 37)]


def _dev():
    return torch.device("cuda:0")


def _run(pred, truth, delta=DELTA, null_value=0.0, mask_value=MASK, sums=None, dloss=None):
    """-> loss (0-dim), valid [1], sums, dpred, all on the device."""
    from ms_gat_amd import ops
    p = pred.to(_dev()).requires_grad_(True)
    y = truth.to(_dev())
    if sums is None:
        sums = torch.zeros(p.shape[-1] + 1, 5, device=_dev(), dtype=torch.float64)
    valid = torch.full((1,), -1.0, device=_dev())
    loss = ops.masked_huber_metrics(p, y, delta, null_value, mask_value, sums, valid)
    (loss if dloss is None else loss * dloss).backward()
    return loss.detach(), valid, sums, p.grad


def _check(got, want, what):
    loss, valid, sums, dpred = got
    assert float(valid) == want["valid"] and torch.equal(sums[:, 0].cpu(), want["sums"][:, 0])       # counts: exact
    e_loss = abs(float(loss) - want["loss"]) / max(abs(want["loss"]), 1e-300)
    ref = want["sums"]
    e_sums = float(((sums.cpu() - ref).abs() / ref.abs().clamp(min=1e-300)).max())
    d, r = dpred.double().cpu(), want["dpred"]
    e_grad = float(((d - r).abs() / r.abs().clamp(min=1e-300))[r != 0].max()) if bool((r != 0).any()) else 0.0
    print(f"{what}: loss {e_loss:.2e} sums {e_sums:.2e} dpred {e_grad:.2e}")
    for key, err in (("loss", e_loss), ("sums", e_sums), ("dpred", e_grad)):
        record_err(f"masked tail {what}", key, err, 1e-5)
    assert e_loss < 1e-5 and e_sums < 1e-5 and e_grad < 1e-5
    assert bool((d[r == 0] == 0).all()) and not torch.isnan(d).any() and not torch.isnan(sums).any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_loss_sums_and_gradient_match_the_restatement(shape):
    pred, truth = make_inputs(shape, seed=sum(shape), delta=DELTA)
    want = restate(pred, truth, DELTA, 0.0, MASK, dloss=0.75)
    assert 0 < want["valid"] < truth.numel()
    _check(_run(pred, truth, dloss=0.75), want, str(shape))


def test_a_batch_without_a_valid_entry_gives_zero_loss_and_zero_gradient():
    pred, truth = make_inputs((3, 47, 24), seed=1, delta=DELTA, null_fraction=1.0)
    truth[0, 0, :5] = float("nan")
    loss, valid, sums, dpred = _run(pred, truth)
    assert float(loss) == 0.0 and float(valid) == 0.0 and not sums.any() and not dpred.any()
    assert not torch.isnan(loss) and not torch.isnan(sums).any() and not torch.isnan(dpred).any()


def test_a_batch_with_one_valid_entry():
    pred, truth = make_inputs((3, 47, 24), seed=2, delta=DELTA, null_fraction=1.0)
    truth[2, 40, 17] = 123.0
    want = restate(pred, truth, DELTA, 0.0, MASK)
    assert want["valid"] == 1.0 and want["sums"][17, 0] == 1.0
    _check(_run(pred, truth), want, "one valid entry")


def test_nan_entries_of_the_truth_are_invalid_and_reach_nothing():
    pred, truth = make_inputs((3, 47, 24), seed=3, delta=DELTA, n_nan=40)
    assert int(torch.isnan(truth).sum()) == 40
    want = restate(pred, truth, DELTA, 0.0, MASK)
    got = _run(pred, truth)
    _check(got, want, "NaN entries, null 0")
    assert not torch.isnan(got[0]) and bool((got[3][torch.isnan(truth).to(_dev())] == 0).all())


def test_null_value_nan_masks_only_the_nan_entries():
    pred, truth = make_inputs((3, 47, 24), seed=4, delta=DELTA, n_nan=40)
    want = restate(pred, truth, DELTA, float("nan"), MASK)
    assert want["valid"] == truth.numel() - 40                  # the zeros count: |e| there is the whole prediction
    _check(_run(pred, truth, null_value=float("nan")), want, "null NaN")


def test_two_calls_on_the_same_input_give_the_same_bits():
    pred, truth = make_inputs((8, 1400, 12), seed=5, delta=DELTA, n_nan=7)
    a, b = _run(pred, truth), _run(pred, truth)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_two_batches_accumulate_into_one_totals_buffer():
    pred, truth = make_inputs((6, 47, 24), seed=6, delta=DELTA)
    sums = torch.zeros(25, 5, device=_dev(), dtype=torch.float64)
    for sl in (slice(0, 4), slice(4, 6)):
        _run(pred[sl], truth[sl], sums=sums)
    want = restate(pred, truth, DELTA, 0.0, MASK)["sums"]
    assert torch.equal(sums[:, 0].cpu(), want[:, 0])
    assert float(((sums.cpu() - want).abs() / want.abs()).max()) < 1e-5


def test_the_unmasked_op_is_unchanged_by_the_masked_one_running_in_the_same_process():
    from ms_gat_amd import ops
    pred, truth = make_inputs((3, 47, 24), seed=7, delta=DELTA)

    def plain():
        p = pred.to(_dev()).requires_grad_(True)
        sums = torch.zeros(4, device=_dev(), dtype=torch.float64)
        loss = ops.huber_metrics(p, truth.to(_dev()), DELTA, 0.0, sums)
        loss.backward()
        return loss.detach(), sums, p.grad

    before = plain()
    _run(pred, truth)
    after = plain()
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    # and it is the unmasked definition: every entry counts, zeros included
    err = (pred.double() - truth.double()).abs()
    want = torch.where(err <= DELTA, 0.5 * err * err, DELTA * err - 0.5 * DELTA * DELTA).mean()
    assert abs(float(before[0]) - float(want)) < 1e-6 * float(want)


def test_module_level_loss_on_the_device_is_the_masked_op():
    from ms_gat_amd import engine
    pred, truth = make_inputs((2, 19, 36), seed=8, delta=DELTA, n_nan=5)
    want = restate(pred, truth, DELTA, 0.0)
    p = pred.to(_dev()).requires_grad_(True)
    loss = engine.HuberLoss(DELTA, null_value=0.0)(p, truth.to(_dev()))
    loss.backward()
    assert abs(float(loss) - want["loss"]) < 1e-5 * want["loss"]
    r = want["dpred"]
    assert bool(((p.grad.double().cpu() - r).abs() <= 1e-5 * r.abs()).all())


# ---- engine -----------------------------------------------------------------------------------------------------------------
def _tiny_model_and_batches(n_batches, seed=0):
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
        y[torch.rand(y.shape, generator=g) < (0.1, 0.5, 0.3, 0.7)[i % 4]] = 0.0
        batches.append([*inputs, y])
    return net.to(_dev()), batches


def test_masked_training_steps_in_a_hip_graph_match_the_eager_steps(tmp_path):
    """Three training steps eager against three steps with hip_graph=True (captured at the first batch, replayed on
    batches with OTHER valid counts): the captured gradient kernel divides by the count of the replayed batch only if
    it reads it on the device.  Bars of test_hip_graph_training_matches_eager_training: losses 1e-4, parameters 2e-2."""
    from ms_gat_amd import engine
    net, batches = _tiny_model_and_batches(3)
    counts = [int((b[-1] != 0).sum()) for b in batches]
    assert len(set(counts)) == 3 and max(counts) > 1.5 * min(counts)
    twin = copy.deepcopy(net)
    eager = engine.Trainer(net, DELTA, str(tmp_path / "eager"), hip_graph=False, null_value=0.0)
    graphed = engine.Trainer(twin, DELTA, str(tmp_path / "graph"), hip_graph=True, null_value=0.0)
    for i, b in enumerate(batches):
        le = eager.run_epoch([b], gpu_id=0, epoch=i + 1, mode="train")
        lg = graphed.run_epoch([b], gpu_id=0, epoch=i + 1, mode="train")
        assert le > 0 and abs(le - lg) < 1e-4 * abs(le), (i, le, lg)
        # Adam's step hardly depends on the gradient's scale, so the parameters alone would not notice a stale count:
        # compare the gradient the update consumed.  A captured 1 / count of the first batch would be off by the ratio
        # of the counts (> 1.5 here); parameters that agree to 2e-2 keep the gradients well inside 5e-2.
        ge, gg = (t.optimizer.flat_grad[: t.optimizer.numel] for t in (eager, graphed))
        print(f"step {i}: valid {counts[i]} loss {le:.6f} / {lg:.6f} gradient rel err {rel_err(gg, ge):.2e}")
        assert rel_err(gg, ge) < 5e-2, (i, rel_err(gg, ge))
        assert eager.last_stats["horizons"]["valid"] == graphed.last_stats["horizons"]["valid"]
        assert sum(graphed.last_stats["horizons"]["valid"]) == counts[i]
    assert len(graphed._graphs) == 1
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name
    assert set(graphed.optimizer._host_steps) == set(eager.optimizer._host_steps) == {3}
    assert float(graphed._valid_count) == counts[-1]


def test_evaluator_reports_per_horizon_metrics_and_logs_them(tmp_path):
    from ms_gat_amd import engine
    net, batches = _tiny_model_and_batches(3, seed=1)
    ckpt = tmp_path / "net.pkl"
    torch.save(dict(model=net.state_dict()), ckpt)
    ev = engine.Evaluator(net, DELTA, str(tmp_path / "masked"), ckpt, hip_graph=False, null_value=0.0)
    loss = ev.eval(batches, gpu_id=0)
    net.eval()
    with torch.no_grad():
        pred = torch.cat([net(*[t.to(_dev()) for t in b[:-1]]) for b in batches])
    want = restate(pred, torch.cat([b[-1] for b in batches]), DELTA, 0.0)
    ref = metrics_of(want["sums"])
    got = ev.last_stats["horizons"]
    assert sorted(got) == ["MAE", "MAPE", "RMSE", "valid"] and got["valid"] == ref["valid"][:12]
    for k in ("MAE", "MAPE", "RMSE"):
        assert len(got[k]) == 12
        for a, b in zip(got[k], ref[k][:12]):
            assert abs(a - b) < 1e-5 * abs(b), (k, got[k], ref[k])
        assert abs(ev.last_stats[k] - ref[k][-1]) < 1e-5 * ref[k][-1]
    assert abs(loss - want["loss"]) < 1e-5 * want["loss"] and ev.last_stats["loss"] == loss
    lines = open(ev.log_file).read().splitlines()
    assert len(lines) == 2 and "per horizon" in lines[1] and "[Evaluate]" in lines[1] and "per horizon" not in lines[0]
    fields = dict(f.split("=") for f in lines[1].split("per horizon - ")[1].split(","))
    assert sorted(fields) == ["MAE", "MAPE", "RMSE"]
    for k, text in fields.items():
        assert [float(v) for v in text.split("/")] == pytest.approx(got[k], rel=1e-5)
    plain = engine.Evaluator(net, DELTA, str(tmp_path / "plain"), ckpt, hip_graph=False)
    plain.eval(batches, gpu_id=0)
    assert "horizons" not in plain.last_stats and sorted(plain.last_stats) == ["MAE", "MAPE", "RMSE", "loss"]
    lines = open(plain.log_file).read().splitlines()
    assert len(lines) == 1 and "per horizon" not in lines[0]
