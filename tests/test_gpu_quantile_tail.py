"""GPU: quantile forecasts in the step tail -- `msgat_quantile_metrics` / `msgat_quantile_grad` through
`ops.quantile_metrics` and `QuantileLoss`, and the engine on top of them (eager and captured steps).  Yardstick: the
float64 restatement of tests/quantile_tail_ref.py.

Bars.  Counts (valid, hits, crossing) are exact.  Loss and the sum columns: 1e-6 relative -- every term is non-negative and
carries at most two fp32 roundings (u = y - p and the product; e and e / y; e and its square), so a term is within 1.2e-7
relative, the fp64 sum keeps that and the final fp32 cast of the loss adds 6e-8.  The width column is a signed sum of
terms with one rounding each: it is compared at 1e-6 * sum |p_{Q-1} - p_0|.  dpred is bit-equal to the fp32 torch
expression c_q * (dloss / max(valid, 1)) with the same c_q, and exactly +0 at the entries that are not valid."""
import copy

import pytest
import torch

from conftest import record_err, rel_err
from quantile_tail_ref import dpred_fp32, make_inputs, restate

pytestmark = pytest.mark.gpu

MASK = 30.0
LEVELS3 = (0.1, 0.5, 0.9)
LEVELS8 = (0.05, 0.1, 0.25, 0.4, 0.6, 0.75, 0.9, 0.95)
# one block; several blocks with a ragged last trip; lanes no power of two (255 of 256); Q * T_out = 64 and all 23 columns;
# T_out at its limit
SHAPES = [(21, 12, LEVELS3), (4099, 12, LEVELS3), (33, 5, (0.5,)), (19, 8, LEVELS8), (7, 64, (0.3,))]


def _dev():
    return torch.device("cuda:0")


def _ids(s):
    return f"{s[0]}x{s[1]}q{len(s[2])}"


def _run(pred, truth, levels, null_value=0.0, sums="new", dloss=None):
    """-> loss (0-dim), valid [1], sums [T_out + 1, 7 + 2Q] (None when run without), dpred; all on the device."""
    from ms_gat_amd import ops
    p = pred.to(_dev()).requires_grad_(True)
    if isinstance(sums, str):
        sums = torch.zeros(truth.shape[-1] + 1, 7 + 2 * len(levels), device=_dev(), dtype=torch.float64)
    valid = torch.full((1,), -1.0, device=_dev())
    loss = ops.quantile_metrics(p, truth.to(_dev()), levels, null_value, MASK, sums, valid)
    (loss if dloss is None else loss * dloss).backward()
    return loss.detach(), valid, sums, p.grad


@pytest.fixture(scope="module")
def cases():
    """Inputs and their restatement, computed once: 10 % NaN and 10 % zeros under null_value = 0, horizon 1 wholly
    invalid, exact ties and crossings planted."""
    out = {}
    for rows, t_out, levels in SHAPES:
        pred, truth = make_inputs(rows, t_out, levels, seed=rows + t_out, dead_horizon=1 if t_out > 1 else None, n_ties=6)
        out[(rows, t_out, levels)] = (pred, truth, restate(pred, truth, levels, 0.0, MASK))
    return out


def _check(what, got, want, levels):
    loss, valid, sums, _ = got
    q = len(levels)
    s = sums.cpu()
    counts = [0, 5] + list(range(7, 7 + q))
    assert float(valid) == want["valid"] and torch.equal(s[:, counts], want["sums"][:, counts]), what       # exact
    e_loss = abs(float(loss) - want["loss"]) / max(abs(want["loss"]), 1e-300)
    positive = [1, 2, 3, 4] + list(range(7 + q, 7 + 2 * q))
    w = want["sums"][:, positive]
    e_sums = float(((s[:, positive] - w).abs() / w.abs().clamp(min=1e-300)).max())
    e_width = float(((s[:, 6] - want["sums"][:, 6]).abs() / want["width_abs"].clamp(min=1e-300)).max())
    print(f"{what}: loss {e_loss:.2e} sums {e_sums:.2e} width {e_width:.2e} (of sum |w|)")
    for key, err in (("loss", e_loss), ("sums", e_sums), ("width / sum |w|", e_width)):
        record_err(f"quantile tail {what}", key, err, 1e-6)
    assert e_loss < 1e-6 and e_sums < 1e-6 and e_width < 1e-6, what
    assert not torch.isnan(s).any()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_loss_valid_totals_and_gradient_match_the_yardstick(cases, shape):
    rows, t_out, levels = shape
    pred, truth, want = cases[shape]
    assert int(torch.isnan(truth).sum()) > 0 and int((truth == 0).sum()) > 0 and 0 < want["valid"] < truth.numel()
    if t_out > 1:
        assert want["sums"][1, 0] == 0.0                                    # a horizon without a valid entry
    if len(levels) > 1:
        assert want["sums"][-1, 5] >= 5                                     # the planted crossings
    p3 = pred.reshape(rows, len(levels), t_out)
    assert int(((p3 == truth.unsqueeze(1)) & (truth != 0).unsqueeze(1)).sum()) >= 6       # the planted ties
    got = _run(pred, truth, levels, dloss=0.75)
    _check(f"{_ids(shape)}", got, want, levels)
    dpred = got[3].cpu()
    ref = dpred_fp32(pred, truth, levels, 0.0, want["valid"], dloss=0.75)
    assert torch.equal(dpred, ref), f"{int((dpred != ref).sum())} entries differ"            # bit for bit
    dead = (torch.isnan(truth) | (truth == 0)).unsqueeze(1).expand(rows, len(levels), t_out).reshape(rows, -1)
    assert not dpred[dead].any() and not torch.signbit(dpred[dead]).any() and not torch.isnan(dpred).any()
    assert int((dpred != 0).sum()) > 0


def test_nan_alone_is_masked_without_a_null_value(cases):
    pred, truth, _ = cases[SHAPES[0]]
    want = restate(pred, truth, LEVELS3, None, MASK)
    assert want["valid"] == float((~torch.isnan(truth)).sum())               # the zeros count now
    got = _run(pred, truth, LEVELS3, null_value=None)
    _check("null_value None", got, want, LEVELS3)
    assert torch.equal(got[3].cpu(), dpred_fp32(pred, truth, LEVELS3, None, want["valid"]))


def test_another_point_level_moves_only_the_point_columns(cases):
    from ms_gat_amd import ops
    pred, truth, want = cases[SHAPES[0]]
    sums = torch.zeros(13, 13, device=_dev(), dtype=torch.float64)
    ops.quantile_metrics(pred.to(_dev()), truth.to(_dev()), LEVELS3, 0.0, MASK, sums, None, point=2)
    other = restate(pred, truth, LEVELS3, 0.0, MASK, point=2)
    s = sums.cpu()
    assert float(((s[:, 1:4] - other["sums"][:, 1:4]).abs() / other["sums"][:, 1:4].clamp(min=1e-300)).max()) < 1e-6
    assert not torch.allclose(s[:, 1], want["sums"][:, 1], rtol=1e-3)
    assert torch.equal(s[:, [0, 5, 7, 8, 9]], want["sums"][:, [0, 5, 7, 8, 9]])


def test_a_batch_without_a_valid_entry_gives_zero_loss_and_a_positive_zero_gradient():
    pred, truth = make_inputs(4099, 12, LEVELS3, seed=2, nan_fraction=0.5, null_fraction=0.5)
    loss, valid, sums, dpred = _run(pred, truth, LEVELS3)
    assert float(loss) == 0.0 and float(valid) == 0.0 and not sums.any() and not dpred.any()
    assert not torch.signbit(dpred).any() and not torch.isnan(loss) and not torch.isnan(sums).any()


def test_zero_rows_give_zero_loss_and_valid_and_leave_the_totals_alone():
    """rows = 0 through the C ABI (the op refuses an empty batch before it gets there): MSGAT_OK, loss 0, valid 0."""
    import ctypes as C
    from ms_gat_amd import _lib
    L = _lib.lib()
    x = torch.zeros(36, device=_dev())
    loss, valid = torch.full((), -1.0, device=_dev()), torch.full((1,), -1.0, device=_dev())
    sums = torch.full((13, 13), 2.0, device=_dev(), dtype=torch.float64)
    part = torch.zeros(1, device=_dev(), dtype=torch.float64)
    levels = (C.c_float * 3)(*LEVELS3)
    stream = _lib.stream_handle(_dev())
    assert L.msgat_quantile_metrics(x.data_ptr(), x.data_ptr(), 0, 12, 3, levels, 1, 0.0, MASK, part.data_ptr(), loss.data_ptr(),
                                    valid.data_ptr(), sums.data_ptr(), stream) == 0
    assert L.msgat_quantile_grad(x.data_ptr(), x.data_ptr(), loss.data_ptr(), valid.data_ptr(), 0, 12, 3, levels, 0.0,
                                 x.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and float(valid) == 0.0 and bool((sums == 2.0).all()) and not x.any()
    assert not torch.signbit(loss) and not torch.signbit(valid).any()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_ids)
def test_two_runs_give_the_same_bits_and_a_second_run_doubles_the_totals(cases, shape):
    pred, truth, _ = cases[shape]
    levels = shape[2]
    a, b = _run(pred, truth, levels), _run(pred, truth, levels)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    again = _run(pred, truth, levels, sums=a[2].clone())
    assert torch.equal(again[2], 2.0 * a[2])                                 # x + x is exact


def test_running_without_totals_gives_the_same_loss_and_gradient(cases):
    pred, truth, _ = cases[SHAPES[1]]
    with_sums, without = _run(pred, truth, LEVELS3), _run(pred, truth, LEVELS3, sums=None)
    assert without[2] is None
    for i in (0, 1, 3):
        assert torch.equal(with_sums[i], without[i])


def test_quantile_loss_on_device_tensors_is_the_op(cases):
    from ms_gat_amd import QuantileLoss, ops
    pred, truth, want = cases[SHAPES[0]]
    y = truth.to(_dev())
    a, b = (pred.to(_dev()).requires_grad_(True) for _ in range(2))
    la, lb = QuantileLoss(LEVELS3, null_value=0.0)(a, y), ops.quantile_metrics(b, y, LEVELS3, 0.0)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad) and float(la.detach()) > 0
    # [..., Q, T_out] and [B, N, Q * T_out] are the same forecast
    c = pred.reshape(3, 7, 3, 12).to(_dev())
    assert torch.equal(ops.quantile_metrics(c, truth.reshape(3, 7, 12).to(_dev()), LEVELS3, 0.0), lb.detach())
    with pytest.raises(ValueError):
        ops.quantile_metrics(pred[:, :24].to(_dev()), y, LEVELS3, 0.0)
    with pytest.raises(ValueError):
        ops.quantile_metrics(pred.to(_dev()), y, LEVELS3, 0.0, sums=torch.zeros(13, 5, device=_dev(), dtype=torch.float64))


# ---- engine -----------------------------------------------------------------------------------------------------------------
def _tiny_model_and_batches(n_batches, seed=0):
    """A small msgat48 (N = 24, B = 4) with a head of 3 x 12 outputs and batches of 12-step truths with zeros -- a
    different share in every batch, so the valid counts of replayed batches differ."""
    from ms_gat_amd import data, model
    torch.manual_seed(seed)
    ds = data.SyntheticPEMS(n_nodes=24, n_edges=30, n_channels=1, in_hours=[1, 2], batch_size=4, days=2)
    net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=36, use_te=True, adj=ds.adj)
    g = torch.Generator().manual_seed(seed + 1)
    batches = []
    for i, b in zip(range(n_batches), ds.training):
        *inputs, y = b
        y = y.clone()
        y[torch.rand(y.shape, generator=g) < (0.1, 0.5, 0.3)[i % 3]] = 0.0
        batches.append([*inputs, y])
    assert len(batches) == n_batches and batches[0][-1].shape == (4, 24, 12)
    return net.to(_dev()), batches


def test_training_steps_with_a_quantile_loss_in_a_hip_graph_match_the_eager_steps(tmp_path):
    """Three training steps eager against three with hip_graph=True (captured at the first batch, replayed on the
    others).  Bars of test_training_steps_with_a_gauss_loss_in_a_hip_graph_match_the_eager_steps: losses 1e-4, gradients
    5e-2, parameters 2e-2."""
    from ms_gat_amd import QuantileLoss, engine
    net, batches = _tiny_model_and_batches(3)
    twin = copy.deepcopy(net)
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False, loss=QuantileLoss(LEVELS3, null_value=0.0))
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True, loss=QuantileLoss(LEVELS3, null_value=0.0))
    assert eager.null_value == 0.0
    for i, b in enumerate(batches):
        le = eager.run_epoch([b], gpu_id=0, epoch=i + 1, mode="train")
        lg = graphed.run_epoch([b], gpu_id=0, epoch=i + 1, mode="train")
        ge, gg = (t.optimizer.flat_grad[: t.optimizer.numel] for t in (eager, graphed))
        print(f"step {i}: loss {le:.6f} / {lg:.6f} gradient rel err {rel_err(gg, ge):.2e}")
        assert le > 0 and abs(le - lg) < 1e-4 * abs(le), (i, le, lg)
        assert rel_err(gg, ge) < 5e-2, (i, rel_err(gg, ge))     # a stale valid count would be off by the counts' ratio
        assert eager.last_stats["horizons"]["valid"] == graphed.last_stats["horizons"]["valid"]
        assert sum(graphed.last_stats["horizons"]["valid"]) == int((b[-1] != 0).sum())
        qe, qg = eager.last_stats["quantiles"], graphed.last_stats["quantiles"]
        assert qg["pinball"] == pytest.approx(qe["pinball"], rel=1e-4) and qg["levels"] == list(LEVELS3)
    assert len(graphed._graphs) == 1
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name
    assert set(graphed.optimizer._host_steps) == set(eager.optimizer._host_steps) == {3}


@pytest.mark.parametrize("hip_graph", [False, "auto"], ids=["eager", "auto"])
def test_the_epoch_statistics_equal_a_float64_recomputation_from_the_predictions(tmp_path, hip_graph):
    from ms_gat_amd import QuantileLoss, engine
    net, batches = _tiny_model_and_batches(3, seed=1)
    ckpt = tmp_path / "net.pkl"
    torch.save(dict(model=net.state_dict()), ckpt)
    ev = engine.Evaluator(net, 50.0, str(tmp_path / "q"), ckpt, hip_graph=hip_graph, loss=QuantileLoss(LEVELS3, null_value=0.0))
    loss = ev.eval(batches, gpu_id=0)
    net.eval()
    with torch.no_grad():
        pred = torch.cat([net(*[t.to(_dev()) for t in b[:-1]]) for b in batches])
    assert pred.shape == (12, 24, 36)
    want = restate(pred, torch.cat([b[-1] for b in batches]), LEVELS3, 0.0)
    n = want["valid"]
    q = ev.last_stats["quantiles"]
    assert q["levels"] == list(LEVELS3) and q["coverage"] == (want["sums"][-1, 7:10] / n).tolist()          # counts: exact
    assert q["crossing"] == float(want["sums"][-1, 5]) / n
    assert q["pinball"] == pytest.approx((want["sums"][-1, 10:13] / n).tolist(), rel=1e-5)
    assert abs(q["width"] - float(want["sums"][-1, 6]) / n) <= 1e-5 * float(want["width_abs"][-1]) / n
    assert abs(loss - want["loss"]) < 1e-5 * want["loss"] and ev.last_stats["loss"] == loss
    per = ev.last_stats["horizons"]
    assert per["valid"] == want["sums"][:12, 0].tolist()
    hn = want["sums"][:12, 0].clamp(min=1.0)
    assert per["coverage"][2] == (want["sums"][:12, 9] / hn).tolist()
    assert per["MAE"] == pytest.approx((want["sums"][:12, 1] / hn).tolist(), rel=1e-5)
    assert "quantiles" in open(ev.log_file).read().splitlines()[-1]
