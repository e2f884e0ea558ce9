"""CPU: quantile forecasts in the step tail -- the three entry points (`msgat_quantile_{partial_doubles,metrics,grad}`)
as declared, bound and refusing bad arguments before any launch; `QuantileLoss`, `engine.quantile_loss`, `Metrics` and
the engine on CPU tensors against the float64 restatement of tests/quantile_tail_ref.py."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from ms_gat_amd import QuantileLoss, engine
from quantile_tail_ref import dpred_fp32, make_inputs, point_of, restate

LEVELS = (0.1, 0.5, 0.9)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


_NEW = {"msgat_quantile_partial_doubles": 3, "msgat_quantile_metrics": 14, "msgat_quantile_grad": 11}


def test_quantile_entry_points_are_declared_exported_and_bound(built_library):
    import ms_gat_amd
    from ms_gat_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in _NEW.items():
        assert hasattr(h, name), name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.exported_symbols() and len(_lib._PROTOTYPES[name][1]) == n_args, name
    assert "const float* levels" in code and "int32_t point" in code
    assert re.search(r"#define MSGAT_ABI_VERSION 10\b", header) and _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10
    assert "QuantileLoss" in ms_gat_amd.__all__ and ms_gat_amd.QuantileLoss is engine.QuantileLoss


def _floats(*values):
    return (C.c_float * len(values))(*values)


def test_quantile_entry_points_report_bad_arguments_before_any_launch(built_library):
    from ms_gat_amd import _lib
    L = _lib.lib()
    x = C.cast(C.create_string_buffer(64), C.c_void_p)       # a non-NULL pointer; nothing is launched on these paths
    nan = float("nan")
    ok = _floats(*LEVELS)

    def metrics(rows=4, t=12, q=3, levels=ok, point=1, pred=x, valid=x):
        return L.msgat_quantile_metrics(pred, x, rows, t, q, levels, point, nan, 0.0, x, x, valid, None, None)

    def grad(rows=4, t=12, q=3, levels=ok, dpred=x):
        return L.msgat_quantile_grad(x, x, x, x, rows, t, q, levels, nan, dpred, None)

    assert metrics(pred=None) == -1 and metrics(valid=None) == -1 and metrics(levels=None) == -1
    assert grad(dpred=None) == -1 and grad(levels=None) == -1
    eight = _floats(*[0.1 * (i + 1) for i in range(8)])
    nine = _floats(*[0.1 * (i + 1) for i in range(9)])
    # limits: MSGAT_ERR_UNSUPPORTED
    for call in (metrics, grad):
        assert call(q=0) == -3
        assert call(q=9, t=1, levels=nine) == -3
        assert call(q=5, t=13, levels=eight) == -3                       # Q * T_out = 65
        assert call(q=1, t=65, levels=ok) == -3
        assert call(t=0) == -3
        assert call(rows=(1 << 24) // 12 + 1) == -3                      # rows * T_out > 2^24
        assert call(rows=-1) == -2
    # levels: MSGAT_ERR_SHAPE
    for bad in ((0.5, 0.5), (0.9, 0.1), (0.0, 0.5), (0.5, 1.0), (nan, 0.5), (0.5, nan), (-0.1, 0.5), (0.5, 1.5)):
        assert metrics(q=2, levels=_floats(*bad), point=0) == -2, bad
        assert grad(q=2, levels=_floats(*bad)) == -2, bad
    assert metrics(point=-1) == -2 and metrics(point=3) == -2
    assert L.msgat_quantile_partial_doubles(4, 12, 0) == 0 and L.msgat_quantile_partial_doubles(4, 12, 9) == 0
    assert L.msgat_quantile_partial_doubles(4, 13, 5) == 0 and L.msgat_quantile_partial_doubles(0, 12, 3) == 0
    assert L.msgat_quantile_partial_doubles((1 << 24) // 12 + 1, 12, 3) == 0
    # one record of [7 + 2Q][T_out] doubles per block; the block count is the masked tail's
    assert L.msgat_quantile_partial_doubles(21, 12, 3) == 13 * 12
    assert L.msgat_quantile_partial_doubles(4099, 12, 3) == 25 * 13 * 12
    assert L.msgat_quantile_partial_doubles(19, 8, 8) == 23 * 8
    assert L.msgat_quantile_partial_doubles(32 * 883, 12, 3) == L.msgat_masked_huber_partial_doubles(32 * 883, 12) // 5 * 13


def test_the_op_refuses_cpu_tensors_and_bad_arguments(built_library):
    from ms_gat_amd import ops
    pred, truth = torch.zeros(2, 3, 36), torch.zeros(2, 3, 12)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        ops.quantile_metrics(pred, truth, LEVELS)                         # the library has no CPU path
    for bad in ((), (0.5, 0.5), (0.9, 0.1), (0.0, 0.5), (0.5, 1.0), (float("nan"),), (0.99999999,), tuple([0.1] * 9), 0.5):
        with pytest.raises(ValueError):
            QuantileLoss(bad)
    assert QuantileLoss().levels == LEVELS and QuantileLoss().point == 1
    assert QuantileLoss((0.4, 0.6)).point == 0 and QuantileLoss((0.05, 0.25, 0.75, 0.95)).point == 1      # the lower on a tie
    assert QuantileLoss((0.9,)).point == 0
    ql = QuantileLoss()
    assert ql.split(pred).shape == (2, 3, 3, 12) and ql.point_forecast(pred).shape == (2, 3, 12)
    p = torch.arange(2 * 3 * 36.0).reshape(2, 3, 36)
    assert torch.equal(ql.point_forecast(p), p[..., 12:24]) and torch.equal(ql.split(p)[..., 2, :], p[..., 24:])
    with pytest.raises(ValueError):
        ql.split(torch.zeros(2, 3, 35))


# ---- QuantileLoss on CPU tensors ------------------------------------------------------------------------------------------------
CASES = [(21, 12, LEVELS, 0.0), (33, 5, (0.5,), 0.0), (19, 8, (0.05, 0.1, 0.25, 0.4, 0.6, 0.75, 0.9, 0.95), 0.0),
         (21, 12, LEVELS, None)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}q{len(c[2])}null{c[3]}")
def test_quantile_loss_and_metrics_on_cpu_tensors_match_the_restatement(case):
    rows, t_out, levels, null_value = case
    pred, truth = make_inputs(rows, t_out, levels, seed=rows + t_out, dead_horizon=2)
    want = restate(pred, truth, levels, null_value, mask_value=30.0)
    assert int(torch.isnan(truth).sum()) > 0 and 0 < want["valid"] < truth.numel()
    assert want["sums"][2, 0] == (0.0 if null_value is not None else float((~torch.isnan(truth[:, 2])).sum()))
    if len(levels) > 1:
        assert want["sums"][-1, 5] >= 5                                      # the planted crossings
    ql = QuantileLoss(levels, null_value=null_value)
    # float64: the definitions themselves
    assert float(ql(pred.double(), truth.double())) == pytest.approx(want["loss"], rel=1e-7)      # fp32 levels vs given
    assert float(engine.quantile_loss(pred.double(), truth.double(), ql.levels, null_value)) == float(ql(pred.double(), truth.double()))
    # fp32 tensors: two roundings per term
    p = pred.clone().requires_grad_(True)
    loss = ql(p, truth)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(want["loss"], rel=1e-5)
    ref = dpred_fp32(pred, truth, levels, null_value, want["valid"])
    assert torch.allclose(p.grad, ref, rtol=1e-6, atol=0.0) and not torch.isnan(p.grad).any()
    assert not p.grad[ref == 0].any() and int((ref != 0).sum()) == int(want["valid"]) * len(levels) - _half_ties(levels, pred, truth, null_value)
    # Metrics: every column
    m = engine.Metrics(mask_value=30.0, null_value=null_value, loss_fn=ql)
    m.update(pred, truth)
    assert tuple(m._sums.shape) == (t_out + 1, 7 + 2 * len(levels))
    counts = [0, 5] + list(range(7, 7 + len(levels)))
    assert torch.equal(m._sums[:, counts], want["sums"][:, counts])
    assert torch.allclose(m._sums, want["sums"], rtol=1e-7, atol=1e-7 * float(want["width_abs"][-1]))
    n = max(want["valid"], 1.0)
    assert m.MAE == pytest.approx(float(want["sums"][-1, 1]) / n) and m.loss == pytest.approx(want["loss"], rel=1e-7)
    assert m.RMSE == pytest.approx(math.sqrt(float(want["sums"][-1, 3]) / n)) and m.MAPE == pytest.approx(float(want["sums"][-1, 2]) / n)
    per = m.per_horizon()
    assert sorted(per) == ["MAE", "MAPE", "RMSE", "coverage", "crossing", "loss", "pinball", "valid", "width"]
    for k in ("MAE", "MAPE", "RMSE", "loss", "valid", "crossing", "width"):
        assert len(per[k]) == t_out, k
    for k in ("coverage", "pinball"):
        assert len(per[k]) == len(levels) and all(len(v) == t_out for v in per[k]), k
    hn = want["sums"][:t_out, 0].clamp(min=1.0)
    assert per["coverage"][0] == pytest.approx((want["sums"][:t_out, 7] / hn).tolist())
    assert per["pinball"][-1] == pytest.approx((want["sums"][:t_out, 6 + 2 * len(levels)] / hn).tolist())
    assert per["valid"][2] == want["sums"][2, 0] and (null_value is None or per["coverage"][0][2] == 0.0)
    assert m.at([1, t_out])["coverage"][0] == [per["coverage"][0][0], per["coverage"][0][-1]]
    s = m.quantile_summary()
    assert sorted(s) == ["coverage", "crossing", "levels", "pinball", "width"] and s["levels"] == list(ql.levels)
    assert s["coverage"] == pytest.approx((want["sums"][-1, 7:7 + len(levels)] / n).tolist())        # hits / valid
    assert s["pinball"] == pytest.approx((want["sums"][-1, 7 + len(levels):] / n).tolist())
    assert s["crossing"] == pytest.approx(float(want["sums"][-1, 5]) / n) and s["width"] == pytest.approx(float(want["sums"][-1, 6]) / n)
    assert sum(s["pinball"]) / len(levels) == pytest.approx(m.loss)
    # a second batch accumulates; reset() starts over on the same buffer
    m.update(pred, truth)
    assert torch.allclose(m._sums, 2 * want["sums"], rtol=1e-7, atol=2e-7 * float(want["width_abs"][-1]))
    buf = m._sums
    m.reset()
    assert m._sums is buf and not buf.any()


def _half_ties(levels, pred, truth, null_value):
    """Planted ties whose slope 1/2 - tau_q is zero (tau_q == 0.5): valid entries with a zero gradient."""
    q, t_out = len(levels), truth.shape[-1]
    p = pred.reshape(-1, q, t_out)
    return sum(int((p[:, i] == truth).sum()) for i, tau in enumerate(levels) if tau == 0.5)


def test_a_batch_without_a_valid_entry_gives_zero_loss_and_a_zero_gradient():
    pred, truth = make_inputs(21, 12, LEVELS, seed=3, nan_fraction=0.5, null_fraction=0.5)
    assert restate(pred, truth, LEVELS, 0.0)["valid"] == 0.0
    p = pred.clone().requires_grad_(True)
    loss = QuantileLoss(LEVELS, null_value=0.0)(p, truth)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not p.grad.any() and not torch.isnan(p.grad).any()
    m = engine.Metrics(loss_fn=QuantileLoss(LEVELS, null_value=0.0))
    m.update(pred, truth)
    assert not m._sums.any() and m.loss == 0.0 and m.quantile_summary()["coverage"] == [0.0, 0.0, 0.0]
    assert engine.Metrics(loss_fn=QuantileLoss()).quantile_summary()["width"] == 0.0          # before any batch
    with pytest.raises(ValueError):
        engine.Metrics(null_value=0.0).quantile_summary()


def test_one_level_at_one_half_is_half_the_masked_mean_absolute_error():
    pred, truth = make_inputs(33, 5, (0.5,), seed=4)
    valid = ~torch.isnan(truth) & (truth != 0.0)
    mae = float((pred.double() - truth.double())[valid].abs().mean())
    assert float(QuantileLoss((0.5,), null_value=0.0)(pred.double(), truth.double())) == pytest.approx(0.5 * mae, rel=1e-12)
    m = engine.Metrics(null_value=0.0, loss_fn=QuantileLoss((0.5,)))
    m.update(pred, truth)
    assert m.loss == pytest.approx(0.5 * m.MAE, rel=1e-12) and m.MAE == pytest.approx(mae, rel=1e-12)


def test_autograd_of_the_cpu_form_is_exactly_the_stated_slopes():
    """Dyadic levels and Q * valid = 256: every product below is exact in float64, so the comparison is `==`."""
    levels = (0.125, 0.25, 0.5, 0.875)
    g = torch.Generator().manual_seed(5)
    truth = torch.randint(20, 400, (8, 9), generator=g).double()
    truth[:, 8] = float("nan")                                           # 64 valid entries
    truth[0, 0] = float("nan")
    truth[0, 8] = 100.0
    pred = (truth.nan_to_num(50.0).unsqueeze(1) + torch.randint(-30, 31, (8, 4, 9), generator=g)).double()
    pred[1, :, 3] = truth[1, 3]                                          # a tie at every level
    p = pred.reshape(8, 36).clone().requires_grad_(True)
    engine.quantile_loss(p, truth, levels, None).backward()
    valid = ~torch.isnan(truth)
    assert int(valid.sum()) == 64
    y = truth.unsqueeze(1)
    tau = torch.tensor(levels, dtype=torch.float64).reshape(1, 4, 1)
    slope = torch.where(y > pred, -tau, torch.where(y < pred, 1.0 - tau, 0.5 - tau))
    want = torch.where(valid.unsqueeze(1), slope / 4.0 / 64.0, torch.zeros_like(pred))
    assert int((pred == y).sum()) >= 4 and bool((y > pred).any()) and bool((y < pred).any())
    assert torch.equal(p.grad.reshape(8, 4, 9), want)
    assert not p.grad.reshape(8, 4, 9)[0, :, 0].any() and not p.grad.reshape(8, 4, 9)[1:, :, 8].any()


def test_exact_empirical_quantiles_are_calibrated_within_one_count():
    """pred = the sample's own order statistics: the number of y <= p_q is ceil(tau_q n) by construction (continuous
    sample, no ties), so coverage differs from tau_q by less than 1 / valid.  A counting bound, not a measurement."""
    levels = (0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95)
    g = torch.Generator().manual_seed(6)
    n, t_out = 997, 3
    truth = (20.0 + 380.0 * torch.rand(n, t_out, generator=g)).float()
    truth[:50, 1] = float("nan")                                         # horizon 1 keeps 947 entries
    pred = torch.empty(n, len(levels), t_out)
    for t in range(t_out):
        col = truth[:, t][~torch.isnan(truth[:, t])].sort().values
        assert len(torch.unique(col)) == len(col)
        for i, tau in enumerate(levels):
            pred[:, i, t] = col[math.ceil(tau * len(col)) - 1]
    m = engine.Metrics(loss_fn=QuantileLoss(levels))
    m.update(pred.reshape(n, -1), truth)
    per = m.per_horizon()
    for t, count in enumerate((997, 947, 997)):
        assert per["valid"][t] == count
        for i, tau in enumerate(levels):
            assert 0.0 <= per["coverage"][i][t] - tau < 1.0 / count, (t, tau, per["coverage"][i][t])
    s = m.quantile_summary()
    valid = sum(per["valid"])
    for tau, cov in zip(levels, s["coverage"]):
        assert abs(cov - tau) < 3.0 / valid                                # one count per horizon
    assert s["crossing"] == 0.0 and s["width"] > 0.0


# ---- Engine --------------------------------------------------------------------------------------------------------------------
class _TinyQuantileMSGAT(torch.nn.Module):
    """CPU stand-in with the MSGAT call signature model(X, H, D) -> [B, N, Q * T_out]: the tiny model of
    test_gauss_tail_cpu.py with a head of Q * T_out outputs."""

    def __init__(self, n_levels=3, t_out=4):
        super().__init__()
        torch.manual_seed(3)
        self.mix = torch.nn.Conv2d(4, 1, 1)
        self.head = torch.nn.Linear(12, n_levels * t_out)

    def forward(self, X, H, D):
        B, R, C_, N, T = X.shape
        return self.head(self.mix(X.reshape(B, R * C_, N, T)).squeeze(1))


def _batches(n, t_out=4):
    g = torch.Generator().manual_seed(11)
    out = []
    for i in range(n):
        y = 100.0 + 30.0 * torch.randn(8, 5, t_out, generator=g)
        y[torch.rand(y.shape, generator=g) < 0.1 * (i + 1)] = float("nan")
        out.append((torch.randn(8, 2, 2, 5, 12, generator=g) * 40, torch.zeros(8, dtype=torch.long),
                    torch.zeros(8, dtype=torch.long), y))
    return out


def test_trainer_with_a_quantile_loss_lowers_the_pinball_loss_and_reports_the_quantiles(tmp_path):
    batches = _batches(3)
    model = _TinyQuantileMSGAT()
    tr = engine.Trainer(model, 50.0, str(tmp_path / "q"), loss=QuantileLoss(LEVELS))
    assert isinstance(tr.loss_fn, QuantileLoss) and math.isnan(tr.null_value)       # None runs as NaN
    first = tr.run_epoch(batches, epoch=1, mode="train")
    assert sorted(tr.last_stats) == ["MAE", "MAPE", "RMSE", "horizons", "loss", "quantiles"]
    second = tr.run_epoch(batches, epoch=2, mode="train")
    assert 0.0 < second < first
    n_lines = len(open(tr.log_file).read().splitlines())
    loss = tr.run_epoch(batches, epoch=2, mode="validate")
    with torch.no_grad():
        pred = torch.cat([model(*b[:3]) for b in batches])
    want = restate(pred, torch.cat([b[3] for b in batches]), LEVELS, None)
    n = want["valid"]
    assert 0 < n < 3 * 8 * 5 * 4 and loss == pytest.approx(want["loss"], rel=1e-6)
    q = tr.last_stats["quantiles"]
    assert q["levels"] == list(LEVELS)
    assert q["coverage"] == pytest.approx((want["sums"][-1, 7:10] / n).tolist(), rel=1e-12)
    assert q["pinball"] == pytest.approx((want["sums"][-1, 10:13] / n).tolist(), rel=1e-6)
    assert q["width"] == pytest.approx(float(want["sums"][-1, 6]) / n, rel=1e-6, abs=1e-6 * float(want["width_abs"][-1]) / n)
    assert q["crossing"] == float(want["sums"][-1, 5]) / n
    per = tr.last_stats["horizons"]
    assert per["valid"] == want["sums"][:4, 0].tolist() and len(per["coverage"]) == 3 and len(per["coverage"][0]) == 4
    assert tr.last_stats["MAE"] == pytest.approx(float(want["sums"][-1, 1]) / n, rel=1e-6)
    lines = open(tr.log_file).read().splitlines()[n_lines:]
    assert len(lines) == 3 and "per horizon" in lines[1] and "quantiles" in lines[2] and "coverage=" in lines[2]
    # evaluation: the same line without an epoch
    ckpt = tmp_path / "net.pkl"
    torch.save(dict(model=model.state_dict()), ckpt)
    ev = engine.Evaluator(_TinyQuantileMSGAT(), 50.0, str(tmp_path / "e"), ckpt, loss=QuantileLoss(LEVELS))
    assert ev.eval(batches) == pytest.approx(loss, rel=1e-12) and ev.last_stats["quantiles"] == q
    assert "quantiles" in open(ev.log_file).read().splitlines()[-1]


def test_engine_refuses_a_width_mismatch_and_foreign_losses_and_leaves_the_other_losses_alone(tmp_path):
    batches = _batches(1)
    tr = engine.Trainer(_TinyQuantileMSGAT(n_levels=2), 50.0, str(tmp_path / "a"), loss=QuantileLoss(LEVELS))
    with pytest.raises(ValueError, match=r"(?s)12.*8|8.*12"):                 # 3 x 4 = 12 outputs wanted, 8 given
        tr.run_epoch(batches, epoch=1, mode="train")
    with pytest.raises(ValueError):
        QuantileLoss(LEVELS)(torch.zeros(2, 5, 8), torch.zeros(2, 5, 4))
    for foreign in (torch.nn.MSELoss(), torch.nn.HuberLoss(), lambda a, b: (a - b).abs().mean(), "quantile", torch.nn.L1Loss()):
        with pytest.raises(TypeError):
            engine.Trainer(_TinyQuantileMSGAT(), 7.0, str(tmp_path / "b"), loss=foreign)
    # the engine's null_value reaches the loss; two different ones are refused
    tr = engine.Trainer(_TinyQuantileMSGAT(), 7.0, str(tmp_path / "c"), null_value=0.0, loss=QuantileLoss(LEVELS))
    assert tr.null_value == 0.0 and tr.loss_fn.null_value == 0.0
    with pytest.raises(ValueError):
        engine.Trainer(_TinyQuantileMSGAT(), 7.0, str(tmp_path / "d"), null_value=0.0, loss=QuantileLoss(LEVELS, null_value=-1.0))
    # a Huber engine: no "quantiles" anywhere
    y_batches = [(b[0], b[1], b[2], b[3].nan_to_num(0.0)) for b in batches]
    hub = engine.Trainer(_TinyQuantileMSGAT(n_levels=1), 50.0, str(tmp_path / "h"), null_value=0.0)
    hub.run_epoch(y_batches, epoch=1, mode="validate")
    assert "quantiles" not in hub.last_stats and "quantiles" not in open(hub.log_file).read()
    assert sorted(hub.last_stats["horizons"]) == ["MAE", "MAPE", "RMSE", "valid"]
