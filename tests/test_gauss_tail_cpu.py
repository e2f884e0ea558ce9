"""Host side of the Gauss loss in the step tail: the yardstick of tests/gauss_tail_ref.py and the torch path of
`GaussLoss` against what the reference computed (tests/golden/gauss_loss_ref.npz), the C-ABI entry points and their
argument checks, and `Trainer(loss=...)` / `Metrics(loss_fn=...)` on CPU tensors.  No device compute is called here."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
from gauss_tail_ref import make_inputs, restate

N_CASES = 4


@pytest.fixture(scope="module")
def golden():
    z = load_golden("gauss_loss_ref.npz")
    cases = []
    for i in range(N_CASES):
        sigma, delta = (float(v) for v in z[f"{i}.sigma_delta"])
        cases.append(dict(pred=torch.from_numpy(z[f"{i}.pred"]), truth=torch.from_numpy(z[f"{i}.truth"]), sigma=sigma,
                          delta=delta, loss=float(z[f"{i}.loss"]), dpred=torch.from_numpy(z[f"{i}.dpred"])))
    return cases


def _same(got, want, rel=1e-12):
    """Every entry within `rel` of the fixture's; its exact zeros exactly."""
    got, want = got.double(), want.double()
    assert bool(((got - want).abs() <= rel * want.abs()).all()), float(((got - want).abs() / want.abs().clamp(min=1e-300)).max())


def test_the_fixture_holds_the_issues_cases(golden):
    assert [tuple(c["pred"].shape) for c in golden] == [(2, 23, 12), (2, 23, 12), (2, 23, 12), (3, 7, 1)]
    assert [(c["sigma"], c["delta"]) for c in golden] == [(1.0, 0.05), (20.0, 0.5), (1.0, 0.0), (1.0, 0.0)]
    assert torch.equal(golden[0]["pred"], golden[1]["pred"]) and torch.equal(golden[0]["truth"], golden[1]["truth"])
    err = [(c["pred"].double() - c["truth"].double()).abs() for c in golden]
    assert 10 < float(err[0].mean()) < 50 and 1e-4 < float(err[2].mean()) < 1e-2 and 1 < float(err[3].mean()) < 8
    assert int((err[3] == 0).sum()) == 5 and int((golden[3]["dpred"] == 0).sum()) == 5
    for c in golden:
        assert c["pred"].dtype == torch.float32 and c["dpred"].dtype == torch.float64 and c["loss"] > 0


def test_the_yardstick_reproduces_the_reference(golden):
    for c in golden:
        want = restate(c["pred"], c["truth"], c["sigma"], c["delta"])
        assert want["valid"] == c["pred"].numel()
        assert want["loss"] == pytest.approx(c["loss"], rel=1e-12, abs=0.0)
        _same(want["dpred"], c["dpred"])
        # with a null value no entry has (NaN), the masked definitions are the plain ones
        masked = restate(c["pred"], c["truth"], c["sigma"], c["delta"], null_value=float("nan"))
        assert masked["loss"] == want["loss"] and torch.equal(masked["dpred"], want["dpred"])
        t_out = c["pred"].shape[-1]
        assert tuple(want["sums"].shape) == (t_out + 1, 5)
        assert float(want["sums"][-1, 4]) == pytest.approx(c["loss"] * c["pred"].numel(), rel=1e-12)


def test_gauss_loss_and_masked_gauss_loss_in_float64_reproduce_the_reference(golden):
    from ms_gat_amd import engine
    for c in golden:
        for fn in (lambda p, y: engine.gauss_loss(p, y, c["sigma"], c["delta"]),
                   lambda p, y: engine.masked_gauss_loss(p, y, c["sigma"], c["delta"], float("nan")),
                   engine.GaussLoss(c["sigma"], c["delta"])):
            p = c["pred"].double().requires_grad_(True)
            loss = fn(p, c["truth"].double())
            loss.backward()
            assert float(loss.detach()) == pytest.approx(c["loss"], rel=1e-12, abs=0.0)
            _same(p.grad, c["dpred"])


def test_masked_gauss_loss_on_cpu_tensors_matches_the_yardstick():
    from ms_gat_amd import engine
    pred, truth = make_inputs((4, 9, 12), seed=0, scale=4.0, null_fraction=0.2, n_nan=3, n_equal=4)
    want = restate(pred, truth, 2.0, 0.1, null_value=0.0)
    assert 0 < want["valid"] < truth.numel() - 3
    p = pred.double().requires_grad_(True)
    loss = engine.GaussLoss(2.0, 0.1, null_value=0.0)(p, truth.double())
    loss.backward()
    assert float(loss.detach()) == pytest.approx(want["loss"], rel=1e-12)
    _same(p.grad, want["dpred"])
    invalid = torch.isnan(truth) | (truth == 0.0)
    assert not torch.isnan(p.grad).any() and bool((p.grad[invalid] == 0).all())
    # fp32 tensors, what a CPU model trains with: the same numbers to fp32 rounding
    q = pred.clone().requires_grad_(True)
    loss32 = engine.GaussLoss(2.0, 0.1, null_value=0.0)(q, truth)
    loss32.backward()
    assert float(loss32.detach()) == pytest.approx(want["loss"], rel=1e-5)
    assert bool(((q.grad.double() - want["dpred"]).abs() <= 1e-5 * want["dpred"].abs() + 1e-7 * want["dpred"].abs().max()).all())
    # nothing valid: 0 with a zero gradient
    z = torch.randn(2, 3, 4, requires_grad=True)
    empty = engine.GaussLoss(null_value=0.0)(z, torch.zeros(2, 3, 4))
    empty.backward()
    assert float(empty.detach()) == 0.0 and not z.grad.any()


def test_gauss_loss_module_has_the_reference_defaults_and_repr():
    from ms_gat_amd import GaussLoss, engine
    m = GaussLoss()
    assert (m.sigma, m.delta, m.null_value) == (1.0, 5e-2, None) and m.extra_repr() == "sigma=1.0, delta=0.05"
    assert repr(m) == "GaussLoss(sigma=1.0, delta=0.05)" and not list(m.state_dict())
    assert GaussLoss(3.0, 0.0).delta == 0.0                     # delta = 0: the saturating term alone
    for bad in ((0.0, 0.1), (-1.0, 0.1), (float("nan"), 0.1), (float("inf"), 0.1), (1.0, -0.1), (1.0, float("nan")),
                (1.0, float("inf"))):
        with pytest.raises(ValueError):
            engine.GaussLoss(*bad)


def test_the_ops_refuse_bad_parameters_and_cpu_tensors():
    from ms_gat_amd import _lib, ops
    x = torch.zeros(2, 3, 4)
    for bad in ((0.0, 0.1), (-1.0, 0.1), (float("nan"), 0.1), (float("inf"), 0.1), (1.0, -0.1), (1.0, float("nan"))):
        with pytest.raises(ValueError):
            ops.gauss_metrics(x, x, *bad)
        with pytest.raises(ValueError):
            ops.masked_gauss_metrics(x, x, *bad, 0.0)
    with pytest.raises(_lib.MsgatError):
        ops.gauss_metrics(x, x, 1.0, 0.05)
    with pytest.raises(_lib.MsgatError):
        ops.masked_gauss_metrics(x, x, 1.0, 0.05, 0.0)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


_NEW = {"msgat_gauss_metrics": 11, "msgat_gauss_grad": 8, "msgat_masked_gauss_metrics": 13, "msgat_masked_gauss_grad": 11}


def test_gauss_entry_points_are_declared_exported_and_bound(built_library):
    from ms_gat_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in _NEW.items():
        assert hasattr(h, name), name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name
        assert "float sigma, float delta" in " ".join(decl.group(1).split()), name      # sigma in front of delta
        assert len(_lib._PROTOTYPES[name][1]) == n_args, name
        # the Huber twin's arguments plus one float
        twin = _lib._PROTOTYPES[name.replace("gauss", "huber")][1]
        assert len(twin) == n_args - 1 and _lib._PROTOTYPES[name][1].count(C.c_float) == twin.count(C.c_float) + 1
    assert re.search(r"#define MSGAT_ABI_VERSION 10\b", header) and _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10
    assert "loss.py:55-95" in header and "msgat_gauss_{metrics,grad} and msgat_masked_gauss_{metrics,grad}" in header


def test_gauss_entry_points_report_bad_arguments_before_any_launch(built_library):
    from ms_gat_amd import _lib
    L = _lib.lib()
    x = C.cast(C.create_string_buffer(64), C.c_void_p)       # a non-NULL pointer; nothing is launched on these paths
    nan, inf = float("nan"), float("inf")
    ok = (1.0, 0.05)
    assert L.msgat_gauss_metrics(None, x, 4, *ok, 0.0, x, x, None, 1.0, None) == -1
    assert L.msgat_gauss_metrics(x, None, 4, *ok, 0.0, x, x, None, 1.0, None) == -1
    assert L.msgat_gauss_metrics(x, x, 4, *ok, 0.0, None, x, None, 1.0, None) == -1
    assert L.msgat_gauss_metrics(x, x, 4, *ok, 0.0, x, None, None, 1.0, None) == -1
    assert L.msgat_gauss_metrics(x, x, 0, *ok, 0.0, x, x, None, 1.0, None) == -2
    assert L.msgat_gauss_grad(x, x, None, 4, *ok, x, None) == -1
    assert L.msgat_gauss_grad(x, x, x, 4, *ok, None, None) == -1
    assert L.msgat_gauss_grad(x, x, x, -3, *ok, x, None) == -2
    assert L.msgat_masked_gauss_metrics(None, x, 4, 3, *ok, 0.0, 0.0, x, x, x, None, None) == -1
    assert L.msgat_masked_gauss_metrics(x, x, 4, 3, *ok, 0.0, 0.0, x, x, None, None, None) == -1     # valid is required
    assert L.msgat_masked_gauss_metrics(x, x, 0, 3, *ok, 0.0, 0.0, x, x, x, None, None) == -2
    assert L.msgat_masked_gauss_metrics(x, x, 4, 0, *ok, 0.0, 0.0, x, x, x, None, None) == -2
    assert L.msgat_masked_gauss_metrics(x, x, 4, 65, *ok, 0.0, 0.0, x, x, x, None, None) == -3
    assert L.msgat_masked_gauss_metrics(x, x, (1 << 24) // 64 + 1, 64, *ok, 0.0, 0.0, x, x, x, None, None) == -3
    assert L.msgat_masked_gauss_grad(x, x, x, None, 4, 3, *ok, 0.0, x, None) == -1
    assert L.msgat_masked_gauss_grad(x, x, x, x, 4, 3, *ok, 0.0, None, None) == -1
    assert L.msgat_masked_gauss_grad(x, x, x, x, -1, 3, *ok, 0.0, x, None) == -2
    assert L.msgat_masked_gauss_grad(x, x, x, x, 4, 65, *ok, 0.0, x, None) == -3
    for sigma, delta in ((0.0, 0.05), (-1.0, 0.05), (nan, 0.05), (inf, 0.05), (1.0, -0.05), (1.0, nan), (1.0, inf)):
        assert L.msgat_gauss_metrics(x, x, 4, sigma, delta, 0.0, x, x, None, 1.0, None) == -2, (sigma, delta)
        assert L.msgat_gauss_grad(x, x, x, 4, sigma, delta, x, None) == -2, (sigma, delta)
        assert L.msgat_masked_gauss_metrics(x, x, 4, 3, sigma, delta, 0.0, 0.0, x, x, x, None, None) == -2, (sigma, delta)
        assert L.msgat_masked_gauss_grad(x, x, x, x, 4, 3, sigma, delta, 0.0, x, None) == -2, (sigma, delta)


# ---- Trainer(loss=...) on CPU tensors ---------------------------------------------------------------------------------------
class _TinyMSGAT(torch.nn.Module):
    """CPU stand-in with the MSGAT call signature model(X, H, D) -> [B,N,T]."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.mix = torch.nn.Conv2d(4, 1, 1)

    def forward(self, X, H, D):
        B, R, C_, N, T = X.shape
        return self.mix(X.reshape(B, R * C_, N, T)).squeeze(1)


def _batches(n, null_fraction=0.0):
    g = torch.Generator().manual_seed(11)
    out = []
    for i in range(n):
        y = 100.0 + 30.0 * torch.randn(8, 5, 12, generator=g)
        if null_fraction:
            y[torch.rand(y.shape, generator=g) < null_fraction * (i + 1)] = 0.0
        out.append((torch.randn(8, 2, 2, 5, 12, generator=g) * 40, torch.zeros(8, dtype=torch.long),
                    torch.zeros(8, dtype=torch.long), y))
    return out


def test_trainer_with_a_gauss_loss_takes_the_steps_of_a_hand_written_torch_loop(tmp_path):
    from ms_gat_amd import GaussLoss, engine
    sigma, delta = 2.0, 0.1
    batches = _batches(2)
    tr = engine.Trainer(_TinyMSGAT(), 50.0, str(tmp_path / "gauss"), loss=GaussLoss(sigma, delta))
    assert isinstance(tr.loss_fn, GaussLoss) and tr.null_value is None
    got = [tr.run_epoch([b], epoch=i + 1, mode="train") for i, b in enumerate(batches)]
    twin = _TinyMSGAT()
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3, weight_decay=5e-4)
    want = []
    for X, H, D, Y in batches:
        a = torch.abs(twin(X, H, D) - Y)
        loss = sigma ** 2 * torch.mean(1 - torch.exp(-(a ** 2) / (2 * sigma ** 2))) + delta * torch.mean(a)    # loss.py:94-95
        opt.zero_grad()
        loss.backward()
        opt.step()
        want.append(float(loss.detach()))
    assert got == pytest.approx(want, rel=1e-6)
    moved = False
    for p, q, fresh in zip(tr.model.parameters(), twin.parameters(), _TinyMSGAT().parameters()):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-6 * float(q.detach().abs().max()))
        moved = moved or not torch.equal(q, fresh)
    assert moved
    assert sorted(tr.last_stats) == ["MAE", "MAPE", "RMSE", "loss"]
    assert "loss=" in open(tr.log_file).read().splitlines()[-1]


def test_masked_training_reports_the_gauss_loss_per_horizon(tmp_path):
    from ms_gat_amd import GaussLoss, engine
    sigma, delta = 30.0, 0.1
    batches = _batches(3, null_fraction=0.2)
    model = _TinyMSGAT()
    tr = engine.Trainer(model, 50.0, str(tmp_path / "masked"), null_value=0.0, loss=GaussLoss(sigma, delta))
    assert tr.loss_fn.null_value == 0.0
    loss = tr.run_epoch(batches, epoch=1, mode="validate")
    with torch.no_grad():
        pred = torch.cat([model(*b[:3]) for b in batches])
    want = restate(pred, torch.cat([b[3] for b in batches]), sigma, delta, null_value=0.0)
    per = tr.last_stats["horizons"]
    assert sorted(per) == ["MAE", "MAPE", "RMSE", "loss", "valid"] and len(per["loss"]) == 12
    counts = want["sums"][:12, 0]
    assert per["valid"] == counts.tolist() and len(set(per["valid"])) > 1
    assert per["loss"] == pytest.approx((want["sums"][:12, 4] / counts).tolist(), rel=1e-6)
    assert per["MAE"] == pytest.approx((want["sums"][:12, 1] / counts).tolist(), rel=1e-6)
    assert loss == pytest.approx(want["loss"], rel=1e-6) and tr.last_stats["loss"] == loss
    # Metrics on its own: `loss_fn=` fills column 4 and names the list, `delta=` keeps working without it
    m = engine.Metrics(null_value=0.0)
    m.update(pred, torch.cat([b[3] for b in batches]), loss_fn=GaussLoss(sigma, delta))
    assert torch.allclose(m._sums, want["sums"], rtol=1e-6, atol=0.0)
    assert m.at([1, 12])["loss"] == pytest.approx([per["loss"][0], per["loss"][11]], rel=1e-6)
    old = engine.Metrics(null_value=0.0)
    old.update(pred, torch.cat([b[3] for b in batches]), delta=50.0)
    assert sorted(old.per_horizon()) == ["MAE", "MAPE", "RMSE", "valid"] and old.loss > 0


def test_the_loss_argument_defaults_to_huber_and_refuses_what_the_tail_does_not_run(tmp_path):
    from ms_gat_amd import GaussLoss, HuberLoss, engine
    tr = engine.Trainer(_TinyMSGAT(), 7.0, str(tmp_path / "a"))
    assert type(tr.loss_fn) is HuberLoss and tr.loss_fn.delta == 7.0 and tr.loss_fn.null_value is None
    tr = engine.Trainer(_TinyMSGAT(), 7.0, str(tmp_path / "b"), null_value=0.0, loss=None)
    assert type(tr.loss_fn) is HuberLoss and tr.loss_fn.null_value == 0.0
    given = HuberLoss(3.0)
    tr = engine.Trainer(_TinyMSGAT(), 7.0, str(tmp_path / "c"), null_value=0.0, loss=given)
    assert tr.loss_fn is given and given.delta == 3.0 and given.null_value == 0.0          # loss_delta is not read
    tr = engine.Trainer(_TinyMSGAT(), 7.0, str(tmp_path / "d"), null_value=0.0, loss=GaussLoss(null_value=0.0))
    assert tr.null_value == 0.0
    for foreign in (torch.nn.MSELoss(), torch.nn.HuberLoss(), lambda a, b: (a - b).abs().mean(), "gauss"):
        with pytest.raises(TypeError):
            engine.Trainer(_TinyMSGAT(), 7.0, str(tmp_path / "e"), loss=foreign)
    with pytest.raises(ValueError):
        engine.Trainer(_TinyMSGAT(), 7.0, str(tmp_path / "f"), null_value=0.0, loss=GaussLoss(null_value=-1.0))
    ckpt = tmp_path / "net.pkl"
    torch.save(dict(model=_TinyMSGAT().state_dict()), ckpt)
    ev = engine.Evaluator(_TinyMSGAT(), 7.0, str(tmp_path / "g"), ckpt, loss=GaussLoss(2.0, 0.0))
    assert isinstance(ev.loss_fn, GaussLoss)
    assert type(engine.Evaluator(_TinyMSGAT(), 7.0, str(tmp_path / "h"), ckpt).loss_fn) is HuberLoss
    with pytest.raises(TypeError):
        engine.Evaluator(_TinyMSGAT(), 7.0, str(tmp_path / "i"), ckpt, loss=torch.nn.L1Loss())
    with pytest.raises(ValueError):
        engine.Evaluator(_TinyMSGAT(), 7.0, str(tmp_path / "j"), ckpt, null_value=0.0, loss=HuberLoss(1.0, null_value=5.0))
