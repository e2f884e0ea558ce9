"""Host side of the masked step tail (missing readings, per-horizon metrics): the torch path of `HuberLoss(null_value)`
and `Metrics(null_value)` against the float64 restatement of tests/masked_tail_ref.py, the off switch, the epoch loss as
a ratio of totals, tensor rank weights over gloo, and the new C-ABI entry points.  No device compute is called here."""
import ctypes as C
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from masked_tail_ref import make_inputs, metrics_of, restate, sharded_truth

DELTA = 50.0
SHAPE = (4, 9, 12)


@pytest.fixture(scope="module")
def case():
    pred, truth = make_inputs(SHAPE, seed=0, delta=DELTA, n_nan=3)
    return pred, truth, restate(pred, truth, DELTA, 0.0, mask_value=30.0)


def _close(got, want, rel=1e-6):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == pytest.approx(b, rel=rel, abs=0.0), (got, want)


def test_masked_huber_loss_and_its_gradient_on_cpu_tensors_match_the_restatement(case):
    from ms_gat_amd import engine
    pred, truth, want = case
    p = pred.clone().requires_grad_(True)
    loss = engine.HuberLoss(DELTA, null_value=0.0)(p, truth)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(want["loss"], rel=1e-5)
    invalid = torch.isnan(truth) | (truth == 0.0)
    assert int((~invalid).sum()) == want["valid"] and 3 <= int(torch.isnan(truth).sum())
    assert not torch.isnan(p.grad).any()
    assert bool((p.grad[invalid] == 0).all())
    ref = want["dpred"]
    assert bool(((p.grad.double() - ref).abs() <= 1e-5 * ref.abs()).all())
    # float64 inputs: the same definition to rounding
    assert float(engine.masked_huber_loss(pred.double(), truth.double(), DELTA, 0.0)) == pytest.approx(want["loss"], rel=1e-12)


def test_masked_loss_of_a_batch_without_a_valid_entry_is_zero_with_a_zero_gradient():
    from ms_gat_amd import engine
    p = torch.randn(2, 3, 4, requires_grad=True)
    truth = torch.zeros(2, 3, 4)
    truth[0, 0, 0] = float("nan")
    loss = engine.HuberLoss(1.0, null_value=0.0)(p, truth)
    loss.backward()
    assert float(loss.detach()) == 0.0 and bool((p.grad == 0).all())


def test_null_value_nan_masks_only_the_nan_entries(case):
    from ms_gat_amd import engine
    pred, truth, _ = case
    want = restate(pred, truth, DELTA, float("nan"))
    assert want["valid"] == truth.numel() - int(torch.isnan(truth).sum())
    assert float(engine.HuberLoss(DELTA, null_value=float("nan"))(pred, truth)) == pytest.approx(want["loss"], rel=1e-5)


def test_masked_metrics_on_cpu_tensors_match_the_restatement_per_horizon(case):
    from ms_gat_amd import engine
    pred, truth, want = case
    m = engine.Metrics(mask_value=30.0, null_value=0.0)
    m.update(pred, truth, delta=DELTA)
    t_out = SHAPE[-1]
    assert tuple(m._sums.shape) == (t_out + 1, 5) and m._sums.dtype == torch.float64
    assert torch.equal(m._sums[:, 0], want["sums"][:, 0])                        # counts are exact
    assert torch.allclose(m._sums, want["sums"], rtol=1e-12, atol=0.0)
    ref = metrics_of(want["sums"])
    per = m.per_horizon()
    assert sorted(per) == ["MAE", "MAPE", "RMSE", "valid"]
    for k in per:
        assert len(per[k]) == t_out
        _close(per[k], ref[k][:t_out])
    ends = m.at([1, t_out])
    for k in per:
        _close(ends[k], [ref[k][0], ref[k][t_out - 1]])
    with pytest.raises(IndexError):
        m.at([0])
    assert m.MAE == pytest.approx(ref["MAE"][-1], rel=1e-12) and m.MAPE == pytest.approx(ref["MAPE"][-1], rel=1e-12)
    assert m.RMSE == pytest.approx(ref["RMSE"][-1], rel=1e-12) and m.loss == pytest.approx(want["loss"], rel=1e-12)
    # a second batch accumulates; reset() zeroes the SAME buffer
    buf = m._sums
    m.update(pred, truth, delta=DELTA)
    assert torch.allclose(m._sums, 2 * want["sums"], rtol=1e-12, atol=0.0)
    m.reset()
    assert m._sums is buf and not m._sums.any() and m.loss == 0.0 and m.MAE == 0.0


def test_loss_and_metrics_without_null_value_are_bit_for_bit_the_plain_formulas():
    """The off switch: `null_value=None` (the default) computes what the plain formulas of the unmasked tail compute, to
    the bit, also on inputs with zeros in the truth."""
    from ms_gat_amd import engine
    pred, truth = make_inputs(SHAPE, seed=1, delta=DELTA)
    err = (pred - truth).abs()
    want_loss = torch.where(err <= DELTA, 0.5 * err * err, DELTA * err - 0.5 * DELTA * DELTA).mean()
    for loss_fn in (engine.HuberLoss(DELTA), engine.HuberLoss(DELTA, null_value=None)):
        assert torch.equal(loss_fn(pred, truth), want_loss)
    m = engine.Metrics()
    assert m.null_value is None
    m.update(pred, truth, want_loss)
    e, y = (pred - truth).double(), truth.double()
    mask = y > 0.0
    ape = torch.where(mask, (e / torch.where(mask, y, torch.ones_like(y))).abs(), torch.zeros_like(e))
    want = torch.stack([e.abs().sum(), 100.0 * ape.sum(), (e * e).sum(), want_loss.double() * 1.0])
    assert tuple(m._sums.shape) == (4,) and torch.equal(m._sums, want)
    n = truth.numel()
    assert m.MAE == float(want[0]) / n and m.MAPE == float(want[1]) / n and m.RMSE == (float(want[2]) / n) ** 0.5
    assert m.loss == float(want[3]) / 1 and m.todict() == {"MAE": m.MAE, "MAPE": m.MAPE, "RMSE": m.RMSE}
    with pytest.raises(ValueError):
        m.per_horizon()


def test_epoch_loss_is_a_ratio_of_totals_the_same_for_one_process_and_a_two_way_split():
    """Two shards with unequal valid counts, merged as `all_reduce()` merges them (a sum of the buffers): the epoch
    loss and metrics equal the single-process ones, while the mean of the two shard means does not."""
    from ms_gat_amd import engine
    pred, truth = make_inputs((8, 6, 12), seed=2, delta=DELTA, null_fraction=0.0)
    truth = sharded_truth(truth, (0.9, 0.4), seed=3)
    whole = engine.Metrics(null_value=0.0)
    whole.update(pred, truth, delta=DELTA)
    parts = []
    for sl in (slice(0, 4), slice(4, 8)):
        m = engine.Metrics(null_value=0.0)
        m.update(pred[sl], truth[sl], delta=DELTA)
        parts.append(m)
    counts = [float(m._sums[-1, 0]) for m in parts]
    assert counts[0] > 1.5 * counts[1] > 0
    merged = engine.Metrics(null_value=0.0)
    merged.totals(torch.device("cpu"), 12).add_(parts[0]._sums).add_(parts[1]._sums)
    want = restate(pred, truth, DELTA, 0.0)
    assert merged.loss == pytest.approx(whole.loss, rel=1e-12) and whole.loss == pytest.approx(want["loss"], rel=1e-12)
    for k in ("MAE", "MAPE", "RMSE"):
        assert getattr(merged, k) == pytest.approx(getattr(whole, k), rel=1e-12)
    _close(merged.per_horizon()["MAE"], whole.per_horizon()["MAE"], rel=1e-12)
    mean_of_means = 0.5 * (parts[0].loss + parts[1].loss)
    assert abs(mean_of_means - whole.loss) > 1e-3 * whole.loss


def test_sample_count_weights_miss_the_gradient_of_the_global_masked_mean_by_a_wide_margin():
    """The inputs of the multi-rank GPU test (shards with 90 % and 40 % valid entries), judged once on the CPU with the
    restatement: valid-count weights reproduce the gradient of the global masked mean, sample-count weights -- the
    unmasked rule -- are off by tens of percent, so that test's 1e-5 bound can fail."""
    pred, truth = make_inputs((8, 6, 12), seed=2, delta=DELTA, null_fraction=0.0)
    truth = sharded_truth(truth, (0.9, 0.4), seed=3)
    whole = restate(pred, truth, DELTA, 0.0)
    shards = [restate(pred[sl], truth[sl], DELTA, 0.0) for sl in (slice(0, 4), slice(4, 8))]
    v = [s["valid"] for s in shards]
    by_valid = torch.cat([s["dpred"] * (c / sum(v)) for s, c in zip(shards, v)])
    by_samples = torch.cat([s["dpred"] * (4 / 8) for s in shards])
    scale = float(whole["dpred"].abs().max())
    assert float((by_valid - whole["dpred"]).abs().max()) < 1e-12 * scale
    assert float((by_samples - whole["dpred"]).abs().max()) > 0.1 * scale


# ---- tensor rank weights over gloo ------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _weights_worker(rank, world, port, out):
    from ms_gat_amd import parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    parallel.init_from_env("gloo")
    g = torch.Generator().manual_seed(7)
    grads = [[torch.randn(3, 2, generator=g), torch.randn(5, generator=g)] for _ in range(world)]    # every rank's, everywhere
    got = {}
    for name, weights, zero in (("v35", (3.0, 5.0), False), ("v00", (0.0, 0.0), True)):
        params = [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(5))]
        for p, gr in zip(params, grads[rank]):
            p.grad = torch.zeros_like(gr) if zero else gr.clone()
        parallel.FlatGradAllReduce(params)(weight=torch.tensor([weights[rank]]))
        got[name] = [p.grad.clone() for p in params]
    if rank == 0:
        torch.save(dict(got=got, grads=grads), out)
    dist.barrier()
    dist.destroy_process_group()


def test_flat_grad_all_reduce_takes_one_element_tensor_weights_over_gloo(tmp_path):
    out = str(tmp_path / "weights.pt")
    mp.spawn(_weights_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r = torch.load(out, weights_only=False)
    for a, g0, g1 in zip(r["got"]["v35"], *r["grads"]):
        assert torch.allclose(a, (3.0 * g0 + 5.0 * g1) / 8.0, rtol=1e-6, atol=1e-7)
    for a in r["got"]["v00"]:        # nothing valid anywhere: the summed weight is clamped to 1, zeros stay zeros
        assert not torch.isnan(a).any() and not a.any()


def test_tensor_rank_weight_must_be_one_float32_element():
    from ms_gat_amd import parallel
    with pytest.raises(ValueError):
        parallel._device_weight(torch.ones(2), torch.device("cpu"))
    with pytest.raises(ValueError):
        parallel._device_weight(torch.ones(1, dtype=torch.float64), torch.device("cpu"))


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


_NEW = {"msgat_masked_huber_partial_doubles": 2, "msgat_masked_huber_metrics": 12, "msgat_masked_huber_grad": 10,
        "msgat_gather_scaled_dev": 8}


def test_new_entry_points_are_declared_exported_and_bound_with_the_documented_arguments(built_library):
    from ms_gat_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in _NEW.items():
        assert hasattr(h, name), name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name
        assert len(_lib._PROTOTYPES[name][1]) == n_args, name
    assert "const float* scale" in re.search(r"msgat_gather_scaled_dev\s*\(([^)]*)\)", code).group(1)
    # the unmasked entry points keep their signatures
    assert len(_lib._PROTOTYPES["msgat_huber_metrics"][1]) == 10 and len(_lib._PROTOTYPES["msgat_huber_grad"][1]) == 7
    assert _lib._PROTOTYPES["msgat_gather_scaled"][1][4] is C.c_float
    assert _lib.lib().msgat_abi_version() == _lib.ABI_VERSION
    assert "msgat_masked_huber_{partial_doubles,metrics,grad} and msgat_gather_scaled_dev" in header


def test_masked_entry_points_report_bad_arguments_before_any_launch(built_library):
    from ms_gat_amd import _lib
    L = _lib.lib()
    x = C.cast(C.create_string_buffer(64), C.c_void_p)       # a non-NULL pointer; nothing is launched on these paths
    assert L.msgat_masked_huber_metrics(None, x, 4, 3, 1.0, 0.0, 0.0, x, x, x, None, None) == -1
    assert L.msgat_masked_huber_metrics(x, x, 4, 3, 1.0, 0.0, 0.0, x, x, None, None, None) == -1     # valid is required
    assert L.msgat_masked_huber_metrics(x, x, 0, 3, 1.0, 0.0, 0.0, x, x, x, None, None) == -2
    assert L.msgat_masked_huber_metrics(x, x, 4, 0, 1.0, 0.0, 0.0, x, x, x, None, None) == -2
    assert L.msgat_masked_huber_metrics(x, x, 4, 65, 1.0, 0.0, 0.0, x, x, x, None, None) == -3       # as the head: T_out <= 64
    assert L.msgat_masked_huber_metrics(x, x, (1 << 24) // 64 + 1, 64, 1.0, 0.0, 0.0, x, x, x, None, None) == -3
    assert L.msgat_masked_huber_grad(x, x, x, None, 4, 3, 1.0, 0.0, x, None) == -1
    assert L.msgat_masked_huber_grad(x, x, x, x, -1, 3, 1.0, 0.0, x, None) == -2
    assert L.msgat_masked_huber_grad(x, x, x, x, 4, 65, 1.0, 0.0, x, None) == -3
    assert L.msgat_gather_scaled_dev(x, x, x, 1, None, x, 0, None) == -1
    assert L.msgat_gather_scaled_dev(x, x, x, 0, x, x, 0, None) == -2
    assert L.msgat_masked_huber_partial_doubles(4, 65) == 0 and L.msgat_masked_huber_partial_doubles(0, 3) == 0
    # one [5, T_out] record per block: a block's lanes cover (256 // T_out) * T_out entries eight times each
    assert L.msgat_masked_huber_partial_doubles(10, 3) == 5 * 3
    assert L.msgat_masked_huber_partial_doubles(3 * 47, 24) == 2 * 5 * 24
    assert L.msgat_masked_huber_partial_doubles(32 * 883, 37) == 512 * 5 * 37


def test_masked_op_refuses_cpu_tensors_and_mismatched_buffers():
    from ms_gat_amd import _lib, ops
    with pytest.raises(_lib.MsgatError):
        ops.masked_huber_metrics(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), 1.0, 0.0)


# ---- Engine.run_epoch with null_value on CPU tensors (torch ops for loss, metrics and the weighted all-reduce) -------------
class _TinyMSGAT(torch.nn.Module):
    """CPU stand-in with the MSGAT call signature model(X, H, D) -> [B,N,T]."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.mix = torch.nn.Conv2d(4, 1, 1)

    def forward(self, X, H, D):
        B, R, C, N, T = X.shape
        return self.mix(X.reshape(B, R * C, N, T)).squeeze(1)


def _epoch_batches():
    g = torch.Generator().manual_seed(11)
    out = []
    for i in range(3):
        y = sharded_truth(100.0 + 30.0 * torch.randn(8, 5, 12, generator=g), ((0.9, 0.4), (0.3, 1.0), (0.6, 0.5))[i], seed=i)
        out.append((torch.randn(8, 2, 2, 5, 12, generator=g) * 40, torch.zeros(8, dtype=torch.long),
                    torch.zeros(8, dtype=torch.long), y))
    return out


def _epoch_worker(rank, world, port, out_dir):
    from ms_gat_amd import engine, parallel
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        parallel.init_from_env("gloo")
    model = _TinyMSGAT()
    tr = engine.Trainer(model, DELTA, os.path.join(out_dir, f"w{world}"), null_value=0.0)
    losses = [tr.run_epoch(_epoch_batches(), epoch=e, mode="train") for e in (1, 2)]
    train_stats = tr.last_stats
    val = tr.run_epoch(_epoch_batches(), epoch=2, mode="validate")
    if rank == 0:
        torch.save(dict(losses=losses, val=val, stats=tr.last_stats, train_stats=train_stats,
                        params=[p.detach().clone() for p in model.parameters()], log=open(tr.log_file).read()),
                   os.path.join(out_dir, f"result_w{world}.pt"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_masked_run_epoch_on_two_ranks_equals_the_single_process_run(tmp_path):
    """Shards with unequal valid counts: valid-count weights make the update, and ratios of totals make the logged
    loss and metrics, those of the single process.  The per-horizon line is logged for validation epochs only."""
    out = str(tmp_path)
    _epoch_worker(0, 1, 0, out)
    mp.spawn(_epoch_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    one, two = (torch.load(os.path.join(out, f"result_w{w}.pt"), weights_only=False) for w in (1, 2))
    for a, b in zip(one["params"], two["params"]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    assert one["losses"] == pytest.approx(two["losses"], rel=1e-5) and one["val"] == pytest.approx(two["val"], rel=1e-5)
    for k in ("MAE", "MAPE", "RMSE"):
        assert one["stats"][k] == pytest.approx(two["stats"][k], rel=1e-6)
        assert one["stats"]["horizons"][k] == pytest.approx(two["stats"]["horizons"][k], rel=1e-6)
    assert one["stats"]["horizons"]["valid"] == two["stats"]["horizons"]["valid"]
    # against the restatement, with the parameters the validation pass ran with
    model = _TinyMSGAT()
    with torch.no_grad():
        for p, q in zip(model.parameters(), one["params"]):
            p.copy_(q)
        batches = _epoch_batches()
        pred = torch.cat([model(*b[:3]) for b in batches])
    want = restate(pred, torch.cat([b[3] for b in batches]), DELTA, 0.0)
    ref = metrics_of(want["sums"])
    assert one["val"] == pytest.approx(want["loss"], rel=1e-6)
    for k in ("MAE", "MAPE", "RMSE", "valid"):
        assert one["stats"]["horizons"][k] == pytest.approx(ref[k][:12], rel=1e-6)
    assert "horizons" in one["train_stats"]
    for r in (one, two):
        lines = r["log"].splitlines()
        assert len(lines) == 4 and ["per horizon" in ln for ln in lines] == [False, False, False, True]
        assert "[Validate] - per horizon - epoch=2,MAE=" in lines[3]


def test_run_epoch_without_null_value_logs_and_reports_what_it_did_before(tmp_path):
    from ms_gat_amd import engine
    tr = engine.Trainer(_TinyMSGAT(), DELTA, str(tmp_path / "plain"))
    assert tr.null_value is None and tr.loss_fn.null_value is None
    tr.run_epoch(_epoch_batches(), epoch=1, mode="validate")
    assert sorted(tr.last_stats) == ["MAE", "MAPE", "RMSE", "loss"]
    lines = open(tr.log_file).read().splitlines()
    assert len(lines) == 1 and "per horizon" not in lines[0] and "[Validate] - epoch=1,loss=" in lines[0]
