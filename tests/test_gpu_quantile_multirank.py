"""GPU: the data-parallel step of a quantile forecast with two ranks on one MI355X (two fresh processes sharing cuda:0
over gloo, as in test_gpu_masked_multirank.py).  A rank's weight in the gradient mean is its batch's VALID count, which
`msgat_quantile_metrics` leaves in device memory and `msgat_gather_scaled_dev` reads there: sum_r v_r g_r / sum_r v_r is
the gradient of the global pinball mean for any split.  The shards here keep 90 % and 40 % of their entries."""
import os
import socket
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import record_err
from masked_tail_ref import sharded_truth

pytestmark = pytest.mark.gpu

LEVELS = (0.1, 0.5, 0.9)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, args, world, limit=240.0):
    """`world` processes under one time limit: whoever is still running when it ends is killed and the test fails."""
    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + limit
    while not ctx.join(timeout=2.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"{fn.__name__}: {world} process(es) still running after {limit:.0f} s")


def _model_and_batch(device="cuda:0"):
    """A small msgat48 with a head of 3 x 12 outputs and one global batch of 8 whose 12-step truth keeps 90 % of its
    entries in the first four samples and 40 % in the last four (zeros elsewhere); identical in every process."""
    assert not dist.is_initialized()
    from ms_gat_amd import data, model
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=40, n_edges=50, n_channels=1, in_hours=[1, 2], batch_size=8, days=2)
    net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=36, use_te=True, adj=ds.adj)
    *inputs, y = next(iter(ds.training))
    return net.to(device), [*inputs, sharded_truth(y, (0.9, 0.4), seed=5)]


def _worker(rank, world, port, out_dir):
    """ONE quantile training step from identical parameters; rank 0 stores the gradient the update consumed."""
    from ms_gat_amd import QuantileLoss, engine
    net, batch = _model_and_batch()
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK="0")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    tr = engine.Trainer(net, 50.0, os.path.join(out_dir, f"w{world}"), loss=QuantileLoss(LEVELS, null_value=0.0))
    tr.run_epoch([batch], gpu_id=0, epoch=1, mode="train")
    opt = tr.optimizer
    weight = float(opt.flat_grad[opt.numel]) if world > 1 else None
    flat = opt.flat_grad[: opt.numel] / opt.flat_grad[opt.numel] if world > 1 else opt.flat_grad[: opt.numel]
    names = {id(p): n for n, p in net.named_parameters()}
    if rank == 0:
        grads = {names[id(p)]: flat[o:o + p.numel()].view_as(p).detach().cpu() for p, o in zip(opt._params, opt._offsets)}
        torch.save(dict(grads=grads, weight=weight, stats=tr.last_stats, own_valid=float(tr._valid_count)),
                   os.path.join(out_dir, f"w{world}.pt"))
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_quantile_step_of_two_ranks_equals_the_single_process_step(tmp_path):
    y = _model_and_batch("cpu")[1][-1]
    counts = [int((y[sl] != 0).sum()) for sl in (slice(0, 4), slice(4, 8))]
    assert counts[0] > 2 * counts[1] > 0 and y.shape[-1] == 12
    for world in (1, 2):
        _spawn(_worker, (world, _free_port(), str(tmp_path)), world)
    one, two = (torch.load(str(tmp_path / f"w{w}.pt"), weights_only=False) for w in (1, 2))
    assert one["own_valid"] == sum(counts) and two["own_valid"] == counts[0]
    assert two["weight"] == sum(counts)              # the buffer's last element: sum_r v_r after the collective
    g1, g2 = one["grads"], two["grads"]
    assert g1.keys() == g2.keys() and len(g1) > 20
    # the measure and the 1e-5 of test_masked_step_of_two_ranks_equals_the_single_process_step: per tensor on its own scale;
    # tensors more than 100x below the largest gradient are judged on that scale
    gscale = max(float(v.abs().max()) for v in g1.values())

    def err(k):
        return float((g2[k].double() - g1[k].double()).abs().max()) / max(float(g1[k].abs().max()), 1e-2 * gscale)
    worst = max(err(k) for k in g1)
    record_err("quantile two_ranks_vs_one_gradient", "worst tensor", worst, 1e-5)
    print(f"valid counts {counts}: worst tensor {worst:.2e}")
    for k in g1:
        assert err(k) < 1e-5, (k, err(k))
    # the epoch's loss, metrics and quantile statistics are ratios of totals: the same for one process and for two
    for k in ("loss", "MAE", "MAPE", "RMSE"):
        assert abs(one["stats"][k] - two["stats"][k]) <= 1e-5 * abs(one["stats"][k]), (k, one["stats"], two["stats"])
    assert one["stats"]["horizons"]["valid"] == two["stats"]["horizons"]["valid"]
    assert sum(two["stats"]["horizons"]["valid"]) == sum(counts)
    q1, q2 = one["stats"]["quantiles"], two["stats"]["quantiles"]
    assert q1["coverage"] == q2["coverage"] and q1["crossing"] == q2["crossing"]         # counts over a count
    assert q2["pinball"] == pytest.approx(q1["pinball"], rel=1e-5)
    assert abs(q1["width"] - q2["width"]) <= 1e-5 * max(abs(q1["width"]), 1.0)
