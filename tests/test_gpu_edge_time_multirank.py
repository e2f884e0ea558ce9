"""GPU: `MSGAT(learn_edge_weights="time")` in the data-parallel step with TWO ranks on one MI355X (fresh child processes
sharing cuda:0 over gloo, the harness of tests/test_gpu_multirank.py): the hour and day tables are ordinary dense
parameters of the flat all-reduce, so the gradient the update consumes -- every rank's dense [24,nnz] / [7,nnz] table
gradient of its shard, scaled by the shard size, summed and divided by the global batch size -- must be the single
process's gradient of the whole batch.  Shards are uneven: 7 = 4 + 3 samples."""
import os
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import record_err
from test_gpu_multirank import _free_port, _join, _leave

pytestmark = pytest.mark.gpu

SIZE = 7
CHILD_LIMIT = 180.0     # seconds for one group of child processes (they take ~20 s)


def _spawn(fn, args, nprocs):
    """`mp.spawn` under a time limit of its own: a child's failure raises here (and ends its siblings), a group that does
    not finish in time is killed; either way nothing of the chain behind it is started."""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + CHILD_LIMIT
    while not ctx.join(timeout=5.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail(f"{fn.__name__} x{nprocs} did not finish within {CHILD_LIMIT:.0f} s")


def _time_model_and_batch(size):
    """A small "time" msgat48 (two components) with non-zero tables and one global batch, identical in every process;
    called before joining the process group, as `_model_and_batches` of tests/test_gpu_multirank.py is."""
    assert not dist.is_initialized()
    from ms_gat_amd import data, model
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=40, n_edges=50, n_channels=1, in_hours=[1, 2], batch_size=8, days=2)
    net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj,
                        learn_edge_weights="time")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for t in (net.edge_h_ebd.weight, net.edge_d_ebd.weight):
            t.copy_(torch.randn(t.shape, generator=g) * 0.05)
    batch = [t[:size] for t in next(iter(ds.training))]
    return net.to("cuda:0"), batch


def _first_step_gradient_worker(rank, world, port, size, out_dir):
    """ONE training step; rank 0 stores the gradient the update consumed, per parameter (see the worker of the same name
    in tests/test_gpu_multirank.py), and the hours and days of the whole batch."""
    from ms_gat_amd import engine
    net, batch = _time_model_and_batch(size)
    _join(rank, world, port)
    tr = engine.Trainer(net, 50.0, os.path.join(out_dir, f"grad_w{world}"), hip_graph=False)
    tr.run_epoch([batch], gpu_id=0, epoch=1, mode="train")
    opt = tr.optimizer
    assert isinstance(opt, engine.FlatAdam)
    flat = opt.flat_grad[: opt.numel] / opt.flat_grad[opt.numel] if world > 1 else opt.flat_grad[: opt.numel]
    names = {id(p): n for n, p in net.named_parameters()}
    if rank == 0:
        grads = {names[id(p)]: flat[o:o + p.numel()].view_as(p).detach().cpu() for p, o in zip(opt._params, opt._offsets)}
        torch.save(dict(grads=grads, H=batch[1].cpu(), D=batch[2].cpu()), os.path.join(out_dir, f"grad_w{world}.pt"))
    _leave(world)


def test_table_gradients_of_two_ranks_equal_the_single_process_gradient(tmp_path):
    for world in (1, 2):
        _spawn(_first_step_gradient_worker, (world, _free_port(), SIZE, str(tmp_path)), world)
    one = torch.load(str(tmp_path / "grad_w1.pt"), weights_only=False)
    two = torch.load(str(tmp_path / "grad_w2.pt"), weights_only=False)
    assert torch.equal(one["H"], two["H"]) and torch.equal(one["D"], two["D"])
    g1, g2 = one["grads"], two["grads"]
    assert g1.keys() == g2.keys()
    tables = {"edge_h_ebd.weight": one["H"], "edge_d_ebd.weight": one["D"]}
    # per tensor on its own scale, floored at 1/100 of the largest gradient, to 1e-5: the bar and the rule of
    # test_whole_step_gradient_of_two_ranks_equals_the_single_process_gradient (only the summation order over the batch differs)
    gscale = max(float(v.abs().max()) for v in g1.values())

    def err(k):
        return float((g2[k].double() - g1[k].double()).abs().max()) / max(float(g1[k].abs().max()), 1e-2 * gscale)
    for k in list(tables) + ["edge_weight"]:
        assert float(g1[k].abs().max()) > 0, k
        record_err("two_ranks_vs_one_time_gradient", k, err(k), 1e-5)
        assert err(k) < 1e-5, (k, err(k))
    for k, idx in tables.items():         # a row no sample of the WHOLE batch selected is exactly zero on both sides
        unused = torch.ones(g1[k].shape[0], dtype=torch.bool)
        unused[idx.long().clamp(0, g1[k].shape[0] - 1)] = False
        assert unused.any() and torch.count_nonzero(g1[k][unused]) == 0 and torch.count_nonzero(g2[k][unused]) == 0, k
    worst = max(err(k) for k in g1)
    record_err("two_ranks_vs_one_time_gradient", "worst tensor", worst, 1e-5)
    assert worst < 1e-5, max((err(k), k) for k in g1)
