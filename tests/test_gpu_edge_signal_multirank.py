"""GPU: `MSGAT(learn_edge_weights="signal")` in the data-parallel step with TWO ranks on one MI355X (fresh child processes
sharing cuda:0 over gloo, the harness of tests/test_gpu_multirank.py): `edge_proj.weight` and `edge_weight` are ordinary
dense parameters of the flat all-reduce, so the gradient the update consumes -- every rank's gradient of its shard, scaled
by the shard size, summed and divided by the global batch size -- must be the single process's gradient of the whole batch.
Shards are uneven: 7 = 4 + 3 samples."""
import os

import pytest
import torch
import torch.distributed as dist

from conftest import record_err
from test_gpu_edge_time_multirank import _spawn
from test_gpu_multirank import _free_port, _join, _leave

pytestmark = pytest.mark.gpu

SIZE = 7


def _signal_model_and_batch(size):
    """A small "signal" msgat48 (two components) with a non-zero projection and one global batch, identical in every
    process; called before joining the process group, as `_model_and_batches` of tests/test_gpu_multirank.py is."""
    assert not dist.is_initialized()
    from ms_gat_amd import data, model
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=40, n_edges=50, n_channels=1, in_hours=[1, 2], batch_size=8, days=2)
    net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj,
                        learn_edge_weights="signal")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        net.edge_proj.weight.copy_(torch.randn(net.edge_proj.weight.shape, generator=g) * 0.1)
    batch = [t[:size] for t in next(iter(ds.training))]
    return net.to("cuda:0"), batch


def _first_step_gradient_worker(rank, world, port, size, out_dir):
    """ONE training step; rank 0 stores the gradient the update consumed, per parameter (see the worker of the same name
    in tests/test_gpu_multirank.py)."""
    from ms_gat_amd import engine
    net, batch = _signal_model_and_batch(size)
    _join(rank, world, port)
    tr = engine.Trainer(net, 50.0, os.path.join(out_dir, f"grad_w{world}"), hip_graph=False)
    tr.run_epoch([batch], gpu_id=0, epoch=1, mode="train")
    opt = tr.optimizer
    assert isinstance(opt, engine.FlatAdam)
    flat = opt.flat_grad[: opt.numel] / opt.flat_grad[opt.numel] if world > 1 else opt.flat_grad[: opt.numel]
    names = {id(p): n for n, p in net.named_parameters()}
    if rank == 0:
        grads = {names[id(p)]: flat[o:o + p.numel()].view_as(p).detach().cpu() for p, o in zip(opt._params, opt._offsets)}
        torch.save(dict(grads=grads), os.path.join(out_dir, f"grad_w{world}.pt"))
    _leave(world)


def test_whole_step_gradient_of_two_ranks_equals_the_single_process_gradient(tmp_path):
    for world in (1, 2):
        _spawn(_first_step_gradient_worker, (world, _free_port(), SIZE, str(tmp_path)), world)
    g1 = torch.load(str(tmp_path / "grad_w1.pt"), weights_only=False)["grads"]
    g2 = torch.load(str(tmp_path / "grad_w2.pt"), weights_only=False)["grads"]
    assert g1.keys() == g2.keys() and "edge_proj.weight" in g1
    # per tensor on its own scale, floored at 1/100 of the largest gradient, to 1e-5: the bar and the rule of
    # test_whole_step_gradient_of_two_ranks_equals_the_single_process_gradient (only the summation order over the batch differs)
    gscale = max(float(v.abs().max()) for v in g1.values())

    def err(k):
        return float((g2[k].double() - g1[k].double()).abs().max()) / max(float(g1[k].abs().max()), 1e-2 * gscale)
    rank = g1["edge_proj.weight"].shape[0] // 2
    assert float(g1["edge_proj.weight"][:rank].abs().max()) > 0 and float(g1["edge_proj.weight"][rank:].abs().max()) > 0
    for k in ("edge_proj.weight", "edge_weight"):
        assert float(g1[k].abs().max()) > 0, k
        record_err("two_ranks_vs_one_signal_gradient", k, err(k), 1e-5)
        assert err(k) < 1e-5, (k, err(k))
    worst = max(err(k) for k in g1)
    record_err("two_ranks_vs_one_signal_gradient", "worst tensor", worst, 1e-5)
    assert worst < 1e-5, max((err(k), k) for k in g1)
