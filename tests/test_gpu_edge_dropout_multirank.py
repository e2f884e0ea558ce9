"""GPU: `MSGAT(edge_dropout=p)` in the data-parallel step with TWO ranks on one MI355X (fresh child processes sharing
cuda:0 over gloo, the harness of tests/test_gpu_edge_time_multirank.py).  A sample's masks are a function of its index in
the GLOBAL batch: `run_epoch` hands the model the offset of its shard, so each rank's masked weights are its rows of the
single process's draw, bit for bit, and the gradient the update consumes is the single process's gradient of the whole
batch.  Shards are uneven: 7 = 4 + 3 samples."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from conftest import record_err
from test_gpu_multirank import _free_port, _join, _leave
from test_gpu_edge_time_multirank import _spawn

import edge_dropout_ref as ref

pytestmark = pytest.mark.gpu

SIZE, P, SEED = 7, 0.25, 41


def _dropout_model_and_batch(size):
    """A small "time" msgat48 (two components) with non-zero tables that drops edges, and one global batch, identical in
    every process; called before joining the process group."""
    assert not dist.is_initialized()
    from ms_gat_amd import data, model
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=40, n_edges=50, n_channels=1, in_hours=[1, 2], batch_size=8, days=2)
    net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj,
                        learn_edge_weights="time", edge_dropout=P, edge_dropout_seed=SEED)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for t in (net.edge_h_ebd.weight, net.edge_d_ebd.weight):
            t.copy_(torch.randn(t.shape, generator=g) * 0.05)
    batch = [t[:size] for t in next(iter(ds.training))]
    return net.to("cuda:0"), batch


def _first_step_worker(rank, world, port, size, out_dir):
    """ONE training step; every rank stores the masked weights its forward drew and the offset it drew them at, rank 0
    also the gradient the update consumed, per parameter."""
    from ms_gat_amd import engine
    net, batch = _dropout_model_and_batch(size)
    _join(rank, world, port)
    seen, inner = [], net._drop_edges

    def recording(weights, samples):
        out = inner(weights, samples)
        seen.append((out.detach().clone(), weights.detach().clone(), int(net.edge_dropout_sample_offset)))
        return out
    net._drop_edges = recording
    tr = engine.Trainer(net, 50.0, os.path.join(out_dir, f"grad_w{world}"), hip_graph=False)
    tr.run_epoch([batch], gpu_id=0, epoch=1, mode="train")
    opt = tr.optimizer
    flat = opt.flat_grad[: opt.numel] / opt.flat_grad[opt.numel] if world > 1 else opt.flat_grad[: opt.numel]
    names = {id(p): n for n, p in net.named_parameters()}
    assert len(seen) == 1                                     # one draw per forward, shared by components and blocks
    masked, weights, offset = seen[0]
    stored = dict(masked=masked.cpu(), weights=weights.cpu(), offset=offset, state=net.edge_dropout_state(),
                  exempt=net.edge_drop_exempt.cpu())
    if rank == 0:
        stored["grads"] = {names[id(p)]: flat[o:o + p.numel()].view_as(p).detach().cpu()
                           for p, o in zip(opt._params, opt._offsets)}
    torch.save(stored, os.path.join(out_dir, f"w{world}_r{rank}.pt"))
    _leave(world)


def test_two_ranks_draw_the_single_process_masks_and_get_its_gradient(tmp_path):
    from ms_gat_amd import parallel
    for world in (1, 2):
        _spawn(_first_step_worker, (world, _free_port(), SIZE, str(tmp_path)), world)
    one = torch.load(str(tmp_path / "w1_r0.pt"), weights_only=False)
    ranks = [torch.load(str(tmp_path / f"w2_r{r}.pt"), weights_only=False) for r in range(2)]
    assert one["offset"] == 0 and one["state"] == {"seed": SEED, "step": 1}
    # the single process's draw is the restatement's
    exempt = one["exempt"].numpy().astype(bool)
    want = ref.forward(one["weights"].numpy(), SEED, 0, SIZE, P, 0, exempt)
    assert np.array_equal(one["masked"].numpy().view(np.int32), want.view(np.int32))
    assert (one["masked"] == 0).any()
    for r, got in enumerate(ranks):
        lo, hi = parallel.shard_bounds(SIZE, r, 2)
        assert got["offset"] == lo and got["state"] == {"seed": SEED, "step": 1}
        assert torch.equal(got["weights"], one["weights"][lo:hi])
        assert torch.equal(got["masked"], one["masked"][lo:hi]), r        # its rows of the whole draw, bit for bit
    assert not torch.equal(ranks[1]["masked"] == 0, (one["masked"] == 0)[:3])   # and not the rows an offset of 0 would give
    # the gradient: per tensor on its own scale, floored at 1/100 of the largest gradient, to 1e-5 -- the bar and the rule
    # of test_table_gradients_of_two_ranks_equal_the_single_process_gradient (only the summation order over the batch differs)
    g1, g2 = one["grads"], ranks[0]["grads"]
    assert g1.keys() == g2.keys()
    gscale = max(float(v.abs().max()) for v in g1.values())

    def err(k):
        return float((g2[k].double() - g1[k].double()).abs().max()) / max(float(g1[k].abs().max()), 1e-2 * gscale)
    for k in ("edge_weight", "edge_h_ebd.weight", "edge_d_ebd.weight"):
        assert float(g1[k].abs().max()) > 0, k
        record_err("two_ranks_vs_one_edge_dropout_gradient", k, err(k), 1e-5)
        assert err(k) < 1e-5, (k, err(k))
    worst = max(err(k) for k in g1)
    record_err("two_ranks_vs_one_edge_dropout_gradient", "worst tensor", worst, 1e-5)
    assert worst < 1e-5, max((err(k), k) for k in g1)
