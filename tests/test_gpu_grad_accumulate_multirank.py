"""GPU: gradient accumulation and the data-parallel step, with the harness of tests/test_gpu_multirank.py (two fresh
processes sharing cuda:0 that talk over gloo on device tensors).

A window of k micro-batches fills the flat buffer the way k ranks and their all-reduce do: `w * g` rounded, then the sum
rounded, the weights summed beside them.  So one process with a window of two IS, to the bit, two ranks on the same two
micro-batches as their shards; and with several ranks the collective runs once per window, on the locally accumulated
buffer."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from conftest import record_err
from test_gpu_multirank import _free_port, _join, _leave, _model_and_batches

pytestmark = pytest.mark.gpu


def _union(batches):
    return [torch.cat([b[i] for b in batches]) for i in range(4)]


def _worker(rank, world, port, what, out_dir):
    from ms_gat_amd import engine, parallel
    kw, poisoned = {}, False
    if what == "window_of_two":          # one process, micro-batches m0 m1 | m2 m3
        net, batches = _model_and_batches((4, 4, 4, 4))
        kw = dict(accumulate_steps=2)
    elif what == "two_shards":           # two ranks, global batches m0 + m1 | m2 + m3: the same micro-batches as shards
        net, micro = _model_and_batches((4, 4, 4, 4))
        batches = [_union(micro[:2]), _union(micro[2:])]
    elif what == "ranks_with_windows":   # two ranks, a window of two global batches of 8: four micro-batches in all
        net, batches = _model_and_batches((8, 8))
        kw = dict(accumulate_steps=2)
    elif what == "union_of_four":        # one process, one batch of the same 16 samples
        net, two = _model_and_batches((8, 8))
        batches = [_union(two)]
    elif what == "six_batches":          # two ranks, k = 3: two windows, two collectives
        net, batches = _model_and_batches((8,) * 6)
        kw = dict(accumulate_steps=3)
    else:                                # "poisoned": a NaN in rank 1's shard of the window's second global batch
        assert what == "poisoned"
        net, batches = _model_and_batches((8, 8))
        batches[1][0][5, 0, 0, 3, 7] = float("nan")
        kw, poisoned = dict(accumulate_steps=2, skip_nonfinite=True), True
    start = {k: v.detach().cpu().clone() for k, v in net.named_parameters()}
    _join(rank, world, port)
    events = parallel.collective_events = []
    tr = engine.Trainer(net, 50.0, os.path.join(out_dir, f"{what}_r{rank}"), hip_graph=False, **kw)
    tr.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
    opt = tr.optimizer
    divided = world > 1 or tr.accumulate_steps > 1
    flat = opt.flat_grad[: opt.numel] / opt.flat_grad[opt.numel] if divided else opt.flat_grad[: opt.numel]
    names = {id(p): n for n, p in net.named_parameters()}
    out = dict(params={k: v.detach().cpu() for k, v in net.named_parameters()}, start=start,
               grads={names[id(p)]: flat[o:o + p.numel()].view_as(p).detach().cpu() for p, o in zip(opt._params, opt._offsets)},
               weight=float(opt.flat_grad[opt.numel]), steps=list(opt._host_steps), collectives=len(events),
               stats={k: v for k, v in tr.last_stats.items() if k in ("optimizer_steps", "skipped_steps")},
               pending=opt.pending, dev_steps=opt._dev_steps.tolist() if poisoned else None)
    torch.save(out, os.path.join(out_dir, f"{what}_r{rank}.pt"))
    _leave(world)


def _run(world, what, out_dir):
    mp.spawn(_worker, args=(world, _free_port(), what, out_dir), nprocs=world, join=True)
    return [torch.load(os.path.join(out_dir, f"{what}_r{r}.pt"), weights_only=False) for r in range(world)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_a_window_of_two_is_bit_equal_to_two_ranks_on_the_same_micro_batches(tmp_path):
    """(a) Two windows, i.e. two optimizer steps, so the moments of the first step are in the second."""
    one = _run(1, "window_of_two", str(tmp_path))[0]
    two = _run(2, "two_shards", str(tmp_path))
    assert one["stats"] == {"optimizer_steps": 2} and one["collectives"] == 0 and two[0]["collectives"] == 2
    assert one["weight"] == two[0]["weight"] == 8.0
    assert set(one["steps"]) == set(two[0]["steps"]) == {2}
    assert len(one["params"]) > 20
    for rank in two:
        for name, p in one["params"].items():
            assert torch.equal(_bits(p), _bits(rank["params"][name])), name
        assert one["grads"].keys() == rank["grads"].keys() and len(one["grads"]) > 20
        for name, g in one["grads"].items():         # the gradient the second update consumed
            assert torch.equal(_bits(g), _bits(rank["grads"][name])), name
    assert any(not torch.equal(p, one["start"][name]) for name, p in one["params"].items())


def test_two_ranks_with_a_window_of_two_feed_the_gradient_of_the_union_of_the_four_micro_batches(tmp_path):
    """(b) At test_gpu_multirank.py's bar and normalisation for the gradient a whole step consumed."""
    one = _run(1, "union_of_four", str(tmp_path))[0]["grads"]
    ranks = _run(2, "ranks_with_windows", str(tmp_path))
    two = ranks[0]["grads"]
    assert ranks[0]["weight"] == ranks[1]["weight"] == 16.0 and ranks[0]["collectives"] == 1
    assert ranks[0]["stats"] == {"optimizer_steps": 1} and set(ranks[0]["steps"]) == {1}
    assert one.keys() == two.keys() and len(one) > 20
    gscale = max(float(v.abs().max()) for v in one.values())

    def err(k):
        return float((two[k].double() - one[k].double()).abs().max()) / max(float(one[k].abs().max()), 1e-2 * gscale)
    record_err("two_ranks_window_of_two_vs_union_gradient", "worst tensor", max(err(k) for k in one), 1e-5)
    for k in one:
        assert err(k) < 1e-5, (k, err(k))
        assert torch.equal(_bits(ranks[0]["params"][k]), _bits(ranks[1]["params"][k])), k      # the ranks stay together


def test_six_batches_with_a_window_of_three_run_two_collectives(tmp_path):
    """(c) `parallel.collective_events` records every flat all-reduce: one per window, not one per batch."""
    ranks = _run(2, "six_batches", str(tmp_path))
    for r in ranks:
        assert r["collectives"] == 2 and r["stats"] == {"optimizer_steps": 2} and set(r["steps"]) == {2} and r["pending"] == 0
        assert r["weight"] == 24.0           # 3 global batches of 8, summed locally (12 per rank) and then over the ranks


def test_a_nan_in_one_ranks_second_micro_batch_skips_the_window_on_both_ranks(tmp_path):
    """(d) The guard reads the all-reduced buffer: every rank takes the same decision from the same bits."""
    ranks = _run(2, "poisoned", str(tmp_path))
    for r in ranks:
        assert r["stats"] == {"optimizer_steps": 1, "skipped_steps": 1} and r["collectives"] == 1
        assert set(r["dev_steps"]) == {0.0}
        for name, p in r["params"].items():
            assert torch.equal(_bits(p), _bits(r["start"][name])), name
            assert torch.equal(_bits(p), _bits(ranks[0]["params"][name])), name
