"""GPU: the guarded optimizer step with TWO ranks on one MI355X (fresh child processes sharing cuda:0 over gloo, as in
tests/test_gpu_multirank.py): the norm is taken after the one all-reduce, from `sum_r w_r g_r` and its clamped divisor,
so it is the norm of the global batch's mean gradient and every rank takes the same decision from the same bits -- a NaN
on one rank leaves the step out on both.  Shards are uneven: 7 = 4 + 3 samples."""
import copy
import math
import os
import time

import pytest
import torch
import torch.multiprocessing as mp

from conftest import record_err, rel_err
from test_gpu_multirank import _free_port, _join, _leave, _model_and_batches

pytestmark = pytest.mark.gpu

SIZE = 7
MAX_NORM = 0.25         # far below the gradient norm of a first step of the small model: the step is clipped
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


def _step_worker(rank, world, port, out_dir, poison):
    """ONE guarded training step through engine.Trainer on the rank's shard of a 7-sample batch.  Every rank stores what
    it ended with.  Beside it a twin takes the step spelled out in torch -- `clip_grad_norm_` + `optim.Adam` -- from
    the whole (global) batch's mean gradient, the one the update consumed (flat[:numel] / flat[numel] after the
    collective); world 1 also stores the norm of its whole-batch gradient as backward left it."""
    from ms_gat_amd import engine
    net, batches = _model_and_batches((SIZE,))
    if poison:       # sample 5 belongs to rank 1's shard (samples 4..6)
        batches[0][0][5].view(-1)[11] = float("nan")
    _join(rank, world, port)
    twin = copy.deepcopy(net)
    before = [p.detach().clone() for p in net.parameters()]
    tr = engine.Trainer(net, 50.0, os.path.join(out_dir, f"w{world}r{rank}"), hip_graph=False, max_grad_norm=MAX_NORM,
                        skip_nonfinite=True)
    tr.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
    opt = tr.optimizer
    stats = opt.guard_stats()
    out = dict(stats=stats, epoch_stats={k: tr.last_stats[k] for k in ("skipped_steps", "grad_norm_max")},
               params=[p.detach().cpu() for p in net.parameters()],
               unchanged=all(torch.equal(p.detach(), q) for p, q in zip(net.parameters(), before)),
               steps=opt._dev_steps.tolist())
    if not poison:
        consumed = opt.flat_grad[: opt.numel] / opt.flat_grad[opt.numel] if world > 1 else opt.flat_grad[: opt.numel]
        fed = {id(p): consumed[o:o + p.numel()].view_as(p) for p, o in zip(opt._params, opt._offsets)}
        ref = torch.optim.Adam(twin.parameters(), lr=1e-3, weight_decay=5e-4)
        active = {id(p) for p, on in zip(opt._params, opt._last_active) if on}      # not the frozen adjacency
        for p, q in zip(net.parameters(), twin.parameters()):
            q.grad = fed[id(p)].clone() if id(p) in active else None
        out["whole_batch_norm"] = math.sqrt(sum(float((q.grad.double() ** 2).sum()) for q in twin.parameters()
                                                if q.grad is not None))
        out["torch_norm"] = float(torch.nn.utils.clip_grad_norm_(list(twin.parameters()), MAX_NORM))
        ref.step()
        out["worst_param"] = max(rel_err(p.detach(), q.detach()) for p, q in zip(net.parameters(), twin.parameters()))
        out["twin_params"] = [q.detach().cpu() for q in twin.parameters()]
    torch.save(out, os.path.join(out_dir, f"step_w{world}_r{rank}_p{int(poison)}.pt"))
    _leave(world)


def _load(out_dir, world, rank, poison):
    return torch.load(os.path.join(out_dir, f"step_w{world}_r{rank}_p{int(poison)}.pt"), weights_only=False)


def test_two_rank_guarded_step_clips_by_the_norm_of_the_global_batch_gradient(tmp_path):
    """(1) The norm the two ranks clip by against the float64 norm of the single process's whole-batch gradient, to the
    1e-5 of test_whole_step_gradient_of_two_ranks_equals_the_single_process_gradient (only the summation order over the
    batch differs).  (2) The parameters after the step against `clip_grad_norm_` + `optim.Adam` on the whole batch's
    gradient, to 1e-6.  As in `_branch_worker` of tests/test_gpu_multirank.py, torch is fed the whole-batch gradient the
    update consumed: Adam's first step moves an entry by ~lr * sign(g), so an entry whose gradient is rounding noise steps
    either way once the batch is summed in another order, and parameters of two such runs agree to ~lr only -- with the
    same gradient in, they must agree to rounding.  (1) is what ties that gradient to the single process's.  The
    parameters of the single process's own guarded step are compared on the side and printed, not asserted."""
    out = str(tmp_path)
    _spawn(_step_worker, (1, _free_port(), out, False), 1)
    _spawn(_step_worker, (2, _free_port(), out, False), 2)
    one, two0, two1 = _load(out, 1, 0, False), _load(out, 2, 0, False), _load(out, 2, 1, False)
    want = one["whole_batch_norm"]
    e_norm = abs(two0["stats"]["grad_norm"] - want) / want
    side = max(rel_err(a, b) for a, b in zip(two0["params"], one["params"]))
    print(f"norm: two ranks {two0['stats']['grad_norm']!r}, one process {one['stats']['grad_norm']!r}, whole batch in float64 "
          f"{want!r}: rel err {e_norm:.2e}; coef {two0['stats']['clip_coef']!r}; parameters vs torch {two0['worst_param']:.2e} "
          f"(rank 1 {two1['worst_param']:.2e}, one process {one['worst_param']:.2e}); two ranks vs one process {side:.2e}")
    record_err("guarded two-rank step", "norm vs whole-batch gradient", e_norm, 1e-5)
    record_err("guarded two-rank step", "parameters vs clip_grad_norm_ + Adam", two0["worst_param"], 1e-6)
    assert want > 2 * MAX_NORM                                  # the step is a clipped one
    assert e_norm < 1e-5
    assert abs(one["stats"]["grad_norm"] - want) < 1e-6 * want
    for r in (one, two0, two1):
        assert r["stats"]["skipped_steps"] == 0 and 0.0 < r["stats"]["clip_coef"] < 0.5
        assert abs(r["stats"]["grad_norm"] - r["torch_norm"]) < 1e-5 * r["torch_norm"]
        assert r["worst_param"] < 1e-6
        assert set(r["steps"]) == {1.0} and not r["unchanged"]
    # the same all-reduced bits on both ranks: the same norm, the same coefficient, the same parameters
    assert two0["stats"] == two1["stats"]
    assert all(torch.equal(a, b) for a, b in zip(two0["params"], two1["params"]))


def test_a_nan_on_one_rank_leaves_the_step_out_on_both(tmp_path):
    out = str(tmp_path)
    _spawn(_step_worker, (2, _free_port(), out, True), 2)
    two0, two1 = _load(out, 2, 0, True), _load(out, 2, 1, True)
    for r in (two0, two1):
        assert r["unchanged"]                                   # bit for bit what the step started from
        assert r["stats"]["skipped_steps"] == 1 and r["epoch_stats"]["skipped_steps"] == 1
        assert not math.isfinite(r["stats"]["grad_norm"]) and r["stats"]["clip_coef"] == 0.0
        assert set(r["steps"]) == {0.0}
    assert all(torch.equal(a, b) for a, b in zip(two0["params"], two1["params"]))
