"""GPU: gradient accumulation -- `msgat_gather_accumulate{,_dev}` (a later micro-batch of a window added into the flat
gradient buffer, product and sum rounded one after the other) through `parallel.gather_scaled(accumulate=True)`, as BITS
against the float32 numpy restatement (tests/grad_accumulate_ref.py); `FlatAdam.accumulate` / `step` as bits against
`msgat_adam_step*` run directly on a flat buffer the restatement built; and `Trainer(accumulate_steps=k)` against one step on
the union of a window's micro-batches, at the shapes and bars of tests/test_gpu_multirank.py."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import grad_accumulate_ref as ref
from conftest import record_err, rel_err
from test_gpu_multirank import _model_and_batches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# one element, the block's stride and the 2048-element chunk from both sides, a tensor of three chunks
NUMELS = [1, 255, 2047, 2048, 2049, 4097]
FOREIGN = 3            # in front of this tensor lies a region of the flat buffer that belongs to a tensor outside the table
SPARE = 37


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _same_but_nan(got: torch.Tensor, want: np.ndarray) -> bool:
    """Bit for bit, except that a NaN only has to be a NaN (its payload is the hardware's)."""
    got = got.detach().cpu().numpy()
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


def _layout():
    """Offsets that are no multiple of 4 elements (4-byte aligned only), gaps between the tensors, one foreign region."""
    offsets, off = [], 3
    for i, n in enumerate(NUMELS):
        off += 300 if i == FOREIGN else 0
        off += 1 if off % 4 == 0 else 0
        offsets.append(off)
        off += n + 5
    assert all(o % 4 for o in offsets)
    return offsets, off        # off: the weight's index


def _sources(seed):
    """Gradients as views of one bank at odd element offsets: their addresses are 4-byte aligned only."""
    rng = np.random.default_rng(seed)
    bank = torch.zeros(sum(NUMELS) + 3 * len(NUMELS) + 1, device=DEV)
    out, off = [], 1
    for n in NUMELS:
        off += 1 if off % 4 == 0 else 0
        bank[off:off + n] = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
        out.append(bank[off:off + n])
        off += n + 2
    assert all(g.data_ptr() % 16 for g in out)
    return out


WEIGHTS = [0.1, 0.2, 0.3, 0.7]       # their float32 sum depends on the order


@pytest.mark.parametrize("on_device", [False, True], ids=["float_weight", "device_weight"])
def test_three_accumulations_in_a_row_have_the_bits_of_the_restatement(on_device):
    from ms_gat_amd import parallel
    offsets, widx = _layout()
    w32 = [np.float32(w) for w in WEIGHTS]
    assert ((w32[0] + w32[1]) + w32[2]) + w32[3] != ((w32[3] + w32[2]) + w32[1]) + w32[0]
    rng = np.random.default_rng(9)
    start = rng.standard_normal(widx + 1 + SPARE).astype(np.float32)      # stale contents everywhere, the weight's slot too
    flat = torch.from_numpy(start.copy()).to(DEV)
    want = start.copy()
    cache = {}
    for k, w in enumerate(WEIGHTS):
        grads = _sources(40 + k)
        if k == 2:
            grads[2][2046] = float("inf")          # the last element of a ragged chunk
        if k == 3:
            grads[4][2048] = float("nan")          # the lone element of a tensor's second chunk
        weight = torch.tensor([w], device=DEV) if on_device else w
        parallel.gather_scaled(flat[:widx + 1], grads, offsets, weight, widx, cache, accumulate=k > 0)
        (ref.accumulate if k else ref.gather)(want, [g.cpu().numpy() for g in grads], offsets, w, widx)
        assert _same_but_nan(flat, want), (k, on_device)
    assert len(cache) == 1                                                # one table for all four launches
    got = flat.cpu().numpy()
    # the weight: the float32 sum in call order
    assert got[widx] == ((w32[0] + w32[1]) + w32[2]) + w32[3]
    # Inf and NaN reached their own element only
    bad = np.flatnonzero(~np.isfinite(got))
    assert bad.tolist() == [offsets[2] + 2046, offsets[4] + 2048]
    assert np.isinf(got[offsets[2] + 2046]) and np.isnan(got[offsets[4] + 2048])
    # what the table does not name keeps its bits: the gaps, the foreign tensor's region, everything behind the weight
    untouched = np.ones(got.size, dtype=bool)
    for o, n in zip(offsets, NUMELS):
        untouched[o:o + n] = False
    untouched[widx] = False
    assert int(untouched.sum()) >= 300 + SPARE
    assert np.array_equal(got.view(np.int32)[untouched], start.view(np.int32)[untouched])


def test_a_table_that_leaves_a_tensor_out_does_not_touch_its_region():
    from ms_gat_amd import parallel
    offsets, widx = _layout()
    flat = torch.arange(widx + 1, device=DEV, dtype=torch.float32)
    before = flat.clone()
    grads = _sources(3)
    some = [0, 2, 5]
    parallel.gather_scaled(flat, [grads[i] for i in some], [offsets[i] for i in some], 2.0, -1, {}, accumulate=True)
    got, was = flat.cpu().numpy(), before.cpu().numpy()
    for i, (o, n) in enumerate(zip(offsets, NUMELS)):
        if i in some:
            assert np.array_equal(got[o:o + n], was[o:o + n] + np.float32(2.0) * grads[i].cpu().numpy())
            got[o:o + n] = was[o:o + n]
    assert np.array_equal(got, was)                    # the other tensors' regions, and (weight_index < 0) the weight


def test_bad_arguments_come_back_as_status_codes_before_anything_is_enqueued():
    from ms_gat_amd import _lib
    L = _lib.lib()
    flat = torch.full((64,), 5.0, device=DEV)
    x = C.c_void_p(flat.data_ptr())
    for n in (0, -1):
        assert L.msgat_gather_accumulate(x, x, x, n, 1.0, x, 0, None) == -2
        assert L.msgat_gather_accumulate_dev(x, x, x, n, x, x, 0, None) == -2
    for hole in (0, 1, 2, 5):
        args = [x, x, x, 1, 1.0, x, 0, None]
        args[hole] = None
        assert L.msgat_gather_accumulate(*args) == -1, hole
    for hole in (0, 1, 2, 4, 5):
        args = [x, x, x, 1, x, x, 0, None]
        args[hole] = None
        assert L.msgat_gather_accumulate_dev(*args) == -1, hole
    torch.cuda.synchronize()
    assert bool((flat == 5.0).all())


# ---- FlatAdam: a window against msgat_adam_step* on a flat buffer built by the restatement ------------------------------
NO_GRAD = 1            # this tensor (255 elements) never has a gradient


def _bank(seed):
    rng = np.random.default_rng(seed)
    bank = torch.full((sum(NUMELS) + SPARE * len(NUMELS),), float("nan"), device=DEV)
    params, off = [], 0
    for n in NUMELS:
        bank[off:off + n] = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
        params.append(torch.nn.Parameter(bank[off:off + n]))
        off += n + SPARE
    return bank, params


def _gradients(seed, params, skip=NO_GRAD, scale=1.0):
    rng = np.random.default_rng(seed)
    return [None if i == skip else torch.from_numpy((scale * rng.standard_normal(p.numel())).astype(np.float32)).to(DEV).view_as(p)
            for i, p in enumerate(params)]


def _direct_step(twin, active):
    """What FlatAdam.step launches behind a closed window, by hand: the guard (if any) and the update, dividing by the
    buffer's last element on the way in."""
    from ms_gat_amd import _lib
    L = _lib.lib()
    ptrs, offs, lens, tens, act, n, n_act = twin._table(active)
    g = twin.param_groups[0]
    stream = torch.cuda.current_stream(twin.flat_grad.device).cuda_stream
    divisor = twin.flat_grad.data_ptr() + 4 * twin.numel
    adam = (ptrs.data_ptr(), offs.data_ptr(), lens.data_ptr(), tens.data_ptr(), n, act.data_ptr(), n_act,
            twin.flat_grad.data_ptr(), twin.exp_avg.data_ptr(), twin.exp_avg_sq.data_ptr(), twin._dev_steps.data_ptr(),
            twin._dev_lr.data_ptr(), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
            divisor)
    if twin.guarded:
        max_norm = float("inf") if twin.max_grad_norm is None else twin.max_grad_norm
        _lib.check(L.msgat_grad_guard(offs.data_ptr(), lens.data_ptr(), n, twin.flat_grad.data_ptr(), divisor, max_norm,
                                      twin._guard_partials.data_ptr(), twin._guard.data_ptr(), stream), "msgat_grad_guard")
    if twin.shadow is not None:
        _lib.check(L.msgat_adam_step_averaged(*adam, twin._guard.data_ptr() if twin.guarded else 0, twin.shadow.data_ptr(),
                                              twin.ema_decay, stream), "msgat_adam_step_averaged")
    elif twin.guarded:
        _lib.check(L.msgat_adam_step_guarded(*adam, twin._guard.data_ptr(), stream), "msgat_adam_step_guarded")
    else:
        _lib.check(L.msgat_adam_step(*adam, stream), "msgat_adam_step")


OPTIONS = {"plain": {}, "guarded": dict(max_grad_norm=1.0), "averaged": dict(ema_decay=0.5),
           "guarded_averaged": dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)}


@pytest.mark.parametrize("on_device", [False, True], ids=["float_weight", "device_weight"])
@pytest.mark.parametrize("form", list(OPTIONS))
def test_a_window_leaves_the_bits_of_the_update_run_on_the_restatements_buffer(form, on_device):
    from ms_gat_amd import engine
    bank, params = _bank(1)
    bank2, params2 = _bank(1)
    opt = engine.FlatAdam(params, lr=1e-2, weight_decay=5e-4, **OPTIONS[form])
    twin = engine.FlatAdam(params2, lr=1e-2, weight_decay=5e-4, **OPTIONS[form])
    twin._build()
    active = tuple(i != NO_GRAD for i in range(len(NUMELS)))
    offsets = [o for o, on in zip(twin._offsets, active) if on]
    weights = [(5.0, 3.0), (2.0, 7.0)]
    for window, (w0, w1) in enumerate(weights):
        micro = []
        for j, w in enumerate((w0, w1)):
            grads = _gradients(100 + 2 * window + j, params)
            for p, g in zip(params, grads):
                p.grad = g
            weight = torch.tensor([w], device=DEV) if on_device else w
            if j == 0:
                assert opt.pending == 0
                opt.accumulate(weight)
                assert opt.pending == 1
            else:
                opt.step(rank_weight=weight)
                assert opt.pending == 0
            micro.append((w, [g.cpu().numpy() for g in grads if g is not None]))
        flat = twin.flat_grad.cpu().numpy()
        ref.window(flat, micro, offsets, twin.numel)
        if on_device:
            flat[twin.numel] = max(flat[twin.numel], np.float32(1.0))
        twin.flat_grad.copy_(torch.from_numpy(flat))
        assert _same(opt.flat_grad, twin.flat_grad)
        _direct_step(twin, active)
    assert _same(bank, bank2)                                   # parameters, and the NaN gaps between them
    assert _same(opt.exp_avg, twin.exp_avg) and _same(opt.exp_avg_sq, twin.exp_avg_sq)
    assert bool(torch.isfinite(opt.exp_avg_sq).all()) and float(opt.exp_avg_sq.abs().max()) > 0
    steps = [0.0 if i == NO_GRAD else 2.0 for i in range(len(NUMELS))]
    assert opt._dev_steps.tolist() == twin._dev_steps.tolist() == steps      # one window, one step
    assert opt._host_steps == [int(t) for t in steps]
    if opt.shadow is not None:
        assert _same(opt.shadow, twin.shadow) and not _same(opt.shadow, torch.cat([p.detach().reshape(-1) for p in params]))
    if opt.guarded:
        assert _same(opt._guard, twin._guard)
        stats = opt.guard_stats()
        assert stats["skipped_steps"] == 0 and 0 < stats["clip_coef"] < 1      # the norm of the MEAN gradient was clipped
    fresh = _bank(1)[0]
    assert not _same(bank, fresh)


def test_one_non_finite_micro_batch_leaves_the_whole_window_out():
    from ms_gat_amd import engine
    bank, params = _bank(2)
    opt = engine.FlatAdam(params, lr=1e-2, skip_nonfinite=True, ema_decay=0.5)
    for k, w in enumerate((4.0, 4.0)):                          # a clean window first: there is state to lose
        for p, g in zip(params, _gradients(300 + k, params)):
            p.grad = g
        opt.accumulate(w) if k == 0 else opt.step(rank_weight=w)
    before = [t.clone() for t in (bank, opt.exp_avg, opt.exp_avg_sq, opt._dev_steps, opt.shadow)]
    for k, w in enumerate((4.0, 4.0, 4.0)):
        grads = _gradients(310 + k, params)
        if k == 1:
            grads[3][17] = float("nan")
        for p, g in zip(params, grads):
            p.grad = g
        opt.accumulate(w) if k < 2 else opt.step(rank_weight=w)
    after = (bank, opt.exp_avg, opt.exp_avg_sq, opt._dev_steps, opt.shadow)
    assert all(_same(a, b) for a, b in zip(after, before))
    assert opt.guard_stats()["skipped_steps"] == 1              # one window, one skipped step


def test_a_changed_active_set_and_calls_that_need_a_closed_window_are_refused():
    from ms_gat_amd import engine
    bank, params = _bank(3)
    opt = engine.FlatAdam(params, lr=1e-2, ema_decay=0.5)
    opt.param_names = {id(p): f"tensor{i}" for i, p in enumerate(params)}
    for p, g in zip(params, _gradients(400, params)):
        p.grad = g
    opt.accumulate(4.0)
    assert opt.pending == 1
    for call in (opt.state_dict, opt.swap_averaged, opt.averaged_state):
        with pytest.raises(RuntimeError, match="accumulation window"):
            call()
    assert not opt.swapped
    for p, g in zip(params, _gradients(401, params, skip=4)):   # tensor 1 gains a gradient, tensor 4 loses its own
        p.grad = g
    with pytest.raises(RuntimeError, match="tensor1 "):
        opt.step(rank_weight=4.0)
    with pytest.raises(RuntimeError, match="tensor1 "):
        opt.accumulate(4.0)
    assert opt.pending == 1
    with pytest.raises(ValueError):                             # a device count in a window of sample counts
        for p, g in zip(params, _gradients(402, params)):
            p.grad = g
        opt.accumulate(torch.tensor([4.0], device=DEV))
    opt.step(rank_weight=4.0)                                   # the window closes; everything is allowed again
    assert opt.pending == 0 and opt._host_steps == [1, 0, 1, 1, 1, 1]
    opt.state_dict(), opt.averaged_state()
    with opt.averaged_parameters():
        pass


# ---- Trainer(accumulate_steps=k) at the shapes of test_gpu_multirank.py: N = 40, micro-batches of 4 -----------------------
def _union(batches):
    return [torch.cat([b[i] for b in batches]) for i in range(4)]


def _mask_truth(batch, seed, keep=0.3):
    """Most of the truth becomes the null value 0: a micro-batch with a small valid count."""
    alive = torch.rand(batch[3].shape, generator=torch.Generator().manual_seed(seed)) < keep
    batch[3] = torch.where(alive, batch[3], torch.zeros(()))
    return batch


def _one_epoch(tmp_path, name, sizes, masked, union=False, only=None, **kw):
    """A fresh copy of the model (the same in every call), one training epoch; the gradient the LAST update consumed per
    parameter, the parameters after it, and the trainer."""
    from ms_gat_amd import engine
    net, batches = _model_and_batches(sizes)
    if masked:
        batches[0] = _mask_truth(batches[0], 5)
    if only is not None:
        batches = [batches[only]]
    if union:
        batches = [_union(batches)]
    tr = engine.Trainer(net, 50.0, str(tmp_path / name), hip_graph=False, null_value=0.0 if masked else None, **kw)
    assert isinstance(tr.optimizer, engine.FlatAdam)
    tr.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
    opt = tr.optimizer
    flat = opt.flat_grad[: opt.numel]
    if tr.accumulate_steps > 1:
        flat = flat / opt.flat_grad[opt.numel]
    names = {id(p): n for n, p in net.named_parameters()}
    grads = {names[id(p)]: flat[o:o + p.numel()].view_as(p).detach().cpu() for p, o in zip(opt._params, opt._offsets)}
    return grads, {k: v.detach().cpu() for k, v in net.named_parameters()}, tr


def _gradient_errors(one, two):
    """test_gpu_multirank.py's normalisation: per tensor on its own scale, tensors more than 100x below the largest gradient
    on that scale."""
    gscale = max(float(v.abs().max()) for v in one.values())
    return {k: float((two[k].double() - one[k].double()).abs().max()) / max(float(one[k].abs().max()), 1e-2 * gscale)
            for k in one}


@pytest.mark.parametrize("sizes,masked", [((4, 4), False), ((4, 4, 3), False), ((4, 4), True)],
                         ids=["2x4", "ragged_4_4_3", "masked_2x4"])
def test_a_window_feeds_the_optimizer_the_gradient_of_the_union_batch(tmp_path, sizes, masked):
    want, want_params, single = _one_epoch(tmp_path, "union", sizes, masked, union=True)
    got, got_params, tr = _one_epoch(tmp_path, "window", sizes, masked, accumulate_steps=len(sizes))
    assert tr.last_stats["optimizer_steps"] == 1 and "optimizer_steps" not in single.last_stats
    assert tr.optimizer.pending == 0 and set(tr.optimizer._host_steps) == set(single.optimizer._host_steps) == {1}
    assert want.keys() == got.keys() and len(want) > 20
    errs = _gradient_errors(want, got)
    record_err(f"window_vs_union_gradient_{'masked_' if masked else ''}{'+'.join(map(str, sizes))}", "worst tensor",
               max(errs.values()), 1e-5)
    for k, e in errs.items():
        assert e < 1e-5, (k, e)
        if float(want[k].abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
    for name, p in want_params.items():          # Adam's first step is sign-like: that file's bar for parameters
        assert rel_err(got_params[name], p) < 2e-2, name
    total = float(tr.optimizer.flat_grad[tr.optimizer.numel])
    if not masked:
        assert total == float(sum(sizes))
        return
    # the weights were the valid counts, and they were unequal: the plain mean of the two gradients is another gradient
    counts = []
    halves = []
    for i in range(2):
        g, _, t = _one_epoch(tmp_path, f"alone{i}", sizes, masked, only=i)
        counts.append(float(t._valid_count))
        halves.append(g)
    assert total == sum(counts) and counts[0] < 0.5 * counts[1]
    mean = {k: (halves[0][k] + halves[1][k]) / 2 for k in want}
    assert max(_gradient_errors(want, mean).values()) > 1e-2
    weighted = {k: (counts[0] * halves[0][k] + counts[1] * halves[1][k]) / total for k in want}
    assert max(_gradient_errors(want, weighted).values()) < 1e-5


def test_captured_micro_batches_with_an_eager_tail_track_the_eager_run(tmp_path):
    """hip_graph=True with a window of 2: the graph ends after backward, accumulate / step run eagerly on the gradients the
    capture owns.  Compared as test_gpu_model.py compares its captured and eager training runs."""
    from ms_gat_amd import engine
    net, batches = _model_and_batches((4,) * 8)
    assert len(batches) == 8
    twin = copy.deepcopy(net)
    eager = engine.Trainer(net, 50.0, str(tmp_path / "eager"), hip_graph=False, accumulate_steps=2)
    graphed = engine.Trainer(twin, 50.0, str(tmp_path / "graph"), hip_graph=True, accumulate_steps=2)
    for epoch in (1, 2, 3):
        le = eager.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        lg = graphed.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train")
        assert abs(le - lg) < 1e-4 * abs(le), (epoch, le, lg)
        assert eager.last_stats["optimizer_steps"] == graphed.last_stats["optimizer_steps"] == 4
    assert len(graphed._graphs) == 1
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, name
    ve = eager.run_epoch(batches[:2], gpu_id=0, epoch=3, mode="validate")
    vg = graphed.run_epoch(batches[:2], gpu_id=0, epoch=3, mode="validate")
    assert abs(ve - vg) < 1e-4 * abs(ve)
    assert set(graphed.optimizer._dev_steps.tolist()) == {12.0}
    assert set(graphed.optimizer._host_steps) == set(eager.optimizer._host_steps) == {12}
    assert graphed.optimizer.pending == eager.optimizer.pending == 0
    line = open(graphed.log_file).read().splitlines()[0]
    assert line.endswith("optimizer_steps=4")
    graphed.save(str(tmp_path / "ckpt.pkl"))                    # nothing is pending between epochs: checkpoints as ever
    assert sorted(torch.load(str(tmp_path / "ckpt.pkl"), weights_only=False)) == ["best", "epoch", "grad_scaler", "model",
                                                                                 "optimizer", "scheduler"]


def test_the_two_micro_batches_of_a_window_draw_different_edge_masks(tmp_path):
    """The same four samples twice in one window: with one mask for both, the second gradient would be the first, and the
    buffer 4 g + 4 g = 8 g to the bit (both operations are exact then).  It is not, and the stream advanced twice."""
    from ms_gat_amd import data, engine, model

    def build():
        torch.manual_seed(0)
        ds = data.SyntheticPEMS(n_nodes=40, n_edges=50, n_channels=1, in_hours=[1, 2], batch_size=8, days=2)
        net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj,
                            edge_dropout=0.1, edge_dropout_seed=5)
        return net.to(DEV), [t[:4] for t in next(iter(ds.training))]

    net, batch = build()
    alone = engine.Trainer(net, 50.0, str(tmp_path / "alone"), hip_graph=False)
    alone.run_epoch([batch], gpu_id=0, epoch=1, mode="train")
    g = alone.optimizer.flat_grad[: alone.optimizer.numel].clone()
    assert net.edge_dropout_state() == {"seed": 5, "step": 1}
    net, batch = build()
    tr = engine.Trainer(net, 50.0, str(tmp_path / "window"), hip_graph=False, accumulate_steps=2)
    tr.run_epoch([batch, batch], gpu_id=0, epoch=1, mode="train")
    assert net.edge_dropout_state() == {"seed": 5, "step": 2}
    opt = tr.optimizer
    assert float(opt.flat_grad[opt.numel]) == 8.0
    assert not torch.equal(opt.flat_grad[: opt.numel], 8.0 * g)
    assert rel_err(opt.flat_grad[: opt.numel], 8.0 * g) > 1e-3
