"""GPU: the guard on the optimizer step -- `msgat_grad_guard` (global gradient norm in double, clipping coefficient,
finite flag, all left in device memory) and `msgat_adam_step_guarded` -- through `FlatAdam(max_grad_norm, skip_nonfinite)`,
a captured step and `Trainer`, against `torch.nn.utils.clip_grad_norm_` + `torch.optim.Adam`.

The parameter sizes straddle the 2048-element chunk edge (9 chunks, the last one ragged: 4100 = 2 * 2048 + 4)."""
import copy
import math

import pytest
import torch
from torch import nn, optim

from conftest import record_err, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (2047,), (2048,), (2049,), (3, 5), (4100,)]
INF, NAN = float("inf"), float("nan")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _param_set():
    torch.manual_seed(3)
    return [nn.Parameter(torch.randn(s, device=_dev())) for s in SHAPES]


def _grads(gen, scale=1.0):
    return [torch.randn(s, device=_dev(), generator=gen) * scale for s in SHAPES]


def _set(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()


def _norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))


def _coef32(max_norm, norm):
    """clip_grad_norm_'s coefficient, in the fp32 arithmetic torch runs it in."""
    c = torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(norm, dtype=torch.float32) + 1e-6)
    return float(torch.clamp(c, max=1.0))


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _state(opt, params):
    """Everything a step may write, bit for bit."""
    return ([_bits(p) for p in params], _bits(opt.exp_avg), _bits(opt.exp_avg_sq), _bits(opt._dev_steps))


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


# ---- the norm ---------------------------------------------------------------------------------------------------------------
def test_norm_matches_float64_and_repeats_bit_for_bit():
    from ms_gat_amd import engine
    params = _param_set()
    opt = engine.FlatAdam(params, lr=1e-3, weight_decay=5e-4, max_grad_norm=1.0)
    gen = torch.Generator(device=_dev()).manual_seed(4)
    for scale in (1.0, 1e-3, 37.0):
        grads = _grads(gen, scale)
        _set(params, grads)
        opt.step()
        first = _bits(opt._guard)
        got, want = opt.guard_stats(), _norm64(grads)
        e = abs(got["grad_norm"] - want) / want
        record_err("guarded step: gradient norm vs float64", f"scale {scale:g}", e, 1e-6)
        print(f"scale {scale:g}: norm {got['grad_norm']!r} float64 {want!r} rel err {e:.2e} coef {got['clip_coef']!r}")
        assert e < 1e-6
        assert got["clip_coef"] == _coef32(1.0, got["grad_norm"]) and got["skipped_steps"] == 0
        opt.step()                                  # the same gradients again: the same bits
        again = _bits(opt._guard)
        assert torch.equal(first[:2], again[:2]) and torch.equal(first[4:], again[4:])
    assert opt.guard_stats()["grad_norm_max"] == pytest.approx(_norm64(grads), rel=1e-6)     # the last scale is the largest
    opt.reset_guard_stats()
    assert opt.guard_stats()["grad_norm_max"] == 0.0


def test_gradient_entries_of_1e30_give_a_finite_norm_and_a_clipped_step():
    """fp32 squares of 1e30 overflow; the sum of squares is taken in double, so the step is clipped, not left out."""
    from ms_gat_amd import engine
    params = _param_set()
    before = [p.detach().clone() for p in params]
    opt = engine.FlatAdam(params, lr=1e-3, weight_decay=5e-4, max_grad_norm=2.0, skip_nonfinite=True)
    grads = _grads(torch.Generator(device=_dev()).manual_seed(5))
    grads[3][7] = 1e30
    grads[5][4099] = -1e30
    grads[0][0] = 1e30
    _set(params, grads)
    opt.step()
    got, want = opt.guard_stats(), _norm64(grads)
    e = abs(got["grad_norm"] - want) / want
    print(f"1e30 entries: norm {got['grad_norm']!r} float64 {want!r} rel err {e:.2e} coef {got['clip_coef']!r}")
    assert math.isfinite(got["grad_norm"]) and e < 1e-6
    assert got["skipped_steps"] == 0 and 0.0 < got["clip_coef"] < 1e-29 and got["clip_coef"] == _coef32(2.0, got["grad_norm"])
    assert opt._dev_steps.tolist() == [1.0] * len(SHAPES)
    for p, old in zip(params, before):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), old)
    assert bool(torch.isfinite(opt.exp_avg).all()) and bool(torch.isfinite(opt.exp_avg_sq).all())


def test_stale_flat_contents_of_a_parameter_without_a_gradient_are_not_read():
    """Step 1 leaves a NaN and large values of parameter 2 in the flat buffer (and is left out for the NaN); on step 2 that
    parameter has no gradient: the norm is that of the others, and the step is taken."""
    from ms_gat_amd import engine
    params = _param_set()
    opt = engine.FlatAdam(params, lr=1e-3, weight_decay=5e-4, max_grad_norm=1.0)
    gen = torch.Generator(device=_dev()).manual_seed(6)
    grads = _grads(gen)
    grads[2] = grads[2] * 1e4
    grads[2][5] = NAN
    _set(params, grads)
    opt.step()
    assert opt.guard_stats()["skipped_steps"] == 1
    lo = opt._offsets[2]
    assert bool(torch.isnan(opt.flat_grad[lo + 5])) and float(opt.flat_grad[lo + 6].abs()) > 0      # stale, still there
    grads = _grads(gen)
    grads[2] = None
    _set(params, grads)
    opt.step()
    got, want = opt.guard_stats(), _norm64(grads)
    assert got["skipped_steps"] == 1 and abs(got["grad_norm"] - want) / want < 1e-6
    assert opt._dev_steps.tolist() == [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]


# ---- against torch, step for step ---------------------------------------------------------------------------------------------
def test_guarded_flat_adam_tracks_clip_grad_norm_and_torch_adam_step_for_step():
    """Bars of test_flat_adam_tracks_torch_adam_step_for_step: 1e-6 on the parameters and both moments."""
    from ms_gat_amd import engine
    max_norm = 5.0
    ours, theirs = _param_set(), _param_set()
    a = engine.FlatAdam(ours, lr=1e-3, weight_decay=5e-4, max_grad_norm=max_norm)
    b = optim.Adam(theirs, lr=1e-3, weight_decay=5e-4)
    gen = torch.Generator(device=_dev()).manual_seed(9)
    clipped = []
    for step, scale in enumerate((1e-3, 1e-2, 1.0, 3e-2, 10.0, 2e-2, 0.1, 1e-2)):     # norms ~ 100 * scale
        grads = _grads(gen, scale)
        if step == 3:                                   # torch's Adam skips parameters without a gradient
            grads[1] = None
        _set(ours, grads)
        _set(theirs, grads)
        a.step()
        norm = float(nn.utils.clip_grad_norm_(theirs, max_norm))
        b.step()
        got = a.guard_stats()
        assert abs(got["grad_norm"] - norm) < 1e-5 * norm       # torch adds fp32 norms of fp32 norms
        clipped.append(got["clip_coef"] < 1.0)
        assert clipped[-1] == (norm + 1e-6 > max_norm)
    assert clipped == [False, False, True, False, True, False, True, False]
    for i, (p, q) in enumerate(zip(ours, theirs)):
        e = rel_err(p.detach(), q.detach())
        record_err("guarded FlatAdam vs clip_grad_norm_ + torch.optim.Adam, 8 steps", f"param{i}{tuple(p.shape)}", e, 1e-6)
        assert e < 1e-6, i
        assert rel_err(a.state[p]["exp_avg"], b.state[q]["exp_avg"]) < 1e-6
        assert rel_err(a.state[p]["exp_avg_sq"], b.state[q]["exp_avg_sq"]) < 1e-6
    assert a._dev_steps.tolist() == [8.0, 7.0, 8.0, 8.0, 8.0, 8.0] and a.guard_stats()["skipped_steps"] == 0


@pytest.mark.parametrize("options", [dict(max_grad_norm=1e30), dict(skip_nonfinite=True)], ids=["huge_max_norm", "skip_only"])
def test_a_coefficient_of_one_gives_the_bits_of_the_unguarded_step(options):
    from ms_gat_amd import engine
    ours, plain = _param_set(), _param_set()
    a = engine.FlatAdam(ours, lr=1e-3, weight_decay=5e-4, **options)
    b = engine.FlatAdam(plain, lr=1e-3, weight_decay=5e-4)
    assert a.guarded and not b.guarded and b._guard is None
    gen = torch.Generator(device=_dev()).manual_seed(10)
    for step in range(4):
        grads = _grads(gen, 10.0 ** step)
        if step == 2:
            grads[4] = None
        _set(ours, grads)
        _set(plain, grads)
        a.step()
        b.step()
        assert a.guard_stats()["clip_coef"] == 1.0
    assert _same(_state(a, ours), _state(b, plain))
    assert len(b.buffer_token()) == 5 and len(a.buffer_token()) == 7      # the guard's buffers join the token
    with pytest.raises(RuntimeError):
        b.guard_stats()


# ---- non-finite gradients -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first_of_first_chunk", "last_of_ragged_last_chunk"])
@pytest.mark.parametrize("bad", [NAN, INF], ids=["nan", "inf"])
def test_a_non_finite_gradient_leaves_the_step_out_and_the_next_one_is_as_if_it_never_came(bad, where):
    from ms_gat_amd import engine
    ours, theirs = _param_set(), _param_set()
    a = engine.FlatAdam(ours, lr=1e-3, weight_decay=5e-4, max_grad_norm=50.0, skip_nonfinite=True)
    b = optim.Adam(theirs, lr=1e-3, weight_decay=5e-4)
    gen = torch.Generator(device=_dev()).manual_seed(12)

    def both(scale):
        grads = _grads(gen, scale)
        _set(ours, grads)
        _set(theirs, grads)
        a.step()
        nn.utils.clip_grad_norm_(theirs, 50.0)
        b.step()

    both(0.1)
    both(2.0)
    before = _state(a, ours)
    grads = _grads(gen)
    if where == "first_of_first_chunk":
        grads[0][0] = bad
    else:
        grads[5][4099] = bad
    _set(ours, grads)
    a.step()                                            # torch never sees this one
    stats = a.guard_stats()
    assert _same(_state(a, ours), before)
    assert stats["skipped_steps"] == 1 and stats["clip_coef"] == 0.0 and not math.isfinite(stats["grad_norm"])
    assert a._dev_steps.tolist() == [2.0] * len(SHAPES)
    both(1.0)
    for i, (p, q) in enumerate(zip(ours, theirs)):
        assert rel_err(p.detach(), q.detach()) < 1e-6, i
        assert rel_err(a.state[p]["exp_avg"], b.state[q]["exp_avg"]) < 1e-6
        assert rel_err(a.state[p]["exp_avg_sq"], b.state[q]["exp_avg_sq"]) < 1e-6
    assert a.guard_stats()["skipped_steps"] == 1
    # the checkpoint carries the device's step counts (the host launched four steps, three were taken)
    sd = a.state_dict()
    assert [float(sd["state"][i]["step"]) for i in range(len(SHAPES))] == [3.0] * len(SHAPES)
    assert [float(b.state[q]["step"]) for q in theirs] == [3.0] * len(SHAPES)
    assert a._dev_steps.tolist() == [3.0] * len(SHAPES) and a._host_steps == [3] * len(SHAPES)


# ---- capture ------------------------------------------------------------------------------------------------------------------
def test_one_captured_guarded_step_replays_finite_and_non_finite_batches_like_eager_steps():
    """The decision is read from device memory by the captured kernels: ONE graph, replayed with finite, NaN and finite
    gradients, equals the eager sequence bit for bit (parameters, moments, step counts and the guard state)."""
    from ms_gat_amd import engine
    eager_p, graph_p = _param_set(), _param_set()
    eager = engine.FlatAdam(eager_p, lr=1e-3, weight_decay=5e-4, max_grad_norm=20.0, skip_nonfinite=True)
    graphed = engine.FlatAdam(graph_p, lr=1e-3, weight_decay=5e-4, max_grad_norm=20.0, skip_nonfinite=True)
    gen = torch.Generator(device=_dev()).manual_seed(13)
    static = [torch.zeros(s, device=_dev()) for s in SHAPES]
    for p, g in zip(graph_p, static):
        p.grad = g                                      # the captured copy reads these addresses
    sequence = [_grads(gen, 0.05), _grads(gen, 3.0), _grads(gen, 1.0), _grads(gen, 0.3)]
    sequence[2][3][2048] = NAN                          # the first element of parameter 3's second chunk

    def feed(grads):
        for dst, src in zip(static, grads):
            dst.copy_(src)

    # warm-up on a side stream: builds the flat buffers, the chunk tables and the guard before the capture
    feed(sequence[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.step()
    torch.cuda.current_stream().wait_stream(side)
    _set(eager_p, sequence[0])
    eager.step()
    token = graphed.buffer_token()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    assert graphed.buffer_token() == token
    for grads in sequence[1:]:
        feed(grads)
        graph.replay()
        _set(eager_p, grads)
        eager.step()
    torch.cuda.synchronize()
    assert _same(_state(graphed, graph_p), _state(eager, eager_p))
    assert torch.equal(_bits(graphed._guard), _bits(eager._guard))
    stats = graphed.guard_stats()
    assert stats["skipped_steps"] == 1 and graphed._dev_steps.tolist() == [3.0] * len(SHAPES)
    assert stats["grad_norm"] == pytest.approx(_norm64(sequence[3]), rel=1e-6)
    assert stats["grad_norm_max"] == pytest.approx(_norm64(sequence[1]), rel=1e-6) and stats["clip_coef"] < 1.0
    assert [float(graphed.state_dict()["state"][i]["step"]) for i in range(len(SHAPES))] == [3.0] * len(SHAPES)


# ---- Trainer --------------------------------------------------------------------------------------------------------------------
def _small_model_and_batches():
    from ms_gat_amd import data, model
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=40, n_edges=50, n_channels=1, in_hours=[1, 2], batch_size=8, days=2)
    net = model.msgat48(n_components=2, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj)
    batches = [[t.clone() for t in b] for _, b in zip(range(5), ds.training)]
    for i in (0, 3):      # a reading of NaN in X (`null_value` masks the truth, not the inputs); batch 0 is also the one
        batches[i][0].view(-1)[17 + i] = NAN          # the capture warms up on, twice, before its first replay
    return net.to(_dev()), batches


def test_trainer_with_the_guard_skips_poisoned_batches_eagerly_and_in_a_hip_graph(tmp_path):
    from ms_gat_amd import engine
    net, batches = _small_model_and_batches()
    twin = copy.deepcopy(net)
    runs = {}
    for name, model_, hip_graph in (("eager", net, False), ("graph", twin, True)):
        tr = engine.Trainer(model_, 50.0, str(tmp_path / name), hip_graph=hip_graph, max_grad_norm=1.0, skip_nonfinite=True)
        assert tr.optimizer.guarded
        tr.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
        runs[name] = tr
        assert tr.last_stats["skipped_steps"] == 2, name
        assert math.isfinite(tr.last_stats["grad_norm_max"]) and tr.last_stats["grad_norm_max"] > 0, name
        assert set(tr.optimizer._dev_steps.tolist()) == {3.0}, name
        assert all(bool(torch.isfinite(p).all()) for p in model_.parameters()), name
        assert {float(st["step"]) for st in tr.optimizer.state_dict()["state"].values()} == {3.0}, name
        lines = open(tr.log_file).read().splitlines()
        assert len(lines) == 2 and "[Train   ] - guard - epoch=1,skipped_steps=2,grad_norm_max=" in lines[1], name
    assert len(runs["graph"]._graphs) == 1
    worst = 0.0
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        e = rel_err(q.detach(), p.detach())
        worst = max(worst, e)
        assert e < 1e-5, (name, e)
    record_err("guarded Trainer: hip graph vs eager, 5 batches (2 poisoned)", "worst parameter", worst, 1e-5)
    print(f"hip graph vs eager: worst parameter rel err {worst:.2e}; grad_norm_max "
          f"{runs['eager'].last_stats['grad_norm_max']!r} / {runs['graph'].last_stats['grad_norm_max']!r}")
    assert runs["eager"].last_stats["grad_norm_max"] == pytest.approx(runs["graph"].last_stats["grad_norm_max"], rel=1e-5)
    # a second, clean epoch reports no skipped step; the cumulative count stays
    runs["graph"].run_epoch(batches[1:3], gpu_id=0, epoch=2, mode="train")
    assert runs["graph"].last_stats["skipped_steps"] == 0 and runs["graph"].guard_stats()["skipped_steps"] == 2


def test_new_flat_buffers_keep_the_guard_counts():
    """A rebuild that allocates new buffers (another layout or device) carries the cumulative skipped count along: the
    engine's per-epoch figure is a difference of cumulative counts."""
    from ms_gat_amd import engine
    params = _param_set()
    opt = engine.FlatAdam(params, lr=1e-3, weight_decay=5e-4, skip_nonfinite=True)
    grads = _grads(torch.Generator(device=_dev()).manual_seed(14))
    grads[4][1, 2] = NAN
    _set(params, grads)
    opt.step()
    token = opt.buffer_token()
    assert opt.guard_stats()["skipped_steps"] == 1
    opt.flat_grad = None                                # what a move to another device amounts to: nothing to re-use
    grads[4][1, 2] = 0.5
    _set(params, grads)
    opt.step()
    stats = opt.guard_stats()
    assert opt.buffer_token() != token and stats["skipped_steps"] == 1 and stats["clip_coef"] == 1.0
    assert opt._dev_steps.tolist() == [1.0] * len(SHAPES)
