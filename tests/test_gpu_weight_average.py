"""GPU: the averaged weights -- `msgat_adam_step_averaged` (the Adam update that also moves a flat shadow of the parameters)
and `msgat_param_swap` (parameters and shadow exchanged in place) -- through `FlatAdam(ema_decay=...)`, the guard, captured
steps and validation on the averaged weights.  The shadow is compared as BITS with the float32 numpy restatement
(tests/weight_average_ref.py) driven by the parameters read back after every step; parameters and moments as bits with a
second `FlatAdam` without the average."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import weight_average_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 12
# the block's stride (256) and the 2048-element chunk, each met from both sides, and a tensor of three chunks
NUMELS = [1, 255, 256, 257, 2047, 2048, 2049, 4097]
NO_GRAD = 3            # this tensor (257 elements) never has a gradient
SPARE = 64             # NaN-filled elements behind every tensor and behind every flat buffer


def _bank(seed):
    """Parameters as views of one NaN-filled bank with SPARE elements between them (odd offsets: 4-byte aligned only)."""
    rng = np.random.default_rng(seed)
    bank = torch.full((sum(NUMELS) + SPARE * len(NUMELS),), float("nan"), device=DEV)
    params, spans, off = [], [], 0
    for n in NUMELS:
        bank[off:off + n] = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
        params.append(torch.nn.Parameter(bank[off:off + n]))
        spans.append((off, n))
        off += n + SPARE
    return bank, params, spans


def _gaps_are_nan(bank, spans):
    keep = torch.ones_like(bank, dtype=torch.bool)
    for off, n in spans:
        keep[off:off + n] = False
    return bool(torch.isnan(bank[keep]).all()) and int(keep.sum()) == SPARE * len(spans)


def _give_tails(opt):
    """Move the flat state buffers into NaN-tailed ones: what lies behind a buffer must stay NaN."""
    opt._build()
    tails = {}
    for name in ("exp_avg", "exp_avg_sq", "shadow"):
        old = getattr(opt, name)
        if old is None:
            continue
        big = torch.full((opt.numel + SPARE,), float("nan"), device=DEV)
        big[:opt.numel].copy_(old)
        setattr(opt, name, big[:opt.numel])
        tails[name] = big
    return tails


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _gradients(seed, params, skip=NO_GRAD):
    rng = np.random.default_rng(seed)
    return [None if i == skip else torch.from_numpy(rng.standard_normal(p.numel()).astype(np.float32)).to(DEV).view_as(p)
            for i, p in enumerate(params)]


@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_shadow_has_the_bits_of_the_restatement_and_adam_the_bits_of_the_plain_update(decay):
    from ms_gat_amd import engine
    bank, params, spans = _bank(1)
    bank2, params2, spans2 = _bank(1)
    opt = engine.FlatAdam(params, lr=1e-2, weight_decay=5e-4, ema_decay=decay)
    plain = engine.FlatAdam(params2, lr=1e-2, weight_decay=5e-4)
    tails, tails2 = _give_tails(opt), _give_tails(plain)
    assert sorted(tails) == ["exp_avg", "exp_avg_sq", "shadow"] and sorted(tails2) == ["exp_avg", "exp_avg_sq"]
    start = [p.detach().cpu().numpy().copy() for p in params]
    assert all(ref.same_bits(e.cpu().numpy(), s) for e, s in zip(opt._shadow_views(), start))     # it starts at the parameters
    want = [s.copy() for s in start]
    for k in range(K):
        for ps, o in ((params, opt), (params2, plain)):
            for p, g in zip(ps, _gradients(100 + k, ps)):
                p.grad = g
            o.step()
        for i, p in enumerate(params):                       # the parameters after this step drive the restatement
            if p.grad is not None:
                want[i] = ref.average_f32(want[i], p.detach().cpu().numpy(), decay, k + 1)
    shadow = opt._shadow_views()
    for i, (e, w) in enumerate(zip(shadow, want)):
        assert ref.same_bits(e.cpu().numpy(), w), (decay, NUMELS[i])
    assert ref.same_bits(shadow[NO_GRAD].cpu().numpy(), start[NO_GRAD])          # no gradient: no chunk, shadow untouched
    assert not ref.same_bits(shadow[0].cpu().numpy(), start[0])
    assert not _same(shadow[-1], params[-1])                                     # the average lags the weights
    # parameters, moments and step counts: the bits the plain update leaves
    assert _same(bank, bank2)
    assert _same(tails["exp_avg"], tails2["exp_avg"]) and _same(tails["exp_avg_sq"], tails2["exp_avg_sq"])
    assert opt._dev_steps.tolist() == plain._dev_steps.tolist() == [0.0 if i == NO_GRAD else float(K) for i in range(len(NUMELS))]
    # nothing was written behind a tensor or behind a flat buffer
    assert _gaps_are_nan(bank, spans)
    for name, big in tails.items():
        assert bool(torch.isnan(big[opt.numel:]).all()) and bool(torch.isfinite(big[:opt.numel]).all()), name


def _stepped(decay=0.5, steps=3, **kw):
    from ms_gat_amd import engine
    bank, params, spans = _bank(2)
    opt = engine.FlatAdam(params, lr=1e-2, ema_decay=decay, **kw)
    for k in range(steps):
        for p, g in zip(params, _gradients(200 + k, params)):
            p.grad = g
        opt.step()
    return bank, params, spans, opt


def test_swap_exchanges_bits_twice_is_the_identity_and_the_context_restores():
    bank, params, spans, opt = _stepped()
    opt.shadow.view(torch.int32)[5] = 0x7FC12345              # a NaN with a payload: the exchange is of words, not of values
    raw, shadow = _bits(bank), _bits(opt.shadow)
    raw_views = [_bits(p) for p in params]
    opt.swap_averaged()
    assert opt.swapped
    assert torch.equal(torch.cat([_bits(p) for p in params]), shadow)            # parameters hold the old shadow bits
    assert torch.equal(_bits(opt.shadow), torch.cat(raw_views))                  # the shadow holds the old parameter bits
    assert _gaps_are_nan(bank, spans)
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.step()
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.state_dict()
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.averaged_state()
    opt.swap_averaged()
    assert not opt.swapped and torch.equal(_bits(bank), raw) and torch.equal(_bits(opt.shadow), shadow)
    with pytest.raises(ZeroDivisionError):
        with opt.averaged_parameters():
            assert opt.swapped and torch.equal(torch.cat([_bits(p) for p in params]), shadow)
            1 / 0
    assert not opt.swapped and torch.equal(_bits(bank), raw) and torch.equal(_bits(opt.shadow), shadow)
    opt.state_dict()                                          # and the optimizer is usable again
    # the accessors for checkpoints: out and back in place
    state = opt.averaged_state()
    assert state["decay"] == 0.5 and sorted(state["shadow"]) == list(range(len(NUMELS)))
    held = opt.shadow.data_ptr()
    opt.shadow.zero_()
    opt.load_averaged_state(state)
    assert opt.shadow.data_ptr() == held and torch.equal(_bits(opt.shadow), shadow)
    assert opt.shadow.data_ptr() in opt.buffer_token()


def test_a_step_the_guard_leaves_out_moves_no_bit_of_the_shadow():
    bank, params, spans, opt = _stepped(steps=1, skip_nonfinite=True)
    before, raw, counts = _bits(opt.shadow), _bits(bank), opt._dev_steps.tolist()
    grads = _gradients(300, params)
    grads[4].view(-1)[1000] = float("nan")
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()
    assert opt.guard_stats()["skipped_steps"] == 1
    assert torch.equal(_bits(opt.shadow), before) and torch.equal(_bits(bank), raw)
    assert opt._dev_steps.tolist() == counts == [0.0 if i == NO_GRAD else 1.0 for i in range(len(NUMELS))]
    # the following finite step: t = 2, as if the skipped one had not happened
    was = [e.cpu().numpy().copy() for e in opt._shadow_views()]
    for p, g in zip(params, _gradients(301, params)):
        p.grad = g
    opt.step()
    for i, (p, e) in enumerate(zip(params, opt._shadow_views())):
        if i != NO_GRAD:
            assert ref.same_bits(e.cpu().numpy(), ref.average_f32(was[i], p.detach().cpu().numpy(), 0.5, 2)), NUMELS[i]
            assert not ref.same_bits(e.cpu().numpy(), ref.average_f32(was[i], p.detach().cpu().numpy(), 0.5, 3))


# ---- the Trainer: captured steps, validation on the averaged weights ---------------------------------------------------
def _dataset():
    from ms_gat_amd import data
    torch.manual_seed(0)
    return data.SyntheticPEMS(n_nodes=32, n_edges=40, n_channels=1, in_hours=[1, 2, 3], batch_size=8, days=2)


def _model(ds, **kw):
    from ms_gat_amd import model
    torch.manual_seed(0)
    return model.msgat48(n_components=3, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True, adj=ds.adj, **kw)


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    """Six steps with decay 0.5 (the cap is not reached: the warm-up decides every step), eager and captured."""
    from ms_gat_amd import engine
    tmp = tmp_path_factory.mktemp("weight_average")
    ds = _dataset()
    net = _model(ds).to(DEV)
    twin = copy.deepcopy(net)
    batches = [b for _, b in zip(range(6), ds.training)]
    eager = engine.Trainer(net, 50.0, str(tmp / "eager"), hip_graph=False, ema_decay=0.5)
    graphed = engine.Trainer(twin, 50.0, str(tmp / "graph"), hip_graph=True, ema_decay=0.5)
    eager.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
    graphed.run_epoch(batches, gpu_id=0, epoch=1, mode="train")
    return ds, eager, graphed


def test_captured_steps_leave_the_shadow_and_the_parameters_of_the_eager_run(two_runs):
    _, eager, graphed = two_runs
    assert len(graphed._graphs) == 1 and not eager._graphs
    assert graphed.optimizer._dev_steps.tolist() == eager.optimizer._dev_steps.tolist()
    assert set(graphed.optimizer._host_steps) <= {0, 6} and 6 in graphed.optimizer._host_steps
    worst_p = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(eager.model.parameters(), graphed.model.parameters()))
    worst_e = float((eager.optimizer.shadow - graphed.optimizer.shadow).abs().max())
    print(f"captured against eager after 6 steps: parameters differ by at most {worst_p:.3e}, shadows by {worst_e:.3e}")
    for (name, p), q in zip(eager.model.named_parameters(), graphed.model.parameters()):
        assert _same(p, q), name
    assert _same(eager.optimizer.shadow, graphed.optimizer.shadow)
    assert not _same(eager.optimizer.shadow, torch.cat([p.detach().reshape(-1) for p in eager.optimizer._params]))


def _fresh_from_shadow(ds, trainer, **kw):
    fresh = _model(ds, **kw).to(DEV)
    fresh.load_state_dict({**trainer.model.state_dict(), **trainer.averaged_state()["shadow"]})
    return fresh


def _validate_on_the_average(ds, trainer, tmp, **kw):
    """The validation loss and the last prediction of `trainer`'s captured validation graph inside averaged_parameters(),
    and the same from a fresh model loaded from the shadow (launched eagerly)."""
    from ms_gat_amd import engine
    val = [b for _, b in zip(range(2), ds.validation)]
    raw_loss = trainer.run_epoch(val, gpu_id=0, epoch=1, mode="validate")      # captures the validation graph: raw weights
    n_graphs = len(trainer._graphs)
    raw = [p.detach().clone() for p in trainer.model.parameters()]
    fresh = _fresh_from_shadow(ds, trainer, **kw)
    with trainer.averaged_parameters():
        got_loss = trainer.run_epoch(val, gpu_id=0, epoch=1, mode="validate")  # a replay: the addresses it already holds
        got_pred = trainer._graphs[(False, tuple(tuple(t.shape) for t in val[-1]), val[-1][0].shape[0])].pred.clone()
    assert len(trainer._graphs) == n_graphs
    assert all(_same(p, q) for p, q in zip(trainer.model.parameters(), raw))   # the raw weights are back
    ev = engine.Engine(fresh, 50.0, str(tmp))
    want_loss = ev.run_epoch(val, gpu_id=0, mode="validate")
    fresh.eval()
    with torch.no_grad():
        want_pred = fresh(*[t.to(DEV) for t in val[-1][:3]])
    print(f"validation loss: raw {raw_loss!r}, averaged (captured) {got_loss!r}, fresh model from the shadow {want_loss!r}; "
          f"predictions differ by at most {float((got_pred - want_pred).abs().max()):.3e}")
    return raw_loss, got_loss, want_loss, got_pred, want_pred


def test_captured_validation_inside_averaged_parameters_is_that_of_a_model_loaded_from_the_shadow(two_runs, tmp_path):
    ds, _, graphed = two_runs
    raw_loss, got_loss, want_loss, got_pred, want_pred = _validate_on_the_average(ds, graphed, tmp_path)
    assert got_loss == want_loss and got_loss != raw_loss
    assert torch.equal(got_pred, want_pred)


def test_learned_edge_weights_validate_on_their_average(tmp_path):
    """Nothing caches a tensor derived from a trainable parameter: the model with learned edge weights, whose graph values
    ARE a parameter, computes with the swapped-in values at once."""
    from ms_gat_amd import engine
    ds = _dataset()
    net = _model(ds, learn_edge_weights=True).to(DEV)
    tr = engine.Trainer(net, 50.0, str(tmp_path / "run"), hip_graph=True, ema_decay=0.5)
    tr.run_epoch([b for _, b in zip(range(3), ds.training)], gpu_id=0, epoch=1, mode="train")
    state = tr.averaged_state()["shadow"]
    assert "edge_weight" in state and not _same(state["edge_weight"], net.edge_weight)
    raw_loss, got_loss, want_loss, got_pred, want_pred = _validate_on_the_average(ds, tr, tmp_path / "fresh",
                                                                                  learn_edge_weights=True)
    assert got_loss == want_loss and got_loss != raw_loss
    assert torch.equal(got_pred, want_pred)


def test_save_load_on_the_device_restores_the_shadow_in_place(two_runs, tmp_path):
    from ms_gat_amd import engine
    ds, eager, graphed = two_runs
    graphed.save(tmp_path / "ck.pkl")
    states = torch.load(tmp_path / "ck.pkl", weights_only=False)
    assert sorted(states) == ["best", "ema", "epoch", "grad_scaler", "model", "optimizer", "scheduler"]
    assert states["ema"]["decay"] == 0.5 and set(states["ema"]["shadow"]) < set(states["model"])
    want = _bits(graphed.optimizer.shadow)
    held, n_graphs = graphed.optimizer.shadow.data_ptr(), len(graphed._graphs)
    graphed.optimizer.shadow.zero_()
    graphed.load(tmp_path / "ck.pkl")
    assert graphed.optimizer.shadow.data_ptr() == held and len(graphed._graphs) == n_graphs
    assert torch.equal(_bits(graphed.optimizer.shadow), want)
    # a fresh trainer, and an evaluator that picks the averaged weights
    other = engine.Trainer(_model(ds).to(DEV), 50.0, str(tmp_path / "other"), hip_graph=False, ema_decay=0.5)
    other.load(tmp_path / "ck.pkl")
    assert torch.equal(_bits(other.optimizer.shadow), want)
    net = _model(ds).to(DEV)
    ev = engine.Evaluator(net, 50.0, str(tmp_path / "eval"), tmp_path / "ck.pkl", hip_graph=False)
    assert ev.weights == "averaged"
    for name, p in net.named_parameters():
        assert _same(p, states["ema"]["shadow"].get(name, states["model"][name])), name
