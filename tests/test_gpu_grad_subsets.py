"""GPU: every autograd op of ms_gat_amd/ops.py with only SOME of its inputs requiring grad, and a multi-output node with only
some of its outputs reaching the loss -- input attribution in eval(), a head fine-tuned on a frozen backbone, frozen biases
or time embedding, modules built with bias=None.  The `ctx.needs_input_grad` branches of the backward functions select
kernel forms (null output pointers, another reduction, separate launches instead of a fused pass) that the other tests,
which make every input a leaf and hand a cotangent to every output, never run.

Cases, restatements and the subset enumeration: grad_subset_fixtures.py; test_grad_subsets_cpu.py shows without a GPU
that the restatements evaluated in fp32 meet every bar applied here.  Per row and subset S of its differentiable inputs:
the forward bits equal the full-set run's; for i in S the gradient meets the bar of the op's own test against the float64
restatement differentiated for the same S, and is finite; for i not in S the leaf's .grad stays None (torch.autograd.grad
refuses a tensor that does not require grad, so the run is a backward() and the leaves are read); `own_launch` gradients
equal the full-set run's bit for bit; where a fused pass and separate passes exist the distance to the full-set run goes
to the parity log.

Null outputs and optional operands the sweep hands to the C entry points, and where each is guarded (read before the first
run on a GPU; csrc = ms_gat_amd/csrc):
  msgat_head_forward_ln          normalised = NULL (W frozen): `xn != nullptr` at both stores, branches.hip k_head_fwd_ln forms
                                 (:414, :493); ln_weight / ln_bias NULL: `if (lnw)` / `if (lnb)` (:391-392, :470-471)
  msgat_layernorm_head_backward  dln_weight / dln_bias NULL: the kernel writes partials only, the sum skips a null
                                 destination (reduce.hip:70-72, :98-100); ln_weight NULL: branches.hip:642
  msgat_layernorm_backward       dweight / dbias NULL: reduce.hip as above; weight, dx_add NULL: layernorm.hip:148, :143, :204
  msgat_layernorm_backward_pooled  dpool_rows NULL: layernorm.hip:167; dpool_w NULL: no reduction job (:274); api.hip:869
                                 refuses one without the other; bias NULL: :178
  msgat_gate_sum_backward        dpred NULL: no blocks for it and tail.hip:214; dh_w / dd_w NULL: :241; d_w, H, D NULL: the
                                 static gate, nd = 0 (tail.hip:265-270)
  msgat_causal_conv_grad_weight  no optional pointer; with_ones = 0 is a flag of the contraction (a virtual channel,
                                 contract.hip:109) and picks launch_reduce_groups over 2 Co Ci sums per relation -- the size
                                 ops.py allocates (api.hip:427-428)
  msgat_time_mix (backward)      bias forced to NULL (api.hip:384), read in the forward branch only (branches.hip:59)
  msgat_node_pool_grad_signal    dx_add NULL: branches.hip:247; msgat_node_pool_grad_weight has no optional pointer
  msgat_contract_segments, msgat_contract_mix_segments  every pointer required (api.hip:534, :572); with_ones as above;
                                 partials sized by the matching *_partial_floats call in ops.py
  msgat_mix_segments (backward)  bias NULL, no add operands: MixEpilogue (common.hpp:303, :316, :320; mfma.hip:191, :245)
  the reduce jobs                reduce.hip:65-72, :93-100 (dst0 / dst1 NULL); launch_reduce_lastcol gets both from one buffer
A LayerNorm's parameter-set count comes from whichever of weight and bias is given (ops._ln_sets), so a bias [R,T] without
a weight gets a gradient of R rows from the reduction that writes R rows (`ln_head ... per relation no LayerNorm weight`,
`layer_norm_t ... no weight per relation bias`, `layer_norm_pool_tee ... no LayerNorm weight` are its rows); a weight and a
bias of different shapes are refused, since the kernels index both by the relation
(test_layernorm_parameters_of_different_shapes_are_refused).

The forward's form follows the grad mode alone, never what requires grad: gacn / attention_core run the score kernel that
also forms pq (it rounds lse differently from the inference kernel), and layer_norm_pool_tee goes through its node wherever
the node's forward is the fused LayerNorm-and-pooling pass (same parameter-set counts, N >= 64; it sums the pooling in
another order than node_pool).  Hence the forward-bits checks: every subset against the full set, and each row once with
NOTHING requiring grad in grad mode -- a wholly frozen block of a fine-tuned backbone.  The tee's node takes unused
cotangents as None, and the output sweep runs its `dy is None` / `dpooled is None` branches."""
import copy
import functools

import pytest
import torch

from conftest import assert_parity, record_err, rel_err

import grad_subset_fixtures as gs
from poison_fixtures import device_errors_end_the_session as _device_errors_end_the_session
from oracle import dense_torch
from ms_gat_amd import engine, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WHAT = "grad_subsets"
TOL = 1e-4


def _run(row, inputs, cots, subset, outsel=None):
    """-> (outputs, {differentiable input: its .grad}) of the library's op with exactly `subset` requiring grad and a
    cotangent at the outputs `outsel` (None: all)"""
    with _device_errors_end_the_session():
        t = gs.leaves(inputs, subset, device=DEV)
        outs = tuple(row.lib(ops, t))
        sel = gs.differentiable(outs, outsel)
        torch.autograd.backward([outs[i] for i in sel], [cots[i].to(DEV) for i in sel])
        torch.cuda.synchronize()
    return tuple(o.detach() for o in outs), {k: t[k].grad for k in row.diff}


def _forward(row, inputs):
    """-> outputs of the library's op in grad mode with NOTHING requiring grad (a wholly frozen block of a fine-tuned model)"""
    with _device_errors_end_the_session():
        outs = tuple(o.detach() for o in row.lib(ops, gs.leaves(inputs, (), device=DEV)))
        torch.cuda.synchronize()
    return outs


def _bar(row, got, want, key, failures, worst):
    """`worst`: {tensor: the largest error over the runs of a case}, what goes to the parity log for a max-norm bar (the
    per-entry bar logs every comparison itself)"""
    try:
        if row.bar == gs.PARITY:
            assert_parity(got, want, WHAT, key)
        else:
            e = rel_err(got, want)
            tensor = key.rsplit(":", 1)[1]
            worst[tensor] = max(worst.get(tensor, 0.0), e)
            assert e < row.bar[1], f"{key}: rel err {e:.3e} >= {row.bar[1]}"
    except AssertionError as err:
        failures.append(str(err))


def _log(row, name, worst):
    for tensor, e in worst.items():
        record_err(WHAT, f"{name}:{tensor}", e, row.bar[1] if len(row.bar) > 1 else TOL)


def _compare(row, run, ref, subset, key, failures, worst):
    """One run against the restatement differentiated for the same inputs and outputs"""
    outs, grads = run
    want_outs, want = ref
    for i, (a, b) in enumerate(zip(outs, want_outs)):
        _bar(row, a, b, f"{key}:out{i}", failures, worst)
    for k in row.diff:
        g = grads[k]
        if k not in subset:
            if g is not None:
                failures.append(f"{key}: frozen input {k} received a gradient")
        elif want[k] is None:       # the selected outputs do not depend on it: nothing, or the zeros of a materialised cotangent
            if g is not None and bool(g.any()):
                failures.append(f"{key}: d{k} is non-zero though no selected output depends on {k}")
        elif g is None:
            failures.append(f"{key}: no gradient for {k}")
        elif g.shape != want[k].shape or not bool(torch.isfinite(g).all()):
            failures.append(f"{key}: d{k} has shape {tuple(g.shape)} or is not finite")
        else:
            _bar(row, g, want[k], f"{key}:d{k}", failures, worst)


@pytest.mark.parametrize("name", [r.name for r in gs.ROWS], ids=gs.ROW_IDS)
def test_op_with_a_subset_of_its_inputs_requiring_grad(name):
    row, inputs, cots = gs.problem(name)
    failures, worst = [], {}
    full = _run(row, inputs, cots, row.diff)
    for i, (a, b) in enumerate(zip(_forward(row, inputs), full[0])):
        if not torch.equal(a, b):
            failures.append(f"{name}: output {i} with nothing requiring grad differs from the full-set run's by {rel_err(a, b):.3e}")
    for subset in gs.subsets(row.diff):
        key = f"{name} [{','.join(subset)}]"
        run = full if subset == row.diff else _run(row, inputs, cots, subset)
        _compare(row, run, gs.reference(name, subset), subset, key, failures, worst)
        for i, (a, b) in enumerate(zip(run[0], full[0])):
            if not torch.equal(a, b):
                failures.append(f"{key}: output {i} differs from the full-set run's by {rel_err(a, b):.3e}")
        for k in subset:
            if run[1][k] is None or full[1][k] is None:
                continue
            if k in row.own_launch:
                if not torch.equal(run[1][k], full[1][k]):
                    failures.append(f"{key}: d{k} differs from the full-set run's by {rel_err(run[1][k], full[1][k]):.3e}")
            elif row.fused and subset != row.diff:
                worst[f"d{k} vs full set"] = max(worst.get(f"d{k} vs full set", 0.0), rel_err(run[1][k], full[1][k]))
    _log(row, name, worst)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", [r.name for r in gs.ROWS if r.out_subsets], ids=[i for r, i in zip(gs.ROWS, gs.ROW_IDS) if r.out_subsets])
def test_multi_output_op_with_a_subset_of_its_outputs_reaching_the_loss(name):
    """Every input requires grad; the cotangent reaches only the outputs `outsel` (autograd hands the node zeros, or None,
    for the others).  The reference differentiates the same outputs."""
    row, inputs, cots = gs.problem(name)
    failures, worst = [], {}
    full = _run(row, inputs, cots, row.diff)
    for outsel in row.out_subsets:
        key = f"{name} outputs {outsel}"
        run = _run(row, inputs, cots, row.diff, outsel)
        _compare(row, run, gs.reference(name, row.diff, outsel), row.diff, key, failures, worst)
        for i, (a, b) in enumerate(zip(run[0], full[0])):
            if not torch.equal(a, b):
                failures.append(f"{key}: output {i} differs from the all-outputs run's")
    _log(row, name + " output subsets", worst)
    assert not failures, "\n".join(failures)


def test_layernorm_parameters_of_different_shapes_are_refused():
    x, pool_w = torch.zeros(gs.G, 5, 13, 12, device=DEV), torch.ones(13, device=DEV)
    w, b = torch.ones(gs.R, 12, device=DEV), torch.zeros(12, device=DEV)
    for call in (lambda: ops.layer_norm_t(x, w, b), lambda: ops.layer_norm_pool_tee(x, w, b, gs.EPS, False, pool_w),
                 lambda: ops.ln_head(x, w, b, gs.EPS, torch.zeros(7, 12, 1, 5, device=DEV)),
                 lambda: ops.layer_norm_t(x, b, w)):
        with pytest.raises(ValueError, match="same shape"):
            call()


# ---- the whole model with part of it frozen ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _all_trainable(factory, cin, stack):
    """-> prediction of the model with every parameter trainable, the schedule `stack`"""
    net, X, H, D, dout = gs.model_problem(factory, cin)
    net.to(DEV)
    net.stack_components = stack
    pred = net(X.to(DEV), H.to(DEV), D.to(DEV))
    return pred.detach()


@pytest.mark.parametrize("stack", [True, False], ids=["stacked", "loop"])
@pytest.mark.parametrize("scenario", gs.SCENARIOS, ids=[s.replace(" ", "_") for s in gs.SCENARIOS])
@pytest.mark.parametrize("factory,cin", gs.MODEL_CASES)
def test_whole_model_with_part_of_it_frozen(factory, cin, scenario, stack):
    """The setup of test_whole_model_matches_the_dense_op_sequence with (a) eval() and every parameter frozen, the gradient
    at the input; (b) only fc.* and the components' last ln.* trainable; (c) every bias frozen; (d) the time embedding frozen:
    the prediction's bits are those of the all-trainable run, the trainable gradients meet that test's bar against float64,
    the frozen parameters keep .grad None."""
    net, X, H, D, dout = gs.model_problem(factory, cin)
    net.to(DEV)
    net.stack_components = stack
    x_grad = gs.freeze(net, scenario)
    X, H, D, dout = X.to(DEV).requires_grad_(x_grad), H.to(DEV), D.to(DEV), dout.to(DEV)
    with _device_errors_end_the_session():
        pred = net(X, H, D)
        pred.backward(dout)
        torch.cuda.synchronize()
    assert torch.equal(pred.detach(), _all_trainable(factory, cin, stack)), rel_err(pred, _all_trainable(factory, cin, stack))
    want_pred, want, want_dx = gs.model_reference(net, X.detach(), H, D, dout, torch.float64, x_grad)
    what = f"{WHAT} {factory} {scenario} {'stacked' if stack else 'loop'}"
    failures = []
    e = rel_err(pred, want_pred)
    record_err(what, "prediction", e, TOL)
    assert e < TOL
    worst = (0.0, None)
    for n, p in net.named_parameters():
        if n in want:
            if p.grad is None or not bool(torch.isfinite(p.grad).all()):
                failures.append(f"{n}: no finite gradient")
                continue
            e = rel_err(p.grad, want[n])
            worst = max(worst, (e, n))
            if not e < TOL:
                failures.append(f"{n}: rel err {e:.3e}")
        elif not p.requires_grad and p.grad is not None:
            failures.append(f"{n}: frozen, but received a gradient")
    assert len(want) == sum(1 for p in net.parameters() if p.requires_grad)
    if want:
        record_err(what, f"worst of {len(want)} gradients: {worst[1]}", worst[0], TOL)
    if x_grad:
        e = rel_err(X.grad, want_dx)
        record_err(what, "dX", e, TOL)
        assert bool(torch.isfinite(X.grad).all()) and e < TOL, e
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("hip_graph", [False, True])
def test_trainer_steps_the_head_of_a_frozen_backbone(tmp_path, hip_graph):
    """Scenario (b) through engine.Trainer, eager and captured: two steps leave every frozen parameter's bits where they
    were and track the plain loop (the same model, the reference's loss, torch.optim.Adam with the Trainer's settings) --
    the losses to 1e-4 and the trained parameters to 2e-4 of their largest entry, the bars of
    test_five_optimizer_steps_track_the_reference_training_loop."""
    net, X, H, D, Y = gs.model_problem("msgat72", 3)
    gs.freeze(net, "head only")
    net.to(DEV)
    twin = copy.deepcopy(net)
    frozen = {n: p.detach().clone() for n, p in net.named_parameters() if not p.requires_grad}
    tr = engine.Trainer(net, 50.0, str(tmp_path), hip_graph=hip_graph)
    losses = [tr.run_epoch([[X, H, D, Y]], gpu_id=0, epoch=k + 1, mode="train") for k in range(2)]
    torch.cuda.synchronize()
    trained = [p for p in twin.parameters() if p.requires_grad]
    assert len(trained) == 8 and len(frozen) == len(list(net.parameters())) - 8
    opt = torch.optim.Adam(trained, lr=1e-3, weight_decay=5e-4)
    what = f"{WHAT} trainer head only {'replayed' if hip_graph else 'eager'} vs the plain fp32 loop"
    for k in range(2):
        loss = dense_torch.huber(twin(X.to(DEV), H.to(DEV), D.to(DEV)), Y.to(DEV), 50.0)
        opt.zero_grad()
        loss.backward()
        opt.step()
        record_err(what, f"loss[{k}]", abs(losses[k] - float(loss.detach())) / abs(float(loss.detach())), 1e-4)
        assert abs(losses[k] - float(loss.detach())) < 1e-4 * abs(float(loss.detach())), (k, losses[k], float(loss.detach()))
    for (n, p), q in zip(net.named_parameters(), twin.parameters()):
        if n in frozen:
            assert torch.equal(p.detach(), frozen[n]) and p.grad is None, n
        else:
            e = rel_err(p.detach(), q.detach())
            record_err(what, n, e, 2e-4)
            assert e < 2e-4, (n, e)
            assert not torch.equal(p.detach(), _initial(n)), n


@functools.lru_cache(maxsize=None)
def _initial_state():
    net = gs.model_problem("msgat72", 3)[0]
    return {n: p.detach().clone() for n, p in net.named_parameters()}


def _initial(name):
    return _initial_state()[name].to(DEV)
