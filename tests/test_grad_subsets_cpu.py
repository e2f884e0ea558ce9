"""No GPU: what test_gpu_grad_subsets.py rests on, so that a failure there blames the kernel and not the case table.

* Every restatement of grad_subset_fixtures.py evaluated in fp32 on the CPU meets, against its float64 self, the bar the
  GPU test applies to the library -- for every row, every subset of inputs that requires grad and every subset of outputs
  that carries a cotangent (the kernels do the same arithmetic in the same format).
* The subset enumeration is the one the GPU test is described with: singles, leave-one-outs, the full set.
* Every torch.autograd.Function subclass of ops.py has a row or a reason for having none, so that an op added later does
  not slip past the sweep.
* The table has the forms it names: the widths, the node counts on both sides of the 512 positions from which the LDS-DMA
  contractions run, a T = 8 row per op, every optional operand once as None, both GACN modes."""
import inspect

import pytest
import torch

from conftest import elementwise_violations, rel_err

import grad_subset_fixtures as gs


def meets(bar, got, want):
    """The bar of the GPU test without its log: -> (met, rel_err)"""
    e = rel_err(got, want)
    if bar == gs.PARITY:
        return e < 1e-4 and elementwise_violations(got, want, 1e-4, 1e-5) == 0.0, e
    return e < bar[1], e


@pytest.mark.parametrize("name", [r.name for r in gs.ROWS], ids=gs.ROW_IDS)
def test_restatement_in_fp32_meets_the_bar_of_the_gpu_test(name):
    row, inputs, cots = gs.problem(name)
    runs = [(s, None) for s in gs.subsets(row.diff)] + [(row.diff, o) for o in row.out_subsets]
    for subset, outsel in runs:
        o64, g64 = gs.reference(name, subset, outsel, torch.float64)
        o32, g32 = gs.reference(name, subset, outsel, torch.float32)
        for a, b in zip(o32, o64):
            ok, e = meets(row.bar, a, b)
            assert ok, (subset, outsel, "output", e)
        for k in subset:
            assert (g32[k] is None) == (g64[k] is None), (subset, outsel, k)
            if g64[k] is not None:
                assert bool(torch.isfinite(g64[k]).all()) and g64[k].shape == inputs[k].shape
                ok, e = meets(row.bar, g32[k], g64[k])
                assert ok, (subset, outsel, k, e)


def test_a_gradient_does_not_depend_on_what_else_requires_grad():
    """The restatement's own gradients agree bit for bit between a subset and the full set (autograd on the CPU computes
    each from the same graph): what the GPU test records or asserts as a difference is the library's."""
    for name in ("mix 5->9 N=13 T=8 bias", "ln_head C=5 N=13 To=7", "causal_conv 9->9 N=13 d=2 bias per relation"):
        row = gs.problem(name)[0]
        full = gs.reference(name, row.diff)[1]
        for s in gs.subsets(row.diff):
            for k, g in gs.reference(name, s)[1].items():
                assert torch.equal(g, full[k]), (name, s, k)


def test_subset_enumeration():
    assert gs.subsets(("a",)) == [("a",)]
    assert gs.subsets(("a", "b")) == [("a",), ("b",), ("a", "b")]
    assert gs.subsets(("a", "b", "c")) == [("a",), ("b",), ("c",), ("b", "c"), ("a", "c"), ("a", "b"), ("a", "b", "c")]
    for row in gs.ROWS:
        k = len(row.diff)
        s = gs.subsets(row.diff)
        assert len(s) == len(set(s)) <= 2 * k + 1 and s[-1] == row.diff and all(s)
        assert {x for x in s if len(x) == 1} == {(n,) for n in row.diff}
        assert {x for x in s if len(x) == k - 1} >= ({tuple(m for m in row.diff if m != n) for n in row.diff} if k > 1 else set())
        inputs = row.make()
        assert all(torch.is_tensor(inputs[n]) and inputs[n].dtype == torch.float32 for n in row.diff), row.name
        # every float tensor among the inputs is either differentiable or the adjacency
        assert {n for n, v in inputs.items() if torch.is_tensor(v) and v.is_floating_point()} - set(row.diff) <= {"adj"}
    assert gs.output_subsets(gs.ROWS[0]) == (None,)
    tee = next(r for r in gs.ROWS if r.function == "_LnPoolTeeFunction")
    assert len(gs.output_subsets(tee)) == 7 and len(set(tee.out_subsets)) == 6


def test_every_autograd_function_of_ops_has_a_row_or_a_reason():
    from ms_gat_amd import ops
    classes = {n for n, c in vars(ops).items()
               if inspect.isclass(c) and issubclass(c, torch.autograd.Function) and c is not torch.autograd.Function}
    covered = {r.function for r in gs.ROWS}
    assert covered <= classes and set(gs.EXCLUDED) <= classes
    assert not covered & set(gs.EXCLUDED)
    assert classes == covered | set(gs.EXCLUDED), sorted(classes - covered - set(gs.EXCLUDED))
    assert all(reason for reason in gs.EXCLUDED.values())


def test_the_table_has_the_forms_it_names():
    from ms_gat_amd import _lib, ops
    rows = {r.name: r for r in gs.ROWS}
    assert len(rows) == len(gs.ROWS)
    largest = 0
    by_function = {}
    for r in gs.ROWS:
        inputs = r.make()
        by_function.setdefault(r.function, []).append(inputs)
        largest = max([largest] + [v.numel() for v in inputs.values() if torch.is_tensor(v)])
    assert largest == 4 * 72 * 64 * 12
    launching = set(by_function) - {"_AssembleRowsFunction", "_BiasJoinFunction", "_Relayout"}
    for f in launching:     # a T = 8 row next to the T = 12 ones, for every op that launches a kernel
        lasts = {v.shape[-1] for t in by_function[f] for k, v in t.items() if torch.is_tensor(v) and v.dim() >= 3 and k != "adj"}
        assert {8, 12} <= lasts or f == "_GateSumFunction", f
    # every optional operand once as None
    for f, names in (("_MixFunction", ("bias", "add")), ("_MixMultiFunction", ("bias",)), ("_TimeMixFunction", ("bias",)),
                     ("_CausalConvFunction", ("bias",)), ("_HeadFunction", ("bias",)), ("_LnHeadFunction", ("lnw", "lnb", "bias")),
                     ("_LayerNormTFunction", ("w", "b")), ("_LnPoolTeeFunction", ("w", "b")), ("_GateSumFunction", ("d_w",))):
        for n in names:
            assert any(t[n] is None for t in by_function[f]) and any(t[n] is not None for t in by_function[f]), (f, n)
    for t in by_function["_CausalConvFunction"]:
        assert ops.causal_conv_fused(t["taps"].shape[2], t["taps"].shape[1] // 2)
    assert not ops.causal_conv_fused(5, 9)
    for t in by_function["_ChannelAttentionMixFunction"]:
        assert ops.channel_attention_fused(t["p"].shape[1], t["conv"].shape[1], t["p"].shape[2])
    L = _lib.lib()
    for name, mode in gs.GACN_MODES.items():
        t = rows[name].make()
        assert L.msgat_gacn_mode(t["x"].shape[1], t["W"].shape[1]) == mode
    assert set(gs.GACN_MODES.values()) == {_lib.MODE_AGG_FIRST, _lib.MODE_PROJ_FIRST}
    # both sides of the 512 positions from which the LDS-DMA contractions run
    assert 13 * 12 < 512 <= 64 * 12


def test_relu_rows_keep_their_cotangent_off_the_kink():
    for r in gs.ROWS:
        if r.pre is None:
            continue
        row, inputs, cots = gs.problem(r.name)
        t64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in inputs.items()}
        for pre, c in zip(r.pre(t64), cots):
            assert not bool(c[pre.abs() <= gs.MARGIN].any())
            assert bool((c != 0).double().mean() > (0.2 if r.premasked else 0.9))
            if r.premasked:
                assert not bool(c[pre <= 0].any())


@pytest.mark.parametrize("scenario", gs.SCENARIOS, ids=[s.replace(" ", "_") for s in gs.SCENARIOS])
@pytest.mark.parametrize("factory,cin", gs.MODEL_CASES)
def test_whole_model_restatement_in_fp32_meets_the_bar_in_every_scenario(factory, cin, scenario):
    """branch_edge_fixtures.msgat_dense with part of the model frozen: prediction, every trainable gradient and the gradient
    at the input within 1e-4 of float64 (the bar of test_whole_model_matches_the_dense_op_sequence), and the scenarios freeze
    what they name."""
    net, X, H, D, dout = gs.model_problem(factory, cin)
    everything = {n for n, p in net.named_parameters() if p.requires_grad}
    x_grad = gs.freeze(net, scenario)
    trainable = {n for n, p in net.named_parameters() if p.requires_grad}
    assert trainable == {"input attribution": set(),
                         "head only": {f"tpcs.{r}.{m}.{p}" for r in range(gs.MODEL_R) for m in ("ln", "fc") for p in ("weight", "bias")},
                         "biases frozen": {n for n in everything if not n.endswith(".bias")},
                         "time embedding frozen": everything - {"te.h_ebd.weight", "te.d_ebd.weight"}}[scenario]
    assert x_grad == (scenario == "input attribution") and net.training != x_grad
    p64, g64, dx64 = gs.model_reference(net, X, H, D, dout, torch.float64, x_grad)
    p32, g32, dx32 = gs.model_reference(net, X, H, D, dout, torch.float32, x_grad)
    assert rel_err(p32, p64) < 1e-4 and set(g64) == trainable
    for k in g64:
        assert rel_err(g32[k], g64[k]) < 1e-4, k
    if x_grad:
        assert dx64.shape == X.shape and rel_err(dx32, dx64) < 1e-4
