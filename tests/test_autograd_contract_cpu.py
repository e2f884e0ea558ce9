"""No GPU: what test_gpu_autograd_contract.py rests on, so that a failure there blames the library and not the harness.

* The checks of autograd_contract_fixtures.py have teeth: four toy torch.autograd.Functions in plain torch, each breaking
  the contract in one way -- a backward that scales its cotangent in place, one that uses a saved buffer as scratch, a
  forward that writes an input, per-call state parked on a shared object -- are each flagged by the check meant for it,
  and the correct toy passes every check.
* The second problem of every row (`seed=1`) leaves the first as it always was (checksums taken before the seed existed).
* Two censuses: every torch.autograd.Function of ops.py is run by a case of the GPU file (by `ast`), and every pointer the
  GPU file's docstring calls read-only is `const` in include/msgat_hip.h, every other pointer named as written (a text parse).
* The conditions on the inputs hold for the reference alone: the restatements in fp32 meet the bars of cases (b), (c), (g)
  and (h) against float64; the second problems differ from the first by more than 1e-2 everywhere, so a mix-up cannot hide
  inside a bar; the ReLU masking leaves out what `gs.problem` leaves out and no more."""
import os
import re
import zlib

import numpy as np
import pytest
import torch

from conftest import elementwise_violations, rel_err

import autograd_contract_fixtures as ac
import grad_subset_fixtures as gs
import poison_fixtures as pf
from test_grad_subsets_cpu import meets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(ROOT, "ms_gat_amd", "ops.py")
GPU_MODULE = os.path.join(ROOT, "tests", "test_gpu_autograd_contract.py")
HEADER = os.path.join(ROOT, "include", "msgat_hip.h")


def _read(path):
    with open(path) as f:
        return f.read()


# ---- the harness has teeth ---------------------------------------------------------------------------------------------------
# every toy computes y = x * w (w [C] along the last axis) and keeps y for a "fused" backward: dx = g * w, dw = sum(g * x)

class _Correct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, scratch):
        ctx.save_for_backward(x, w)
        return x * w

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return g * w, (g * x).reshape(-1, x.shape[-1]).sum(0), None


class _ScalesItsCotangent(torch.autograd.Function):
    """dx formed in the cotangent's own memory: one allocation less, and the caller's tensor is gone"""
    @staticmethod
    def forward(ctx, x, w, scratch):
        ctx.save_for_backward(x, w)
        return x * w

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dw = (g * x).reshape(-1, x.shape[-1]).sum(0)
        return (g.mul_(w) if 0 not in g.stride() else g * w), dw, None      # (torch refuses to write an expanded tensor)


class _ScratchInSavedBuffer(torch.autograd.Function):
    """keeps a buffer for backward and uses it as scratch there: the second backward reads what the first left"""
    @staticmethod
    def forward(ctx, x, w, scratch):
        buf = x.clone()
        ctx.save_for_backward(buf, w)
        return x * w

    @staticmethod
    def backward(ctx, g):
        buf, w = ctx.saved_tensors
        dw = (g * buf).reshape(-1, buf.shape[-1]).sum(0)
        buf.mul_(0.5)                                      # "scratch"
        return g * w, dw, None


class _WritesAnInput(torch.autograd.Function):
    """parks an intermediate in a tensor the caller handed in for reading"""
    @staticmethod
    def forward(ctx, x, w, scratch):
        ctx.save_for_backward(x, w)
        scratch.copy_(w * 2)
        return x * w

    backward = _Correct.backward


class _StateOnASharedPlan(torch.autograd.Function):
    """per-call state on an object every call with these dimensions shares: the last forward's wins"""
    plan = {}

    @staticmethod
    def forward(ctx, x, w, scratch):
        _StateOnASharedPlan.plan["x"] = x
        ctx.save_for_backward(w)
        return x * w

    @staticmethod
    def backward(ctx, g):
        w, = ctx.saved_tensors
        x = _StateOnASharedPlan.plan["x"]
        return g * w, (g * x).reshape(-1, x.shape[-1]).sum(0), None


def _toy(function, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    inputs = dict(x=torch.randn(3, 4, 5, generator=g), w=torch.randn(5, generator=g), scratch=torch.zeros(5))
    return ac.Case(f"{function.__name__} problem {seed}", inputs, ("x", "w"),
                   lambda t: (function.apply(t["x"], t["w"], t["scratch"]),), (torch.randn(3, 4, 5, generator=g),))


def _toy_reference(case, cots):
    x, w = (case.inputs[k].double().requires_grad_(True) for k in ("x", "w"))
    return dict(zip(("x", "w"), torch.autograd.grad(x * w, [x, w], cots[0].double())))


def _all_checks(function):
    """-> {check: findings} of the four checks on a toy"""
    a, b = _toy(function, 0), _toy(function, 1)
    repeat, third = ac.check_repeatable(a, b.cots)
    want = _toy_reference(a, b.cots)
    repeat += [f"d{k}: {rel_err(third[k], want[k]):.1e} from float64" for k in want if rel_err(third[k], want[k]) > 1e-6]
    forms, ran = ac.check_cotangent_forms(a)
    assert ran == len(ac.FORMS)
    return dict(a=ac.check_operands_intact(a), b=repeat, d=ac.check_interleaved(a, b), e=forms)


def test_the_correct_toy_passes_every_check():
    assert _all_checks(_Correct) == dict(a=[], b=[], d=[], e=[])
    got = ac.check_one_output_at_a_time(_toy(_Correct))
    want = _toy_reference(_toy(_Correct), _toy(_Correct).cots)
    assert all(rel_err(got[k], want[k]) < 1e-6 for k in want)


@pytest.mark.parametrize("function,check,says", [
    (_ScalesItsCotangent, "a", "the backward wrote its cotangent"),
    (_ScratchInSavedBuffer, "b", "the second backward differs from the first"),
    (_WritesAnInput, "a", "the forward wrote its input['scratch']"),
    (_StateOnASharedPlan, "d", "differs from its run alone"),
], ids=["cotangent_written", "saved_buffer_as_scratch", "input_written", "state_on_a_shared_object"])
def test_each_toy_violation_is_caught_by_the_check_meant_for_it(function, check, says):
    found = _all_checks(function)
    print("\n".join(f"({k}) {line}" for k, lines in found.items() for line in lines))
    assert any(says in line for line in found[check]), found[check]


def test_the_saved_buffer_is_seen_by_the_observer_and_the_slice_keeps_its_neighbours_out():
    found = _all_checks(_ScratchInSavedBuffer)
    assert any("the backward wrote its saved" in line for line in found["a"]), found["a"]       # a buffer no input aliases
    found = _all_checks(_ScalesItsCotangent)
    assert any("channel_slice: the backward wrote the cotangent's memory[1]" in line for line in found["e"]), found["e"]
    out = torch.zeros(2, 4, 3)
    for form in ac.FORMS:
        c, holder, dense = ac.cotangent_form(form, out, torch.ones(2, 4, 3))
        assert c.shape == out.shape and dense.is_contiguous() and pf.same_bits(c.contiguous(), dense)
        assert dense.data_ptr() not in (c.data_ptr(), out.data_ptr())
    c, holder, _ = ac.cotangent_form("channel_slice", out, torch.ones(2, 4, 3))
    assert not c.is_contiguous() and bool(torch.isnan(holder[:, :3]).all()) and bool(torch.isnan(holder[:, 7:]).all())
    assert c.stride()[1:] == (3, 1) and c.stride(0) == 9 * 3 and c.data_ptr() == holder[:, 3:].data_ptr()
    assert ac.cotangent_form("expanded", out, out)[0].stride() == (0, 0, 0)
    assert ac.cotangent_form("own_storage", out, out)[0].data_ptr() == out.data_ptr()
    assert ac.cotangent_form("channel_slice", torch.zeros(()), torch.zeros(())) is None
    before = ac.snapshot(dict(a=out, b=[out, None], c=3))
    out[1, 2, 0] = -0.0
    assert len(ac.changed(before, dict(a=out, b=[out, None], c=3))) == 2 and before["a"].data_ptr() != out.data_ptr()


class _ViewsOfOneGradient(torch.autograd.Function):
    """ops._BiasJoinFunction as it was: both gradients are views of the incoming one"""
    @staticmethod
    def forward(ctx, wide, narrow):
        out = wide.clone()
        out[:, : narrow.shape[1]].add_(narrow)
        ctx.cb = narrow.shape[1]
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g[:, : ctx.cb]


def _stacked_biases(join):
    """R = 2 components' biases stacked, joined and scaled, as stacked.py's bank hands them to ops.bias_join: the gradient
    that reaches the join is a tensor only autograd holds, and every parameter receives a contiguous row of it"""
    g = torch.Generator().manual_seed(9)
    inputs = {k: torch.randn(6 if k[0] == "w" else 2, generator=g) for k in ("w0", "w1", "n0", "n1")}
    return ac.Case(f"stacked biases through {getattr(join, '__name__', join)}", inputs, tuple(inputs),
                   lambda t: (join(torch.stack([t["w0"], t["w1"]]), torch.stack([t["n0"], t["n1"]])) * 1.5,),
                   (torch.randn(2, 6, generator=g),))


def test_two_backwards_accumulate_to_twice_one_and_no_two_grads_share_memory():
    """What the whole-model case of the GPU file found in ops.bias_join: AccumulateGrad kept two views of one gradient as
    the .grad of two parameters"""
    from ms_gat_amd import ops
    found = ac.check_accumulates(_stacked_biases(_ViewsOfOneGradient.apply))
    assert any("the .grad of n0 and of w0 share memory" in line for line in found), found
    assert any("are not twice one at grad['n0']" in line for line in found) and any("grad['w1']" in line for line in found), found
    assert ac.check_accumulates(_stacked_biases(ops.bias_join)) == []
    assert ac.check_accumulates(_toy(_Correct)) == []


# ---- the second problem leaves the first as it was ---------------------------------------------------------------------------
# crc32 over the input tensors (by name) and the cotangents of gs.problem(name), taken before `seed` existed
CHECKSUMS = {
    "mix 72->24 N=64 bias add relu": 0xb7aec4d6,
    "mix_multi relu premasked 5->9 N=13": 0x8bb7c080,
    "gate_sum time embedding N=13 To=7": 0xecb9bf93,
    "layer_norm_pool_tee fused C=72 N=64 relu_input=True": 0xccc969c5,
    "gacn PROJ_FIRST 72->24 N=64 with masked weights": 0xd8457991,
    "causal_conv 9->9 N=13 T=8 d=3 no bias": 0x4c07f591,
}


def _checksum(inputs, cots):
    c = 0
    for k in sorted(inputs):
        if torch.is_tensor(inputs[k]):
            c = zlib.crc32(inputs[k].contiguous().numpy().tobytes(), c)
    for t in cots:
        c = zlib.crc32(t.contiguous().numpy().tobytes(), c)
    return c


def test_the_seed_suffix_leaves_every_existing_problem_bit_identical():
    for name, want in CHECKSUMS.items():
        row, inputs, cots = gs.problem(name)
        assert _checksum(inputs, cots) == want, name
        assert _checksum(*gs.problem(name, 0)[1:]) == want and _checksum(*gs.problem(name, 0, 0)[1:]) == want
        assert _checksum(*gs.problem(name, 1)[1:]) != want
        assert pf.same_bits(gs.problem(name, 0, 1)[1], inputs) and not pf.same_bits(gs.problem(name, 0, 1)[2], cots)
    assert gs.seed_name("a row") == "a row" and gs.seed_name("a row", 1) == "a row seed 1"
    for row in gs.ROWS:                                     # same shapes, same plain values, the same graph
        first, second = row.make(), row.make(1)
        assert first.keys() == second.keys(), row.name
        for k, v in first.items():
            if torch.is_tensor(v):
                assert v.shape == second[k].shape and v.dtype == second[k].dtype, (row.name, k)
                assert (k == "adj") == bool(torch.equal(v, second[k])) or v.dtype != torch.float32, (row.name, k)
            else:
                assert v == second[k], (row.name, k)
    a, b = gs.model_problem("msgat48", 1), gs.model_problem("msgat48", 1, seed=1)
    again = gs.model_problem("msgat48", 1, seed=0)
    assert pf.same_bits(list(a[1:]), list(again[1:])) and pf.same_bits(dict(a[0].state_dict()), dict(again[0].state_dict()))
    assert not pf.same_bits(a[1], b[1]) and not pf.same_bits(a[0].state_dict()["te.h_ebd.weight"], b[0].state_dict()["te.h_ebd.weight"])


# ---- census: every Function of ops.py is run by a case ------------------------------------------------------------------------

def test_every_autograd_function_of_ops_is_run_by_a_case_of_the_gpu_file():
    gaps = ac.census(_read(OPS), _read(GPU_MODULE), gs.ROWS)
    print("\n".join(gaps))
    assert not gaps, "\n".join(gaps)
    classes = ac.function_classes(_read(OPS))
    assert len(classes) >= 23 and set(ac.OTHER_FUNCTIONS) == set(gs.EXCLUDED) and set(ac.FORM_ROWS) == {r.function for r in gs.ROWS}
    assert set(classes) == set(ac.OTHER_FUNCTIONS) | set(ac.FORM_ROWS)
    names = [r.name for r in gs.ROWS]
    assert all(n in names for n in ac.FORM_ROWS_MORE)
    for f, (name, why) in ac.FORM_ROWS.items():            # the N = 64 row where the Function has one
        has64 = any(r.function == f and "N=64" in r.name for r in gs.ROWS)
        assert ("N=64" in name) == has64 or f in ("_ChannelAttentionMixFunction",), (f, name)
        assert why in ("copy first", "stride argument", "accepted in place", "views")
    # the GPU file runs (a)-(d) over the whole table, (e) over FORM_ROWS, (f) over OTHER_FUNCTIONS
    src = _read(GPU_MODULE)
    for needle in ("gs.ROWS", "ac.FORM_ROWS", "ac.OTHER_FUNCTIONS", "check_operands_intact", "check_repeatable",
                   "check_one_output_at_a_time", "check_interleaved", "check_cotangent_forms"):
        assert needle in src, needle


def test_the_census_fails_when_a_function_leaves_the_case_table_or_a_new_one_arrives():
    ops_src, gpu_src = _read(OPS), _read(GPU_MODULE)
    without = [r for r in gs.ROWS if r.function != "_TimeMixFunction"]
    assert any("_TimeMixFunction" in g and "no case" in g for g in ac.census(ops_src, gpu_src, without))
    other = {k: v for k, v in ac.OTHER_FUNCTIONS.items() if k != "_EdgeDropoutFunction"}
    assert any("_EdgeDropoutFunction" in g for g in ac.census(ops_src, gpu_src, gs.ROWS, other=other))
    forms = {k: v for k, v in ac.FORM_ROWS.items() if k != "_GACNFunction"}
    assert any("_GACNFunction" in g and "cotangent forms" in g for g in ac.census(ops_src, gpu_src, gs.ROWS, form_rows=forms))
    added = ops_src + "\n\nclass _AddedFunction(torch.autograd.Function):\n    pass\n"
    assert any("_AddedFunction" in g for g in ac.census(added, gpu_src, gs.ROWS))
    assert any("ops.edge_dropout" in g for g in ac.census(ops_src, gpu_src.replace("ops.edge_dropout(", "ops.edge_dropped("), gs.ROWS))


# ---- census: what the GPU file calls read-only is const in the header -------------------------------------------------------
_ENTRY = re.compile(r"^[ \t]+(msgat_\w+)[ \t]+read only: ([\w, ]*?); written:[ \t]*([\w, ]*?)[ \t]*$", re.M)


def _documented():
    """{entry point or struct: (read-only names, written names)} of the GPU file's docstring"""
    import ast
    doc = ast.get_docstring(ast.parse(_read(GPU_MODULE)))
    split = lambda s: [n.strip() for n in s.split(",") if n.strip()]          # noqa: E731
    return {m.group(1): (split(m.group(2)), split(m.group(3))) for m in _ENTRY.finditer(doc)}


def _declared(header, name):
    """[(parameter or field name, is a pointer, is const)] of an entry point or a struct of the header, comments stripped"""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    m = re.search(r"typedef struct\s*\w*\s*\{([^}]*)\}\s*%s\s*;" % name, text) if name.endswith("_t") else \
        re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
    assert m, f"{name} is not declared in include/msgat_hip.h"
    out = []
    for decl in re.split(r"[;,]", m.group(1)):
        decl = " ".join(decl.split())
        if decl:
            out.append((re.split(r"[ *]", decl)[-1], "*" in decl, decl.startswith("const ")))
    return out


def _header_problems(header, documented):
    problems = []
    for name, (read_only, written) in documented.items():
        params = {p: (ptr, const) for p, ptr, const in _declared(header, name)}
        for p in read_only:
            if p not in params or not params[p][0]:
                problems.append(f"{name}: `{p}` is no pointer parameter")
            elif not params[p][1]:
                problems.append(f"{name}: `{p}` is listed as read only and is not const")
        pointers = {p for p, (ptr, _) in params.items() if ptr and p != "stream"}
        if set(read_only) | set(written) != pointers:
            problems.append(f"{name}: the docstring lists {sorted(set(read_only) | set(written))}, the header has {sorted(pointers)}")
        problems += [f"{name}: `{p}` is listed as written and is const" for p in written if p in params and params[p][1]]
    return problems


def test_every_pointer_the_gpu_file_calls_read_only_is_const_in_the_header():
    import ast
    header, documented = _read(HEADER), _documented()
    assert len(documented) >= 35 and "msgat_bwd_t" in documented and documented["msgat_gacn_backward"] == (["shape", "graph", "io"], [])
    problems = _header_problems(header, documented)
    assert not problems, "\n".join(problems)
    # every library call of a backward in ops.py is documented
    called = set()
    for cls in ast.parse(_read(OPS)).body:
        if isinstance(cls, ast.ClassDef) and cls.name in ac.function_classes(_read(OPS)):
            for fn in cls.body:
                if isinstance(fn, ast.FunctionDef) and fn.name == "backward":
                    called |= {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and n.attr.startswith("msgat_")
                               and not re.search(r"(_floats|_bytes|_doubles|accepts_strided_d[zv])$", n.attr)}
    assert len(called) >= 25 and called <= set(documented), sorted(called - set(documented))
    # the parse has teeth: a cotangent that loses its const, a written pointer the docstring leaves out
    assert ("x", True, True) in _declared(header, "msgat_layernorm_backward") and ("dx", True, False) in _declared(header, "msgat_layernorm_backward")
    broken = re.sub(r"const float\*\s*dy\b", "float* dy", header)
    assert "msgat_layernorm_backward: `dy` is listed as read only and is not const" in _header_problems(broken, documented)
    fewer = dict(documented, msgat_head_grad_signal=(["dout", "W"], []))
    assert any(p.startswith("msgat_head_grad_signal: the docstring lists") for p in _header_problems(header, fewer))


# ---- the conditions hold for the reference alone ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [r.name for r in gs.ROWS], ids=gs.ROW_IDS)
def test_restatement_in_fp32_meets_the_bars_of_cases_b_and_c_and_the_second_problem_differs(name):
    row, inputs, cots = gs.problem(name)
    # (b): the first problem's forward with the second problem's cotangent; (c): all outputs together
    for cot_seed in (1, None):
        o64, g64 = gs.reference(name, row.diff, None, torch.float64, 0, cot_seed)
        o32, g32 = gs.reference(name, row.diff, None, torch.float32, 0, cot_seed)
        for k in row.diff:
            ok, e = meets(row.bar, g32[k], g64[k])
            assert ok, (cot_seed, k, e)
    # teeth: the second problem, and the second cotangent alone, move every output and gradient by more than 1e-2
    first, second, other = gs.reference(name, row.diff), gs.reference(name, row.diff, None, torch.float64, 1), \
        gs.reference(name, row.diff, None, torch.float64, 0, 1)
    for i, (a, b) in enumerate(zip(first[0], second[0])):
        assert rel_err(a, b) > 1e-2, ("output", i, rel_err(a, b))
    for k in row.diff:
        assert rel_err(first[1][k], second[1][k]) > 1e-2, (k, rel_err(first[1][k], second[1][k]))
        assert rel_err(first[1][k], other[1][k]) > 1e-2, (k, "cotangent", rel_err(first[1][k], other[1][k]))


def test_the_relu_masking_leaves_out_what_the_problem_leaves_out():
    """The third backward of case (b) takes the second problem's draw masked by the FIRST problem's pre-activations: the
    same entries are zero as in the first problem's own cotangent, a few in 1e5"""
    rows = [r for r in gs.ROWS if r.pre is not None]
    assert len(rows) >= 4
    for r in rows:
        for seed in (0, 1):
            _, inputs, cots = gs.problem(r.name, seed)
            _, _, other = gs.problem(r.name, seed, 1 - seed)
            t64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in inputs.items()}
            for pre, c, o in zip(r.pre(t64), cots, other):
                near = pre.abs() <= gs.MARGIN
                share = float(near.double().mean())
                print(f"{r.name} seed {seed}: {share:.2e} of the entries within MARGIN of the kink")
                assert share < 1e-3
                assert not bool(c[near].any()) and not bool(o[near].any())
                assert bool(torch.equal(c == 0, o == 0))
                if not r.premasked:
                    assert float((c == 0).double().mean()) == share


def _adjacency_problem(C, O, form, seed=0):
    from test_gpu_adjacency_grad import _case, _learned_adjacency
    N, T, B = 64, 12, 2
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=seed + C + O)
    adj = _learned_adjacency(N, seed=seed + 17, V={"1nn": 1, "bnn": B}.get(form))
    return x, dz, Wg, alpha, W, adj


@pytest.mark.parametrize("form", ["nn", "bnn"])
@pytest.mark.parametrize("C,O", [(72, 24), (3, 24)], ids=["proj_first", "agg_first"])
def test_adjacency_restatement_in_fp32_meets_parity_and_a_write_has_teeth(C, O, form):
    """Case (g): oracle/dense_torch.py in fp32 meets conftest.assert_parity's two bars against float64 at the loss
    0.5 |z - target|^2, at the first and the second problem's values; and the two writes of the stale-state case (values
    scaled; every zero filled) move z and dadj by more than 1e-2"""
    x, dz, Wg, alpha, W, adj = _adjacency_problem(C, O, form)
    scaled = adj * _factors(adj.shape, 5)
    filled = np.where(adj == 0, np.float32(0.05), adj * np.float32(1.5)).astype(np.float32)
    refs = {}
    for what, a in (("old", adj), ("scaled", scaled), ("filled", filled)):
        refs[what] = want = ac.gacn_reference(x, alpha, Wg, W, a, target=dz)
        got = ac.gacn_reference(x, alpha, Wg, W, a, target=dz, dtype=torch.float32)
        for k in want:
            e = rel_err(got[k], want[k])
            assert e < 1e-4 and elementwise_violations(got[k], want[k], 1e-4, 1e-5) == 0.0, (what, k, e)
    for what in ("scaled", "filled"):
        for k in ("z", "dadj"):
            assert rel_err(refs["old"][k], refs[what][k]) > 1e-2, (what, k)
    # a fixed cotangent (cases (a), (b), (d)): parity as well, and the second problem differs
    want = ac.gacn_reference(x, alpha, Wg, W, adj, dz=dz)
    got = ac.gacn_reference(x, alpha, Wg, W, adj, dz=dz, dtype=torch.float32)
    x2, dz2, Wg2, alpha2, W2, adj2 = _adjacency_problem(C, O, form, seed=1)
    second = ac.gacn_reference(x2, alpha2, Wg2, W2, adj2, dz=dz2)
    for k in want:
        assert rel_err(got[k], want[k]) < 1e-4 and elementwise_violations(got[k], want[k], 1e-4, 1e-5) == 0.0, k
        assert rel_err(want[k], second[k]) > 1e-2, k


def _factors(shape, seed):
    """test_gpu_adjacency_coherence.py's: a factor per entry, none inside [0.8, 1.25]"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.5, rng.uniform(0.3, 0.8, shape), rng.uniform(1.25, 3.0, shape)).astype(np.float32)


def test_reversed_rows_is_not_the_library_order():
    from test_gpu_adjacency_grad import _learned_adjacency
    adj = _learned_adjacency(13, seed=3)
    crow, rows, cols = ac.reversed_rows(adj)
    assert crow[-1] == len(rows) == np.count_nonzero(adj) and (adj[rows, cols] != 0).all()
    assert all((np.diff(cols[crow[i]:crow[i + 1]]) < 0).all() for i in range(13)) and (np.diff(rows) >= 0).all()
    assert any(crow[i + 1] - crow[i] > 1 for i in range(13))


def test_whole_model_restatement_in_fp32_meets_the_bar_with_everything_trainable():
    """Case (h): one backward per forecast horizon adds up to the backward of the whole cotangent (the columns of `dout`
    partition it), so the reference is gs.model_reference at `dout`; in fp32 it is within 1e-4 of float64, and the second
    model differs from the first by more than 1e-2"""
    net, X, H, D, dout = gs.model_problem("msgat48", 1)
    p64, g64, _ = gs.model_reference(net, X, H, D, dout, torch.float64, False)
    p32, g32, _ = gs.model_reference(net, X, H, D, dout, torch.float32, False)
    assert rel_err(p32, p64) < 1e-4 and len(g64) == len(list(net.parameters())) - 1        # all but the frozen adjacency
    for k in g64:
        assert rel_err(g32[k], g64[k]) < 1e-4, k
    columns = sum(dout * (torch.arange(gs.MODEL_T) == t) for t in range(gs.MODEL_T))
    assert torch.equal(columns, dout)
    net2, X2, H2, D2, dout2 = gs.model_problem("msgat48", 1, seed=1)
    q64, h64, _ = gs.model_reference(net2, X2, H2, D2, dout2, torch.float64, False)
    assert rel_err(p64, q64) > 1e-2
    flat = [k for k in g64 if not bool(g64[k].any()) and not bool(h64[k].any())]
    # with one input channel the first block's channel attention is a softmax over one channel: its Wc and alpha get exactly 0
    assert flat == [f"tpcs.{r}.tgacns.0.cacn.seq.0.{p}" for r in range(gs.MODEL_R) for p in ("Wc", "alpha")]
    assert all(rel_err(g64[k], h64[k]) > 1e-2 for k in g64 if k not in flat)
