"""No GPU: the harness of the poisoned-buffer tests (poison_fixtures.py) catches what it should, and two censuses by `ast`
keep it honest -- every call of the package that returns uninitialised memory is one of the three spellings the harness
patches, and everything in the package that allocates such memory or hands a buffer to the library is run by a case of
test_gpu_poisoned_buffers.py."""
import ast
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import grad_subset_fixtures as gs
import poison_fixtures as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "ms_gat_amd")
GPU_MODULE = os.path.join(ROOT, "tests", "test_gpu_poisoned_buffers.py")
FIXTURES = os.path.join(ROOT, "tests", "grad_subset_fixtures.py")


# ---- the harness ---------------------------------------------------------------------------------------------------------

def _toy(reads_unwritten, device="cpu"):
    """A reduction over a workspace of five slots of which four are written: the wrong one sums all five"""
    ws = torch.empty(5, device=device)
    ws[:4] = torch.tensor([1.0, 2.0, 3.0, 4.0], device=device)
    return ws[:5 if reads_unwritten else 4].sum()


def test_the_harness_catches_a_read_of_an_unwritten_slot_and_passes_the_correct_op():
    bad = pf.run_under_fills(lambda: _toy(True))
    good = pf.run_under_fills(lambda: _toy(False))
    assert float(bad[0]) == 10.0 and bool(torch.isnan(bad[1])) and 3.3e38 < float(bad[2]) < 3.41e38
    assert not pf.same_bits(bad[0], bad[1]) and not pf.same_bits(bad[0], bad[2]) and not pf.same_bits(bad[1], bad[2])
    with pytest.raises(AssertionError, match="fill 0xFF"):
        pf.check_fills(bad, "toy")
    assert [float(g) for g in good] == [10.0] * 3
    pf.check_fills(good, "toy")


def test_a_finite_result_that_turns_non_finite_is_named():
    assert pf.nonfinite_where_finite(torch.zeros(3), torch.tensor([0.0, float("nan"), float("inf")]))
    assert not pf.nonfinite_where_finite(torch.tensor([float("nan")]), torch.tensor([float("nan")]))


def test_every_patched_spelling_is_filled_in_every_type():
    like = torch.zeros(2, 3)
    for byte, integer in zip(pf.FILLS, (0, 1, 2)):
        with pf.poisoned(byte):
            made = [torch.empty(2, 3), torch.empty((2, 3), dtype=torch.float64), torch.empty_like(like), like.new_empty((4,)),
                    torch.empty(7, dtype=torch.float16), torch.empty_like(like.t()), torch.empty(3, requires_grad=True),
                    torch.empty(5, dtype=torch.uint8), torch.empty(()), torch.empty((), dtype=torch.float64)]
            ints = [torch.empty(3, dtype=torch.int64), torch.empty((2, 2), dtype=torch.int32), like.new_empty(2, dtype=torch.int16)]
            flag = torch.empty(3, dtype=torch.bool)
            nothing = torch.empty(0)
            meta = torch.empty(3, device="meta")
        for t in made:
            assert bool((t.detach().contiguous().reshape(-1).view(torch.uint8) == byte).all()), (byte, t.dtype, t.stride())
        assert made[5].stride() == like.t().stride() and made[6].requires_grad and made[6].grad_fn is None
        for t in ints:
            assert bool((t == integer).all()), (byte, t.dtype)
        assert bool((flag == bool(byte)).all())
        assert nothing.numel() == 0 and meta.is_meta
    with pf.poisoned(0xFF):
        assert bool(torch.isnan(torch.empty(2)).all()) and bool(torch.isnan(torch.empty(2, dtype=torch.float64)).all())
    with pf.poisoned(0x7F):
        assert 3.3e38 < float(torch.empty(1)) < 3.41e38 and 1.3e306 < float(torch.empty(1, dtype=torch.float64)) < 1.4e306


def test_the_originals_are_back_after_a_normal_exit_and_after_an_exception():
    originals = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pf.poisoned(0xFF):
        assert torch.empty is not originals[0] and torch.empty_like is not originals[1]
        assert torch.Tensor.new_empty is not originals[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals
    with pytest.raises(KeyError):
        with pf.poisoned(0x7F):
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals
    assert torch.empty is originals[0] and torch.empty_like is originals[1] and torch.Tensor.new_empty is originals[2]


def test_the_patch_holds_through_modules_optimizers_and_autograd():
    def step():
        torch.manual_seed(0)
        net = nn.Sequential(nn.Linear(6, 5), nn.ReLU(), nn.Linear(5, 3))
        opt = torch.optim.Adam(net.parameters(), lr=1e-2)
        x = torch.randn(4, 6)
        for _ in range(2):
            opt.zero_grad()
            F.layer_norm(net(x), [3]).square().sum().backward()
            opt.step()
        return [p.detach().clone() for p in net.parameters()]
    pf.check_fills(pf.run_under_fills(step), "a torch training step")


def test_same_bits_compares_words_and_containers():
    nan = torch.tensor([float("nan"), 1.0])
    other = nan.clone()
    assert pf.same_bits(nan, other) and not torch.equal(nan, other)
    other.view(torch.int32)[0] ^= 1                              # another NaN
    assert not pf.same_bits(nan, other)
    assert not pf.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not pf.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64)) and not pf.same_bits(torch.zeros(2), torch.zeros(3))
    assert pf.same_bits(None, None) and not pf.same_bits(None, nan) and not pf.same_bits(nan, None)
    assert pf.same_bits((nan, {"a": nan, "b": None}), (nan.clone(), {"a": nan.clone(), "b": None}))
    assert not pf.same_bits((nan, {"a": nan}), (nan, {"a": other})) and not pf.same_bits((nan,), (nan, nan))
    assert pf.same_bits(torch.tensor([3, 4]), torch.tensor([3, 4])) and pf.same_bits(torch.tensor(True), torch.tensor(True))
    assert pf.differences({"a": (nan, nan)}, {"a": (nan, other)}) == ["result['a'][1]: 1 of 2 words differ, the first at [0]"]


def test_the_keyed_walk_runs_every_key_under_every_fill_and_shuffles_the_later_ones():
    seen = []

    def fn(key):
        seen.append(key)
        if key == 3:
            raise ValueError("key 3")
        return torch.empty(1) * 0 + key
    keys = list(range(8))
    out = pf.run_under_fills(fn, order=keys)
    assert seen[:8] == keys and sorted(seen[8:16]) == keys and sorted(seen[16:]) == keys and seen[8:16] != keys
    assert float(out[5][0]) == 5.0 and bool(torch.isnan(out[5][1]))          # 0xFF: NaN * 0
    with pytest.raises(ValueError, match="key 3"):
        pf.check_fills(out[3])


# ---- census 1: every call that returns uninitialised memory is a spelling the harness patches ------------------------------
PATCHED = ("torch.empty", "torch.empty_like")                   # and <tensor>.new_empty
_LEGACY = re.compile(r"^(Float|Double|Half|BFloat16|Int|Long|Short|Byte|Char|Bool)?(Tensor|Storage)$|^(Untyped|Typed)Storage$")
_UNINITIALISED = {"resize_", "resize_as_", "resize", "new", "from_file", "ndarray"}


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    parts.append(node.id if isinstance(node, ast.Name) else "<expr>")
    return ".".join(reversed(parts))


def _is_allocation_name(last):
    return (last == "empty" or last.startswith(("empty_", "new_empty", "_empty")) or last in _UNINITIALISED
            or bool(_LEGACY.match(last)))


def allocation_sites(source, filename="<source>"):
    """-> [(line, spelling, whether the harness reaches it)] of every call in `source` that returns uninitialised memory,
    plus every mention of a patched spelling that is not a call of it (an alias, a default argument, `from torch import
    empty`: bound once, the patch would not reach it)"""
    tree = ast.parse(source, filename)
    sites, called = [], set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, (ast.Attribute, ast.Name)):
            name = _dotted(node.func)
            called.add(id(node.func))
            last = name.rsplit(".", 1)[-1]
            if _is_allocation_name(last) or "._C." in name:
                ok = name in PATCHED or (last == "new_empty" and isinstance(node.func, ast.Attribute))
                sites.append((node.lineno, name, ok))
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and id(node) not in called and node.attr in ("empty", "empty_like", "new_empty") \
                and _dotted(node).startswith("torch"):
            sites.append((node.lineno, _dotted(node) + " (not called here)", False))
        if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[0] == "torch":
            sites += [(node.lineno, f"from {node.module} import {a.name}", False) for a in node.names
                      if _is_allocation_name(a.name)]
    return sorted(sites)


def _package_files(package=PACKAGE):
    return sorted(os.path.join(package, f) for f in os.listdir(package) if f.endswith(".py"))


def unpatched_sites(package=PACKAGE):
    out = []
    for path in _package_files(package):
        with open(path) as f:
            out += [f"{os.path.relpath(path, os.path.dirname(package))}:{line}: {name}"
                    for line, name, ok in allocation_sites(f.read(), path) if not ok]
    return out


def test_the_allocation_census_knows_the_spellings_the_harness_does_not_reach():
    bad = ["torch.empty_strided((2,), (1,))", "x.new_empty_strided((2,), (1,))", "x.resize_(4)", "torch.Tensor(3)",
           "torch.FloatTensor(3)", "torch.cuda.FloatTensor(3)", "x.new(3)", "torch._C._nn.something(x)", "np.empty(3)",
           "torch.empty_permuted((2, 3), (1, 0))", "empty(3)", "torch.UntypedStorage(8)", "alias = torch.empty",
           "def f(make=torch.empty_like): pass", "from torch import empty", "from torch import empty_like as e"]
    for line in bad:
        sites = allocation_sites(line)
        assert sites and not any(ok for _, _, ok in sites), line
    for line in ["torch.empty(3)", "torch.empty_like(x)", "x.new_empty((3,))", "torch.empty((2, 3), device=d, dtype=torch.uint8)"]:
        assert [ok for _, _, ok in allocation_sites(line)] == [True], line
    for line in ["torch.zeros(3)", "x.is_empty()", "torch.full((3,), 1.0)", "'non-empty'", "renew(3)"]:
        assert allocation_sites(line) == [], line


def test_every_uninitialised_allocation_of_the_package_is_a_patched_spelling():
    """A spelling listed here must be patched in poison_fixtures.poisoned or rewritten as one of the three it patches"""
    found = unpatched_sites()
    print("\n".join(found))
    assert not found, "uninitialised memory the poisoned-buffer tests do not reach:\n" + "\n".join(found)
    with open(os.path.join(PACKAGE, "ops.py")) as f:
        assert sum(ok for _, _, ok in allocation_sites(f.read())) >= 60          # the walk does see them


def test_the_gpu_module_documents_every_allocation_site():
    """Its docstring says, per site, what is carved from the allocation and where it is written before it is read: every
    class or function of the package that holds such a call is named there"""
    with open(GPU_MODULE) as f:
        doc = ast.get_docstring(ast.parse(f.read()))
    missing = []
    for path in _package_files():
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for top in tree.body:
            if isinstance(top, (ast.FunctionDef, ast.ClassDef)) and any(
                    isinstance(n, ast.Call) and isinstance(n.func, (ast.Attribute, ast.Name))
                    and _is_allocation_name(_dotted(n.func).rsplit(".", 1)[-1]) for n in ast.walk(top)):
                if not re.search(rf"(?<![A-Za-z0-9_]){re.escape(top.name)}(?![A-Za-z0-9])", doc):
                    missing.append(f"{os.path.basename(path)}: {top.name}")
    assert not missing, missing


# ---- census 2: everything that allocates or launches is run by a case ------------------------------------------------------
# A torch.autograd.Function of ops.py that no case names: the one admissible reason is that it allocates nothing
# uninitialised and calls no library entry point, which `coverage_gaps` checks against its body.
EXCLUDED = {}


def _code_nodes(node):
    """ast.walk without docstrings (they name library entry points)"""
    for child in ast.walk(node):
        if isinstance(child, ast.Expr) and isinstance(child.value, ast.Constant) and isinstance(child.value.value, str):
            continue
        yield child


def _hands_over_a_buffer(call):
    """Whether a call passes a device address: `_ptr(t)`, `t.data_ptr()`, `C.byref(...)` or an unpacked argument list"""
    for arg in list(call.args) + [k.value for k in call.keywords]:
        for n in ast.walk(arg):
            if isinstance(n, ast.Starred):
                return True
            if isinstance(n, ast.Call) and _dotted(n.func).rsplit(".", 1)[-1] in ("_ptr", "data_ptr", "byref"):
                return True
    return False


def _directly_dirty(node):
    """Whether the body allocates uninitialised memory itself or launches a library entry point on a buffer"""
    for n in _code_nodes(node):
        if isinstance(n, ast.Call) and isinstance(n.func, (ast.Attribute, ast.Name)):
            name = _dotted(n.func)
            last = name.rsplit(".", 1)[-1]
            if _is_allocation_name(last):
                return True
            if last.startswith("msgat_") and _hands_over_a_buffer(n):
                return True
        if isinstance(n, ast.JoinedStr) and n.values and isinstance(n.values[0], ast.Constant) \
                and str(n.values[0].value).startswith("msgat_"):
            return True                                         # getattr(L, f"msgat_{stem}_metrics")(...)
    return False


def _is_function_class(node):
    return isinstance(node, ast.ClassDef) and any(_dotted(b).endswith("autograd.Function") for b in node.bases
                                                  if isinstance(b, (ast.Attribute, ast.Name)))


def _module(path):
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    return {n.name: n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}


def _reached(defs, start):
    """The names of `defs` reachable from `start` through the names their bodies mention"""
    seen, todo = set(), [s for s in start if s in defs]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        todo += [n.id for n in ast.walk(defs[name]) if isinstance(n, ast.Name) and n.id in defs and n.id not in seen]
    return seen


def _named_by_the_cases(ops_defs, gpu_module=GPU_MODULE):
    """What the cases name: `ops.<name>` in the GPU module and in the op table's fixtures, the strings the fixtures hand to
    `getattr(ops, ...)`, and each table row's Function"""
    named = {r.function for r in gs.ROWS}
    for path in (gpu_module, FIXTURES):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for n in _code_nodes(tree):
            if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "ops":
                named.add(n.attr)
            if path == FIXTURES and isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value in ops_defs:
                named.add(n.value)
    return named


def coverage_gaps(package=PACKAGE, gpu_module=GPU_MODULE, excluded=EXCLUDED):
    defs = _module(os.path.join(package, "ops.py"))
    reached = _reached(defs, _named_by_the_cases(defs, gpu_module))
    gaps = []
    for name, node in defs.items():
        dirty = _directly_dirty(node)
        if name in excluded:
            if dirty or name in reached:
                gaps.append(f"ops.{name} is excluded ({excluded[name]}) but "
                            + ("allocates or launches (line %d)" % node.lineno if dirty else "is run by a case"))
        elif name not in reached and (dirty or _is_function_class(node)):
            gaps.append(f"ops.{name} (line {node.lineno}) "
                        + ("allocates uninitialised memory or launches a kernel" if dirty else "is an autograd.Function")
                        + " and no case of test_gpu_poisoned_buffers.py runs it")
    # the optimizer: every public method of FlatAdam that launches, and each of its forms
    eng = _module(os.path.join(package, "engine.py"))
    with open(gpu_module) as f:
        tree = ast.parse(f.read(), gpu_module)
    attrs = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)}
    keywords = {k.arg for n in ast.walk(tree) if isinstance(n, ast.Call) for k in n.keywords} | \
        {k.value for n in ast.walk(tree) if isinstance(n, ast.Dict) for k in n.keys if isinstance(k, ast.Constant)}
    for method in eng["FlatAdam"].body:
        if isinstance(method, ast.FunctionDef) and not method.name.startswith("_") and _directly_dirty(method) \
                and method.name not in attrs:
            gaps.append(f"engine.FlatAdam.{method.name} launches a kernel and no case calls it")
    for need in ("FlatAdam", "accumulate", "swap_averaged", "step"):
        if need not in attrs:
            gaps.append(f"engine.FlatAdam: no case uses `{need}`")
    for form in ("max_grad_norm", "skip_nonfinite", "ema_decay", "rank_weight", "accumulate_steps"):
        if form not in keywords:
            gaps.append(f"engine.FlatAdam: no case runs the form `{form}`")
    return gaps


def test_every_op_that_allocates_or_launches_is_run_by_a_case():
    gaps = coverage_gaps()
    print("\n".join(gaps))
    assert not gaps, "\n".join(gaps)
    defs = _module(os.path.join(PACKAGE, "ops.py"))
    functions = [n for n, d in defs.items() if _is_function_class(d)]
    launchers = ["window_gather", "window_gather_imputed", "ring_push", "ring_windows", "forecast_store", "forecast_score",
                 "huber_metrics", "gauss_metrics", "masked_huber_metrics", "masked_gauss_metrics", "quantile_metrics",
                 "edge_adjacency"]
    named = _named_by_the_cases(defs)
    assert len(functions) >= 23 and all(_directly_dirty(defs[n]) or n in ("_BiasJoinFunction", "_Relayout") for n in functions)
    assert all(n in named for n in launchers), [n for n in launchers if n not in named]
    assert all(_directly_dirty(defs[n]) for n in ("_window_gather", "ring_push", "forecast_score", "_map_grad", "_AdjacencyGrad"))
    assert not _directly_dirty(defs["channel_attention_fused"]) and not _directly_dirty(defs["edge_validity_table"])


def test_the_censuses_fail_on_a_scratch_copy_with_an_unpatched_spelling_or_an_op_without_a_case(tmp_path):
    import shutil
    pkg = tmp_path / "ms_gat_amd"
    shutil.copytree(PACKAGE, pkg, ignore=shutil.ignore_patterns("*.so*", "__pycache__", "csrc"))
    with open(pkg / "ops.py", "a") as f:
        f.write("\n\nclass _AddedFunction(torch.autograd.Function):\n    @staticmethod\n    def forward(ctx, x):\n"
                "        out = torch.empty_strided(x.shape, x.stride(), device=x.device)\n"
                "        _lib.check(_lib.lib().msgat_added(_ptr(x), _ptr(out)), 'msgat_added')\n        return out\n\n\n"
                "def added_op(x):\n    ws = torch.empty(8, device=x.device)\n    return _lib.lib().msgat_added_op(_ptr(x), _ptr(ws))\n")
    assert any("empty_strided" in s and "ops.py" in s for s in unpatched_sites(str(pkg)))
    gaps = coverage_gaps(str(pkg))
    assert any("_AddedFunction" in g for g in gaps) and any("added_op" in g for g in gaps), gaps
