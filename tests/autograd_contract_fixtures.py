"""What the autograd-contract tests (test_gpu_autograd_contract.py, test_autograd_contract_cpu.py) share.

The contract of every torch.autograd.Function of ms_gat_amd/ops.py: a forward leaves its inputs as they were; a backward
leaves inputs, outputs, everything the node saved and the cotangents it was handed as they were; a backward can be run
again (`retain_graph=True`) and gives the same bits, and with another cotangent what a fresh forward + backward with that
cotangent gives; two forwards may run before the first backward, in either order of the backwards; the cotangent may
arrive in any layout autograd delivers.

A `Case` is one op at one problem, device-agnostic: the checks below run the library's ops on the GPU and the toy
Functions of the CPU test alike.  Every check returns the list of what it found (empty: the contract holds); bars
against a float64 reference are the caller's, applied to the gradients a check hands back.  Nothing is compared with a
tolerance here: the library has no float atomics and fixed summation orders (poison_fixtures.py)."""
import contextlib
import dataclasses
from typing import Callable

import torch

import poison_fixtures as pf


# ---- snapshot and compare ------------------------------------------------------------------------------------------------

def snapshot(tensors):
    """Bit copies of every tensor of a nested dict / list / tuple, in memory of their own; anything else as it is"""
    if isinstance(tensors, torch.Tensor):
        return tensors.detach().clone()
    if isinstance(tensors, dict):
        return {k: snapshot(v) for k, v in tensors.items()}
    if isinstance(tensors, (list, tuple)):
        return type(tensors)(snapshot(v) for v in tensors)
    return tensors


def changed(before, tensors, path="operand"):
    """The paths at which `tensors` no longer hold the bits of their `snapshot` `before`"""
    return pf.differences(before, tensors, path)


@contextlib.contextmanager
def saved_tensors():
    """Yields the list of every tensor an autograd node saves inside the block, in order.  The pack hook hands back the
    tensor itself, so the graph keeps what it would have kept: the carved buffer of the graph attention, a stored
    LayerNorm output, a ReLU output -- the very memory a later backward re-reads."""
    seen = []

    def pack(t):
        seen.append(t)
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        yield seen


# ---- cotangent forms -----------------------------------------------------------------------------------------------------
FORMS = ("contiguous", "expanded", "channel_slice", "permuted", "own_storage")


def cotangent_form(form, out, cot):
    """-> (c, holder, dense) or None where the form does not exist for this output.  `c`: a cotangent for the output `out` in
    the layout `form`; `holder`: the wider tensor it is a view of (or None); `dense`: a contiguous tensor of c's values in
    memory of its own -- what the comparison run is handed.
      contiguous     `cot` itself, copied
      expanded       one constant expanded to the output's shape, every stride 0: what `.sum().backward()` delivers
      channel_slice  [:, a:a+C] of a contiguous tensor with a channels before and b behind, all NaN: what the backward of
                     `torch.cat(..., dim=1)` delivers; a NaN in any gradient is a read outside the slice
      permuted       the values of `cot` in reversed-axes memory order, viewed back: not contiguous, no axis of stride 0
      own_storage    the output's own memory (`out.detach()`): the cotangent of 0.5 * out^2"""
    cot = cot.to(out.device)
    if form == "contiguous":
        c, holder = cot.clone(), None
    elif form == "expanded":
        c, holder = torch.full((), 0.75, device=out.device, dtype=out.dtype).expand(out.shape), None
    elif form == "channel_slice":
        if out.dim() < 2:
            return None
        a, b, C = 3, 2, out.shape[1]
        holder = torch.full((out.shape[0], a + C + b) + tuple(out.shape[2:]), float("nan"), device=out.device, dtype=out.dtype)
        holder[:, a:a + C] = cot
        c = holder[:, a:a + C]
    elif form == "permuted":
        if out.dim() < 2 or out.numel() == max(out.shape):
            return None
        axes = tuple(reversed(range(out.dim())))
        holder = cot.permute(*axes).contiguous()
        c = holder.permute(*axes)
        assert c.shape == out.shape and not c.is_contiguous()
    elif form == "own_storage":
        c, holder = out.detach(), None
    else:
        raise ValueError(form)
    return c, holder, c.detach().clone().contiguous()


# ---- a case and its runs ---------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Case:
    """One op at one problem"""
    name: str
    inputs: dict                        # input name -> CPU tensor | None | plain value; every run gets fresh copies
    diff: tuple                         # the inputs that require grad
    call: Callable                      # ({input name: leaf on the device}) -> tuple of outputs
    cots: tuple                         # a CPU cotangent per output
    device: torch.device = torch.device("cpu")
    allowed: dict = dataclasses.field(default_factory=dict)      # input name -> the documented side effect of the forward on it
    guard: Callable = contextlib.nullcontext                      # around every run (the GPU file: device errors end the session)

    def leaves(self):
        out = {}
        for k, v in self.inputs.items():
            if torch.is_tensor(v):
                v = v.detach().clone().to(self.device)
                if k in self.diff:
                    v.requires_grad_(True)
            out[k] = v
        return out

    def cotangents(self, cots=None):
        return [c.detach().clone().to(self.device) for c in (self.cots if cots is None else cots)]

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()


@dataclasses.dataclass
class Step:
    """A forward whose backward has not run yet"""
    case: Case
    leaves: dict
    outs: tuple
    saved: list

    def sel(self):
        return [i for i, o in enumerate(self.outs) if o.requires_grad]

    def backward(self, cots=None, retain=False):
        """-> {differentiable input: fresh gradient | None} by torch.autograd.grad; `cots`: one per output, on the device"""
        case = self.case
        cots = case.cotangents() if cots is None else cots
        sel = self.sel()
        with case.guard():
            grads = torch.autograd.grad([self.outs[i] for i in sel], [self.leaves[k] for k in case.diff], [cots[i] for i in sel],
                                        retain_graph=retain, allow_unused=True)
            case.sync()
        return dict(zip(case.diff, grads))

    def outputs(self):
        return tuple(o.detach() for o in self.outs)


def forward(case):
    with case.guard():
        leaves = case.leaves()
        with saved_tensors() as saved:
            outs = tuple(case.call(leaves))
        case.sync()
    return Step(case, leaves, outs, saved)


def alone(case, cots=None):
    """-> (outputs, gradients) of a forward and its backward with nothing in between"""
    step = forward(case)
    grads = step.backward(None if cots is None else case.cotangents(cots))
    return snapshot(step.outputs()), snapshot(grads)


# ---- the checks ------------------------------------------------------------------------------------------------------------

def check_operands_intact(case):
    """(a) after the forward every input holds its bits (but for `case.allowed`); after the backward so do the inputs, the
    outputs, every saved tensor and every cotangent"""
    found = []
    with case.guard():
        leaves = case.leaves()
        before = snapshot(leaves)
        with saved_tensors() as saved:
            outs = tuple(case.call(leaves))
        case.sync()
    keep = [k for k in leaves if k not in case.allowed]
    found += [f"{case.name}: the forward wrote its {d}" for d in changed({k: before[k] for k in keep}, {k: leaves[k] for k in keep}, "input")]
    step = Step(case, leaves, outs, saved)
    cots = case.cotangents()
    held = dict(input=leaves, output=step.outputs(), saved=list(saved), cotangent=cots)
    before = snapshot(held)
    grads = step.backward(cots)
    for what in held:
        found += [f"{case.name}: the backward wrote its {d}" for d in changed(before[what], held[what], what)]
    if not any(g is not None for g in grads.values()):
        found.append(f"{case.name}: no gradient came back")
    return found


def check_repeatable(case, other_cots):
    """(b) two backwards of one forward with the same cotangents give the same bits; a third with `other_cots` gives the
    bits of a fresh forward + backward with them.  -> (findings, the third backward's gradients)"""
    found = []
    step = forward(case)
    first = snapshot(step.backward(retain=True))
    second = snapshot(step.backward(retain=True))
    found += [f"{case.name}: the second backward differs from the first at {d}" for d in pf.differences(first, second, "grad")]
    third = snapshot(step.backward(case.cotangents(other_cots)))
    _, fresh = alone(case, other_cots)
    found += [f"{case.name}: a backward with another cotangent after two backwards differs from a fresh run at {d}"
              for d in pf.differences(fresh, third, "grad")]
    if pf.same_bits(first, third):
        found.append(f"{case.name}: another cotangent gave the same gradients: the check has no teeth")
    return found, third


def check_accumulates(case):
    """(b) two backwards of one forward accumulated into the leaves' .grad give twice the first, bit for bit (g + g is exact).
    AccumulateGrad keeps a gradient tensor nobody else holds as the leaf's .grad and adds the next one IN PLACE -- and a
    view counts as a tensor nobody else holds: two gradients that are views of one buffer, or of the cotangent, make two
    .grad share memory, and the second backward (or a clipping, a zero_()) of one changes the other.  -> findings"""
    step = forward(case)
    leaves = [step.leaves[k] for k in case.diff]
    with case.guard():
        for _ in range(2):
            cots = case.cotangents()
            torch.autograd.backward([step.outs[i] for i in step.sel()], [cots[i] for i in step.sel()], retain_graph=True,
                                    inputs=leaves)
        case.sync()
    twice = {k: None if g is None else g * 2 for k, g in alone(case)[1].items()}
    got = {k: step.leaves[k].grad for k in case.diff}
    found = [f"{case.name}: two backwards accumulated in .grad are not twice one at {d}" for d in pf.differences(twice, got, "grad")]
    ptrs = {}
    for k, g in got.items():
        if g is not None and g.numel():
            lo = g.data_ptr()
            for other, (a, b) in ptrs.items():
                if lo < b and a < lo + g.numel() * g.element_size():
                    found.append(f"{case.name}: the .grad of {k} and of {other} share memory")
            ptrs[k] = (lo, lo + g.numel() * g.element_size())
    return found


def check_one_output_at_a_time(case):
    """(c) one backward per output with retain_graph=True, accumulated into .grad -> {input: accumulated gradient}"""
    step = forward(case)
    cots = case.cotangents()
    with case.guard():
        for i in step.sel():
            torch.autograd.backward([step.outs[i]], [cots[i]], retain_graph=True, inputs=[step.leaves[k] for k in case.diff])
        case.sync()
    return {k: step.leaves[k].grad for k in case.diff}


def check_interleaved(a, b):
    """(d) forward A, forward B, then the backwards in both orders: outputs and gradients of each hold the bits of its
    run alone.  -> findings"""
    found = []
    want = {x.name: alone(x) for x in (a, b)}
    if pf.same_bits(want[a.name], want[b.name]):
        found.append(f"{a.name}: the two problems give the same bits: the check has no teeth")
    for order in ("BA", "AB"):
        steps = {a.name: forward(a), b.name: forward(b)}
        grads = {}
        for x in ((b, a) if order == "BA" else (a, b)):
            grads[x.name] = steps[x.name].backward()
        for x in (a, b):
            got = (steps[x.name].outputs(), grads[x.name])
            found += [f"{x.name}: forwards A, B then backwards {order}: differs from its run alone at {d}"
                      for d in pf.differences(want[x.name], got, "(outputs, grads)")]
    return found


def check_cotangent_forms(case, forms=FORMS):
    """(e) every form to every output, the other outputs with their contiguous cotangents: the gradients hold the bits of
    the run with the contiguous copy of the same values, none of them has a NaN (the neighbours of the channel slice), the
    cotangent and the tensor it is a view of are unchanged.  -> (findings, how many (output, form) pairs ran)"""
    found, ran = [], 0
    n_out = len(case.cots)
    for i in range(n_out):
        for form in forms:
            step = forward(case)
            if not step.outs[i].requires_grad:
                continue
            made = cotangent_form(form, step.outs[i], case.cots[i])
            if made is None:
                continue
            c, holder, dense = made
            cots = case.cotangents()
            cots[i] = c
            before = snapshot((c, holder))
            got = snapshot(step.backward(cots))
            found += [f"{case.name}: output {i} {form}: the backward wrote the cotangent's {d}"
                      for d in changed(before, (c, holder), "memory")]
            for k, g in got.items():
                if g is not None and g.is_floating_point() and not bool(torch.isfinite(g).all()):
                    found.append(f"{case.name}: output {i} {form}: d{k} is not finite")
            twin = forward(case)
            cots = case.cotangents()
            cots[i] = dense
            want = snapshot(twin.backward(cots))
            found += [f"{case.name}: output {i} {form}: differs from the contiguous run at {d}"
                      for d in pf.differences(want, got, "grad")]
            ran += 1
    return found, ran


# ---- the graph attention with an adjacency that requires grad ---------------------------------------------------------------
ADJACENCY_FORMS = ("nn", "1nn", "bnn", "csr", "coo", "edge", "edge sets")


def gacn_reference(x, alpha, Wg, W, adj, dz=None, target=None, dtype=torch.float64, device="cpu"):
    """Autograd of oracle/dense_torch.py's gacn_dense (graph_attention_dense where W is None) for ONE relation in `dtype`:
    x [B,C,N,T], alpha [1,C], Wg [1,T,T], W [1,O,C] | None, adj [N,N], [1,N,N] or [B,N,N] (CPU tensors or arrays), with the
    cotangent `dz` at z or, `target` given, that of the loss 0.5 |z - target|^2.  -> {z, dx, dalpha, dWg, dW, dadj} on the CPU"""
    from oracle import dense_torch

    def leaf(t):
        return torch.as_tensor(t).detach().to(device, dtype).clone().requires_grad_(True)
    xt, at, Wgt, a = leaf(x), leaf(alpha), leaf(Wg), leaf(adj)
    Wt = None if W is None else leaf(W)
    if Wt is None:
        z = dense_torch.graph_attention_dense(xt, a, Wgt[0], at[0])
    else:
        z = dense_torch.gacn_dense(xt, a, Wgt[0], at[0], Wt[0])
    if target is not None:
        dz = z.detach() - torch.as_tensor(target).to(device, dtype)
    z.backward(torch.as_tensor(dz).to(device, dtype))
    out = dict(z=z.detach(), dx=xt.grad, dalpha=at.grad, dWg=Wgt.grad, dadj=a.grad)
    if Wt is not None:
        out["dW"] = Wt.grad
    return {k: v.cpu() for k, v in out.items()}


def reversed_rows(adj):
    """-> (crow, rows, cols) of the non-zeros of the dense [N,N] array `adj` with the columns of every row DEscending: not
    the library's edge order, so the values cross through SparsePattern's permutation and its one shared value buffer"""
    import numpy as np
    r, c = np.nonzero(adj)
    n = adj.shape[0]
    crow = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    perm = np.concatenate([np.arange(crow[i], crow[i + 1])[::-1] for i in range(n)]).astype(np.int64)
    return crow, r[perm], c[perm]


# ---- the census: which case of test_gpu_autograd_contract.py runs which torch.autograd.Function of ops.py --------------------
# the Functions outside grad_subset_fixtures.ROWS -> the op of ops.py whose case (f) of the GPU file runs them
OTHER_FUNCTIONS = {
    "_EdgeTimeWeightsFunction": "edge_time_weights",
    "_EdgeSignalWeightsFunction": "edge_signal_weights",
    "_EdgeDropoutFunction": "edge_dropout",
    "_EdgeValidityFunction": "edge_validity",
    "_TailMetricsFunction": "huber_metrics gauss_metrics masked_huber_metrics masked_gauss_metrics quantile_metrics",
}

# case (e): the row of grad_subset_fixtures.ROWS whose outputs receive every cotangent form, one per Function (the N = 64
# row where there is one: the in-place slice paths _sliced_grad / _as_segment depend on the shape).  Every row compares bit
# for bit with the contiguous run: no strided form selects another kernel.  Why, per group of Functions:
#   copy first        the backward begins with `.contiguous()` on the cotangent (a copy of the same values for every form
#                     but the contiguous one), then runs what the contiguous run runs
#   stride argument   `_as_segment` hands a channel slice of a contiguous wider tensor to the SAME kernel with its group
#                     stride (time_mix, causal_conv, mix_multi's segments, _channel_sums); any other layout is copied first
#   accepted in place `_sliced_grad`: the library reads the slice in place only where msgat_bwd_accepts_strided_dz /
#                     msgat_attention_bwd_accepts_strided_dv say so, which is where the fused edge pass runs -- chosen by shape
#                     and graph, never by the stride (api.hip) -- and that pass takes the group stride as an argument
#   views             the glue Functions hand out views or torch copies of the cotangent
FORM_ROWS = {
    "_MixFunction": ("mix 72->24 N=64 bias add relu", "copy first"),
    "_MixMultiFunction": ("mix_multi three inputs with adds 72->24 N=64", "stride argument"),
    "_TimeMixFunction": ("time_mix K=2 per group 24 N=64 bias per relation", "stride argument"),
    "_CausalConvFunction": ("causal_conv 72->24 N=64 d=2 bias", "stride argument"),
    "_NodePoolFunction": ("node_pool C=72 N=64 T=12 sets=True", "copy first"),
    "_ChannelPoolFunction": ("channel_pool C=72 N=64 T=12 sets=True", "copy first"),
    "_HeadFunction": ("head C=72 N=64 To=12 per relation bias", "copy first"),
    "_LnHeadFunction": ("ln_head C=72 N=64 To=12 per relation relu input", "copy first"),
    "_LayerNormTFunction": ("layer_norm_t C=72 N=64 per relation relu input", "copy first"),
    "_LnPoolTeeFunction": ("layer_norm_pool_tee fused C=72 N=64 relu_input=True", "copy first"),
    "_GateSumFunction": ("gate_sum time embedding N=64 To=12", "copy first"),
    "_ChannelAttentionMixFunction": ("channel_attention_mix C=72 cb=24", "copy first"),
    "_TemporalAttentionTapsFunction": ("temporal_attention_taps N=64 d=2", "copy first"),
    "_AssembleRowsFunction": ("assemble_rows 9 + 5 rows of 13", "views"),
    "_BiasJoinFunction": ("bias_join 24 + 9", "views"),
    "_Relayout": ("relayout [2,9,5,2] -> (0,3,1,2)", "views"),
    "_AttentionCoreFunction": ("attention_core Cu=24 N=64", "accepted in place"),
    "_GACNFunction": ("gacn PROJ_FIRST 72->24 N=64", "accepted in place"),
}
# further rows of case (e): the second GACN mode (dz feeds channel-mixing passes with a group stride), the weights output
FORM_ROWS_MORE = ("gacn AGG_FIRST 5->9 N=13", "gacn PROJ_FIRST 72->24 N=64 with masked weights",
                  "mix_multi several outputs 72->24 N=64", "mix_multi relu premasked 72->24 N=64 bias")


def function_classes(ops_source):
    """The names of the torch.autograd.Function subclasses a module's source defines, by `ast`"""
    import ast

    def base(b):
        parts = []
        while isinstance(b, ast.Attribute):
            parts.append(b.attr)
            b = b.value
        parts.append(b.id if isinstance(b, ast.Name) else "")
        return ".".join(reversed(parts))
    return [n.name for n in ast.parse(ops_source).body
            if isinstance(n, ast.ClassDef) and any(base(b).endswith("autograd.Function") for b in n.bases)]


def census(ops_source, gpu_source, rows, other=None, form_rows=None):
    """What of ops.py's Functions no case of the GPU file runs.  A Function is run by cases (a)-(d) through its rows of
    `rows` (the GPU file parametrises them over the whole table) or by case (f) through `other`, whose op the GPU file must
    name as `ops.<op>`; a Function with rows also has its row of case (e) in `form_rows`.  -> the gaps, as sentences"""
    import ast
    other = OTHER_FUNCTIONS if other is None else other
    form_rows = FORM_ROWS if form_rows is None else form_rows
    named = {n.attr for n in ast.walk(ast.parse(gpu_source))
             if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "ops"}
    by_rows = {r.function for r in rows}
    row_names = {r.name: r.function for r in rows}
    gaps = []
    for f in function_classes(ops_source):
        if f in by_rows:
            if f not in form_rows:
                gaps.append(f"ops.{f} has no row for the cotangent forms (case e)")
            elif row_names.get(form_rows[f][0]) != f:
                gaps.append(f"ops.{f}: its row for the cotangent forms, {form_rows[f][0]!r}, is not a row of it")
        elif f in other:
            gaps += [f"ops.{f}: the GPU file does not call ops.{op}" for op in other[f].split() if op not in named]
        else:
            gaps.append(f"ops.{f} is an autograd.Function and no case of test_gpu_autograd_contract.py runs it")
    return gaps
