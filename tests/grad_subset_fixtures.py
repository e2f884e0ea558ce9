"""What the gradient-subset tests (test_gpu_grad_subsets.py, test_grad_subsets_cpu.py) share, and the float64 restatements
the older per-op tests (test_gpu_branches.py, test_gpu_layernorm.py, test_gpu_tail.py) state as well: written once, in plain
torch ops, evaluated in whatever dtype their arguments have.

One `Row` per op and form: the library callable, its restatement, seeded CPU inputs, the names of its differentiable
inputs.  `subsets` says which of them require grad in a run; `reference` differentiates the restatement for the same
subset of inputs and the same subset of outputs.  `problem(name, seed=1)` is a second problem of a row -- the same shapes,
call and graph, other values -- for the autograd-contract tests (test_gpu_autograd_contract.py); problem 0 is drawn as ever.

Shapes are the smallest at which the kernel forms differ: R = 2 relations of Bg = 2 groups; widths 72 -> 24 and 5 -> 9 (no
multiple of 4, 8 or 16; the causal convolution has no kernel for 5 -> 9 and runs 9 -> 9); N = 13 (156 positions: the
register-staged contraction) and N = 64 (768 positions: the LDS-DMA forms from 512 up); T = 12 and one T = 8 row per op;
12 outputs, 7 for the heads.  The largest tensor is [4,72,64,12].

ReLU rows: a pre-activation within rounding of zero would let the kernel's fp32 mask and the float64 one differ, so the
cotangent is zero wherever |pre-activation| < MARGIN in float64 (a few entries in a hundred thousand).  A row with
`premasked` runs `relu_grad_premasked=True`, whose contract is a cotangent that is already zero where the output is:
its cotangent is masked that way, and the gradient is then the ReLU's own."""
import dataclasses
import functools
import zlib
from typing import Callable, Optional

import torch
import torch.nn.functional as F

from oracle import dense_torch

import branch_edge_fixtures as fx

R, BG = 2, 2
G = R * BG
EPS = 1e-5
MARGIN = 1e-5
PARITY, REL4, REL5 = ("parity",), ("rel", 1e-4), ("rel", 1e-5)


# ---- restatements ------------------------------------------------------------------------------------------------------

def _rows(p, groups):
    """[R, ...] -> [groups, ...]: each relation's row for its groups (relation-major); a tensor without the axis as it is"""
    return p.repeat_interleave(groups // p.shape[0], dim=0)


def _channel_bias(bias, groups, Co):
    """bias [Co] or [R,Co] -> broadcastable against [groups,Co,N,T]"""
    return bias.view(1, Co, 1, 1) if bias.dim() == 1 else _rows(bias, groups).view(groups, Co, 1, 1)


def mix_dense(x, M, bias=None, add=None, relu=False):
    """relu?(M_r x + bias + add): ops.mix (a 1x1 convolution, a per-sample channel matrix, MEAM's tail msgat.py:130-131)"""
    Gx, Ci, N, T = x.shape
    Rm, Co = M.shape[0], M.shape[1]
    out = torch.einsum("roc,rgcnt->rgont", M, x.reshape(Rm, Gx // Rm, Ci, N, T)).reshape(Gx, Co, N, T)
    if bias is not None:
        out = out + _channel_bias(bias, Gx, Co)
    if add is not None:
        out = out + add
    return torch.relu(out) if relu else out


def mix_multi_dense(ins, M, bias=None, adds=(), relu=False, out_channels=None):
    """split(relu?(M cat(ins) + bias + cat(adds))): ops.mix_multi"""
    out = mix_dense(torch.cat(list(ins), dim=1), M, bias, torch.cat(list(adds), dim=1) if len(adds) else None, relu)
    return tuple(torch.split(out, list(out_channels), dim=1)) if out_channels else (out,)


def time_mix_dense(y, A, bias=None):
    """out[g,o] = bias + sum_k A[g|0,k] y[g,k Co+o] along time: ops.time_mix with shared or per-group matrices"""
    Gy, KC, N, T = y.shape
    K = A.shape[1]
    out = torch.einsum("gkti,gkoni->gont", A.expand(Gy, K, T, T), y.reshape(Gy, K, KC // K, N, T))
    return out if bias is None else out + _channel_bias(bias, Gy, KC // K)


def causal_conv_dense(h, taps, bias, dilation):
    """Conv2d(Ci, Co, [1,2], padding=[0,d], dilation=[1,d]) + Chomp(d) (msgat.py:69-74), relation by relation, from the
    stacked taps [R,2Co,Ci] = [W0; W1] of ops.causal_conv"""
    Gh, T = h.shape[0], h.shape[3]
    Rt, Co = taps.shape[0], taps.shape[1] // 2
    w = torch.stack([taps[:, :Co], taps[:, Co:]], dim=-1).unsqueeze(-2)          # [R,Co,Ci,1,2]: nn.Conv2d's layout
    Bg = Gh // Rt
    out = torch.cat([F.conv2d(h[r * Bg:(r + 1) * Bg], w[r], None, padding=(0, dilation), dilation=(1, dilation))[..., :T]
                     for r in range(Rt)])
    return out if bias is None else out + _channel_bias(bias, Gh, Co)


def node_pool_dense(x, w):
    return fx.node_pool_dense(x, w if w.dim() == 2 else w.unsqueeze(0))


def channel_pool_dense(x, alpha):
    return fx.channel_pool_dense(x, alpha if alpha.dim() == 2 else alpha.unsqueeze(0))


def head_dense(x, W, bias=None):
    """TPC.fc (msgat.py:153,:159-160): Conv2d(T, T_out, [1, C]) on x.transpose(1, 3), squeezed, transposed; W with a
    leading [R] axis: relation by relation"""
    if W.dim() == 4:
        return F.conv2d(x.transpose(1, 3), W, bias)[..., 0].transpose(1, 2)
    Rw, Bg = W.shape[0], x.shape[0] // W.shape[0]
    return torch.cat([head_dense(x[r * Bg:(r + 1) * Bg], W[r], None if bias is None else bias[r]) for r in range(Rw)])


def layer_norm_dense(x, weight=None, bias=None, eps=EPS, relu_input=False):
    """F.layer_norm over T with [T] or [R,T] parameters.  `relu_input`: x is a ReLU output whose backward mask the op
    applies; relu(x) = x bit for bit there, and its backward is that mask."""
    T = x.shape[-1]
    y = F.layer_norm(torch.relu(x) if relu_input else x, [T], None, None, eps)
    shape = (x.shape[0],) + (1,) * (x.dim() - 2) + (T,)
    if weight is not None:
        y = y * (weight if weight.dim() == 1 else _rows(weight, x.shape[0]).view(shape))
    if bias is not None:
        y = y + (bias if bias.dim() == 1 else _rows(bias, x.shape[0]).view(shape))
    return y


def ln_head_dense(x, ln_weight, ln_bias, eps, W, bias=None, relu_input=False):
    """head(layer_norm(x)): a component's last two steps (msgat.py:158-160)"""
    return head_dense(layer_norm_dense(x, ln_weight, ln_bias, eps, relu_input), W, bias)


def layer_norm_pool_tee_dense(x, weight, bias, eps, relu_input, pool_w):
    """(LayerNorm(x), x again, node_pool(LayerNorm(x))): msgat.py:122-125 with attention.py:89; `relu_input` masks the
    gradient of both uses of x"""
    xr = torch.relu(x) if relu_input else x
    y = layer_norm_dense(xr, weight, bias, eps)
    return y, (xr if relu_input else x * 1.0), node_pool_dense(y, pool_w)


def gate_sum_dense(pred, H, D, h_w, d_w=None):
    """sum_r pred_r * gate_r, summed left to right as the reference's generator does (msgat.py:203-205); the gate from the
    embedding tables (embeddings.py:36-39) or the static gate h_w [R,N,To]"""
    Rp, B = pred.shape[:2]
    if H is not None:
        gates = (F.embedding(H, h_w) + F.embedding(D, d_w)).view(B, Rp, *pred.shape[2:]).unbind(1)
    else:
        gates = h_w.view(Rp, *pred.shape[2:]).unbind(0)
    out = None
    for r in range(Rp):
        term = pred[r] * gates[r]
        out = term if out is None else out + term
    return out


def assemble_rows_dense(per_group, per_relation):
    return torch.cat([per_group, _rows(per_relation, per_group.shape[0])], dim=1)


def bias_join_dense(wide, narrow):
    return wide + F.pad(narrow, (0, wide.shape[1] - narrow.shape[1]))


def relayout_dense(t, perm):
    return t.permute(*perm).contiguous()


def attention_core_dense(u, q, Wg, adj):
    """(softmax(q Wg q^T) . adj) u: attention.py:34-36 on projected features, relation by relation"""
    Rw, Bg = Wg.shape[0], u.shape[0] // Wg.shape[0]
    out = []
    for r in range(Rw):
        qr = q[r * Bg:(r + 1) * Bg]
        coeff = torch.softmax(qr @ Wg[r] @ qr.transpose(1, 2), dim=-1) * adj
        out.append(torch.einsum("bnm,bcmt->bcnt", coeff, u[r * Bg:(r + 1) * Bg]))
    return torch.cat(out)


def gacn_dense(x, alpha, Wg, W, adj):
    Rw, Bg = Wg.shape[0], x.shape[0] // Wg.shape[0]
    return torch.cat([dense_torch.gacn_dense(x[r * Bg:(r + 1) * Bg], adj, Wg[r], alpha[r], W[r]) for r in range(Rw)])


# ---- the case table ----------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Row:
    name: str
    function: str                       # the torch.autograd.Function subclass of ops.py the row runs
    make: Callable                      # (seed=0) -> {input name: CPU tensor | None | plain value}, seeded by name and seed
    diff: tuple                         # names of the differentiable inputs
    lib: Callable                       # (ops, inputs) -> tuple of outputs
    dense: Callable                     # (inputs) -> tuple of outputs
    bar: tuple                          # PARITY (conftest.assert_parity), REL4 / REL5 (rel_err < tol): the op's own test's
    own_launch: tuple = ()              # gradients whose launch does not depend on the other needs: equal bits in every run
    fused: bool = False                 # a fused pass and separate passes exist: the distance to the full-set run is recorded
    pre: Optional[Callable] = None      # (inputs) -> tuple of pre-activations (ReLU rows)
    premasked: bool = False
    out_subsets: tuple = ()             # multi-output nodes: the subsets of outputs that carry a cotangent, besides all


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _n(gen, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=gen) * scale + shift


ROWS = []


def seed_name(name, seed=0):
    """What seeds the draws of a row's problem `seed`: the row's name for problem 0 (every value as it always was), the name
    with a suffix for any other -- the same shapes, graph and call, other values"""
    return name if not seed else f"{name} seed {seed}"


def _seeded(make, name, seed=0):
    return make(seed_name(name, seed))


def _add(name, function, make, diff, lib, dense, bar, **kw):
    ROWS.append(Row(name, function, functools.partial(_seeded, make, name), tuple(diff), lib, dense, bar, **kw))


# mix: backward launches dx (ops.py _MixFunction.backward `if need[0]`), dM (`if need[1]`) and dbias (`_channel_sums`) each
# on its own from dpre; dadd is dpre itself
def _mix(name, Ci, Co, N, T, bias, add, relu, Rm=R):
    def make(name):
        g = _gen(name)
        return dict(x=_n(g, G, Ci, N, T), M=_n(g, Rm, Co, Ci, scale=Ci ** -0.5), bias=_n(g, Co) if bias else None,
                    add=_n(g, G, Co, N, T) if add else None)
    diff = ["x", "M"] + (["bias"] if bias else []) + (["add"] if add else [])
    _add(name, "_MixFunction", make, diff,
         lambda ops, t: (ops.mix(t["x"], t["M"], t["bias"], t["add"], relu),),
         lambda t: (mix_dense(t["x"], t["M"], t["bias"], t["add"], relu),), REL4, own_launch=tuple(diff),
         pre=(lambda t: (mix_dense(t["x"], t["M"], t["bias"], t["add"], False),)) if relu else None)


_mix("mix 72->24 N=64 bias add relu", 72, 24, 64, 12, True, True, True)
_mix("mix 5->9 N=13", 5, 9, 13, 12, False, False, False)
_mix("mix 5->9 N=13 T=8 bias", 5, 9, 13, 8, True, False, False)
_mix("mix 72->24 N=13 per-group matrix bias", 72, 24, 13, 12, True, False, False, Rm=G)


# mix_multi: one input with its gradient and the matrix's both wanted is ONE pass (msgat_contract_mix_segments), any other
# subset the separate launches; the gradients of the add operands are views of cat(dpre)
def _mix_multi(name, cin, Co, N, T, bias, cadd=(), relu=False, premasked=False, out_channels=None, out_subsets=()):
    Ci = sum(cin)

    def make(name):
        g = _gen(name)
        t = dict(M=_n(g, R, Co, Ci, scale=Ci ** -0.5),
                 bias=None if bias is None else _n(g, *((Co,) if bias == "shared" else (R, Co))))
        t.update({f"in{i}": _n(g, G, c, N, T) for i, c in enumerate(cin)})
        t.update({f"add{i}": _n(g, G, c, N, T) for i, c in enumerate(cadd)})
        return t
    ins, adds = [f"in{i}" for i in range(len(cin))], [f"add{i}" for i in range(len(cadd))]
    diff = ["M"] + (["bias"] if bias else []) + ins + adds

    def dense(t, relu=relu):
        return mix_multi_dense([t[k] for k in ins], t["M"], t["bias"], [t[k] for k in adds], relu, out_channels)
    _add(name, "_MixMultiFunction", make, diff,
         lambda ops, t: ops.mix_multi([t[k] for k in ins], t["M"], t["bias"], adds=[t[k] for k in adds], relu=relu,
                                      out_channels=out_channels, relu_grad_premasked=premasked),
         dense, REL4, own_launch=tuple(adds), fused=True, pre=(lambda t: dense(t, False)) if relu else None,
         premasked=premasked, out_subsets=out_subsets)


_mix_multi("mix_multi one input 72->24 N=64 bias", (72,), 24, 64, 12, "shared")
_mix_multi("mix_multi one input 5->9 N=13", (5,), 9, 13, 12, None)
_mix_multi("mix_multi one input 3->9 N=13 T=8 bias per relation", (3,), 9, 13, 8, "relation")
_mix_multi("mix_multi one input 3->24 N=64 bias", (3,), 24, 64, 12, "shared")
_mix_multi("mix_multi three inputs with adds 72->24 N=64", (24, 43, 5), 24, 64, 12, "relation", cadd=(9, 15))
_mix_multi("mix_multi three inputs with adds 5->9 N=13", (2, 2, 1), 9, 13, 12, "shared", cadd=(4, 5))
_mix_multi("mix_multi several outputs 72->24 N=64", (72,), 24, 64, 12, None, out_channels=(8, 12, 4),
           out_subsets=((0,), (1,), (2,), (1, 2), (0, 2), (0, 1)))
_mix_multi("mix_multi several outputs 5->9 N=13 bias", (5,), 9, 13, 12, "shared", out_channels=(1, 8),
           out_subsets=((0,), (1,)))
_mix_multi("mix_multi relu 72->24 N=64 bias", (72,), 24, 64, 12, "shared", cadd=(24,), relu=True)
_mix_multi("mix_multi relu premasked 72->24 N=64 bias", (72,), 24, 64, 12, "shared", cadd=(24,), relu=True, premasked=True)
_mix_multi("mix_multi relu premasked 5->9 N=13", (5,), 9, 13, 12, None, relu=True, premasked=True)


# time_mix: dy (`if need[0]`: msgat_time_mix backward), dA (`if need[1]`: msgat_time_mix_grad_matrix) and dbias
# (`_channel_sums`) are launches of their own in _TimeMixFunction.backward
def _time_mix(name, K, Co, N, T, per_group, bias):
    def make(name):
        g = _gen(name)
        return dict(y=_n(g, G, K * Co, N, T), A=_n(g, G if per_group else 1, K, T, T, scale=T ** -0.5),
                    bias=None if bias is None else _n(g, *((Co,) if bias == "shared" else (R, Co))))
    diff = ["y", "A"] + (["bias"] if bias else [])
    _add(name, "_TimeMixFunction", make, diff, lambda ops, t: (ops.time_mix(t["y"], t["A"], t["bias"]),),
         lambda t: (time_mix_dense(t["y"], t["A"], t["bias"]),), PARITY, own_launch=tuple(diff))


_time_mix("time_mix K=2 per group 24 N=64 bias per relation", 2, 24, 64, 12, True, "relation")
_time_mix("time_mix K=1 shared 9 N=13", 1, 9, 13, 12, False, None)
_time_mix("time_mix K=2 shared 9 N=13 T=8 bias", 2, 9, 13, 8, False, "shared")
_time_mix("time_mix K=1 per group 9 N=13 bias", 1, 9, 13, 12, True, "shared")


# causal_conv: dh is its own launch (`if need[0]`); dtaps and dbias share one contraction, whose form (`with_ones`) and
# reduction depend on whether the bias gradient is wanted
def _causal_conv(name, Ci, Co, N, T, d, bias):
    def make(name):
        g = _gen(name)
        return dict(h=_n(g, G, Ci, N, T), taps=_n(g, R, 2 * Co, Ci, scale=(2 * Ci) ** -0.5),
                    bias=None if bias is None else _n(g, *((Co,) if bias == "shared" else (R, Co)), scale=0.3))
    diff = ["h", "taps"] + (["bias"] if bias else [])
    _add(name, "_CausalConvFunction", make, diff, lambda ops, t: (ops.causal_conv(t["h"], t["taps"], t["bias"], d),),
         lambda t: (causal_conv_dense(t["h"], t["taps"], t["bias"], d),), REL5, own_launch=("h",), fused=True)


_causal_conv("causal_conv 72->24 N=64 d=2 bias", 72, 24, 64, 12, 2, "shared")
_causal_conv("causal_conv 72->24 N=64 d=4 bias per relation", 72, 24, 64, 12, 4, "relation")
_causal_conv("causal_conv 72->24 N=64 d=1 no bias", 72, 24, 64, 12, 1, None)
_causal_conv("causal_conv 9->9 N=13 d=2 bias per relation", 9, 9, 13, 12, 2, "relation")
_causal_conv("causal_conv 9->9 N=13 T=8 d=3 no bias", 9, 9, 13, 8, 3, None)
_causal_conv("causal_conv 9->9 N=13 T=8 d=1 bias", 9, 9, 13, 8, 1, "shared")


# node_pool / channel_pool: `if ctx.needs_input_grad[0]` and `[1]` guard one launch each
def _pool(name, function, call, dense, C, N, T, sets, axis):
    def make(name):
        g = _gen(name)
        n = N if axis == "nodes" else C
        return dict(x=_n(g, G, C, N, T), w=_n(g, *((R, n) if sets else (n,)), scale=n ** -0.5))
    _add(name, function, make, ("x", "w"), lambda ops, t: (getattr(ops, call)(t["x"], t["w"]),),
         lambda t: (dense(t["x"], t["w"]),), PARITY, own_launch=("x", "w"))


for _C, _N, _T, _sets in ((72, 64, 12, True), (5, 13, 12, False), (5, 13, 8, True)):
    _pool(f"node_pool C={_C} N={_N} T={_T} sets={_sets}", "_NodePoolFunction", "node_pool", node_pool_dense, _C, _N, _T, _sets,
          "nodes")
    _pool(f"channel_pool C={_C} N={_N} T={_T} sets={_sets}", "_ChannelPoolFunction", "channel_pool", channel_pool_dense, _C, _N,
          _T, _sets, "channels")


# head: dx, dW and dbias are a launch each in _HeadFunction.backward
def _head_inputs(g, C, N, T, To, sets, bias):
    lead = (R,) if sets else ()
    return dict(x=_n(g, G, C, N, T), W=_n(g, *lead, To, T, 1, C, scale=(T * C) ** -0.5),
                bias=_n(g, *lead, To, scale=0.1) if bias else None)


def _head(name, C, N, T, To, sets, bias):
    diff = ["x", "W"] + (["bias"] if bias else [])
    _add(name, "_HeadFunction", lambda name: _head_inputs(_gen(name), C, N, T, To, sets, bias), diff,
         lambda ops, t: (ops.head(t["x"], t["W"], t["bias"]),), lambda t: (head_dense(t["x"], t["W"], t["bias"]),), REL4,
         own_launch=tuple(diff))


_head("head C=72 N=64 To=12 per relation bias", 72, 64, 12, 12, True, True)
_head("head C=5 N=13 To=7 bias", 5, 13, 12, 7, False, True)
_head("head C=5 N=13 T=8 To=7 no bias", 5, 13, 8, 7, False, False)


# ln_head: dx, dln_weight and dln_bias leave the fused pass (msgat_layernorm_head_backward, skipped when none of the three
# is wanted); dW (from the LayerNorm output the FORWARD kept only because W requires grad) and dbias are launches of
# their own
def _ln_head(name, C, N, T, To, sets, lnw=True, lnb=True, bias=True, relu=False):
    def make(name):
        g = _gen(name)
        t = _head_inputs(g, C, N, T, To, sets, bias)
        if relu:
            t["x"] = torch.relu(t["x"] + 0.3)
        shape = (R, T) if sets else (T,)
        t.update(lnw=_n(g, *shape, scale=0.3, shift=1.0) if lnw else None, lnb=_n(g, *shape, scale=0.2) if lnb else None)
        return t
    diff = ["x"] + (["lnw"] if lnw else []) + (["lnb"] if lnb else []) + ["W"] + (["bias"] if bias else [])
    _add(name, "_LnHeadFunction", make, diff,
         lambda ops, t: (ops.ln_head(t["x"], t["lnw"], t["lnb"], EPS, t["W"], t["bias"], relu_input=relu),),
         lambda t: (ln_head_dense(t["x"], t["lnw"], t["lnb"], EPS, t["W"], t["bias"], relu),), REL4,
         own_launch=("W",) + (("bias",) if bias else ()), fused=True)


_ln_head("ln_head C=72 N=64 To=12 per relation relu input", 72, 64, 12, 12, True, relu=True)
_ln_head("ln_head C=5 N=13 To=7", 5, 13, 12, 7, False)
_ln_head("ln_head C=5 N=13 To=7 no LayerNorm weight", 5, 13, 12, 7, False, lnw=False)
_ln_head("ln_head C=5 N=13 To=7 no LayerNorm bias no head bias", 5, 13, 12, 7, False, lnb=False, bias=False)
_ln_head("ln_head C=5 N=13 To=7 per relation no LayerNorm weight", 5, 13, 12, 7, True, lnw=False)
_ln_head("ln_head C=5 N=13 To=7 plain normalisation", 5, 13, 12, 7, False, lnw=False, lnb=False)
_ln_head("ln_head C=5 N=13 T=8 To=7 per relation", 5, 13, 8, 7, True)


# layer_norm_t: one backward launch gives dx and the partials of both parameter gradients whatever is wanted
def _layer_norm(name, C, N, T, sets, w=True, b=True, relu=False):
    def make(name):
        g = _gen(name)
        x = _n(g, G, C, N, T, scale=3.0, shift=1.5)
        shape = (R, T) if sets else (T,)
        return dict(x=torch.relu(x) if relu else x, w=_n(g, *shape, scale=0.3, shift=1.0) if w else None,
                    b=_n(g, *shape, scale=0.2) if b else None)
    diff = ["x"] + (["w"] if w else []) + (["b"] if b else [])
    _add(name, "_LayerNormTFunction", make, diff, lambda ops, t: (ops.layer_norm_t(t["x"], t["w"], t["b"], EPS, relu),),
         lambda t: (layer_norm_dense(t["x"], t["w"], t["b"], EPS, relu),), REL4, own_launch=tuple(diff))


_layer_norm("layer_norm_t C=72 N=64 per relation relu input", 72, 64, 12, True, relu=True)
_layer_norm("layer_norm_t C=5 N=13", 5, 13, 12, False)
_layer_norm("layer_norm_t C=5 N=13 no weight per relation bias", 5, 13, 12, True, w=False)
_layer_norm("layer_norm_t C=5 N=13 no bias", 5, 13, 12, False, b=False)
_layer_norm("layer_norm_t C=5 N=13 T=8 no parameters", 5, 13, 8, False, w=False, b=False)


# layer_norm_pool_tee: a frozen x takes the two separate ops unless the node's forward is the fused one (same parameter-set
# counts, N >= 64), where in grad mode everything goes through the node; the node's backward is one launch when the pooling has the LayerNorm's parameter-set count (null
# dpool_w / dpool_rows when pool_w is frozen), else the pooling's own passes first
TEE_OUTPUT_SUBSETS = ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2))


def _tee(name, C, N, T, ln_sets, pool_sets, relu, w=True, b=True):
    def make(name):
        g = _gen(name)
        x = _n(g, G, C, N, T)
        return dict(x=torch.relu(x + 0.3) if relu else x,
                    w=_n(g, *((R, T) if ln_sets else (T,)), scale=0.3, shift=1.0) if w else None,
                    b=_n(g, *((R, T) if ln_sets else (T,)), scale=0.2) if b else None,
                    pool_w=_n(g, *((R, N) if pool_sets else (N,))))
    diff = ["x"] + (["w"] if w else []) + (["b"] if b else []) + ["pool_w"]
    _add(name, "_LnPoolTeeFunction", make, diff,
         lambda ops, t: ops.layer_norm_pool_tee(t["x"], t["w"], t["b"], EPS, relu, t["pool_w"]),
         lambda t: layer_norm_pool_tee_dense(t["x"], t["w"], t["b"], EPS, relu, t["pool_w"]), REL4, fused=True,
         out_subsets=TEE_OUTPUT_SUBSETS)


for _relu in (False, True):
    _tee(f"layer_norm_pool_tee fused C=72 N=64 relu_input={_relu}", 72, 64, 12, True, True, _relu)
    _tee(f"layer_norm_pool_tee small C=5 N=13 relu_input={_relu}", 5, 13, 12, True, True, _relu)
    _tee(f"layer_norm_pool_tee one LayerNorm two poolings C=5 N=64 relu_input={_relu}", 5, 64, 12, False, True, _relu)
_tee("layer_norm_pool_tee two LayerNorms one pooling C=5 N=13 T=8", 5, 13, 8, True, False, False)
_tee("layer_norm_pool_tee fused C=5 N=64 no LayerNorm weight", 5, 64, 12, True, True, True, w=False)
_tee("layer_norm_pool_tee fused C=5 N=64 no LayerNorm parameters", 5, 64, 12, False, False, False, w=False, b=False)


# gate_sum: one backward launch; dpred, dh_w and dd_w are each written by threads of their own and left out when null
def _gate_sum(name, N, To, te, B=3):
    def make(name):
        g = _gen(name)
        t = dict(pred=_n(g, R, B, N, To), H=None, D=None, d_w=None)
        if te:
            t.update(h_w=_n(g, 24, R * N * To), d_w=_n(g, 7, R * N * To), H=torch.randint(0, 24, (B,), generator=g),
                     D=torch.randint(0, 7, (B,), generator=g))
        else:
            t.update(h_w=_n(g, R, N, To))
        return t
    diff = ["pred", "h_w"] + (["d_w"] if te else [])
    _add(name, "_GateSumFunction", make, diff, lambda ops, t: (ops.gate_sum(t["pred"], t["H"], t["D"], t["h_w"], t["d_w"]),),
         lambda t: (gate_sum_dense(t["pred"], t["H"], t["D"], t["h_w"], t["d_w"]),), REL5, own_launch=tuple(diff))


_gate_sum("gate_sum time embedding N=64 To=12", 64, 12, True)
_gate_sum("gate_sum time embedding N=13 To=7", 13, 7, True)
_gate_sum("gate_sum static gate N=13 To=12", 13, 12, False)


# the two small attentions: one backward launch gives every gradient whatever is wanted
def _channel_attention(name, C, cb, T):
    def make(name):
        g = _gen(name)
        return dict(p=_n(g, G, C, T, scale=0.7), Wc=_n(g, R, T, T, scale=0.4), conv=_n(g, R, cb, C, scale=0.5))
    _add(name, "_ChannelAttentionMixFunction", make, ("p", "Wc", "conv"),
         lambda ops, t: (ops.channel_attention_mix(t["p"], t["Wc"], t["conv"]),),
         lambda t: (fx.channel_attention_mix_dense(t["p"], t["Wc"], t["conv"]),), REL4, own_launch=("p", "Wc", "conv"))


_channel_attention("channel_attention_mix C=72 cb=24", 72, 24, 12)
_channel_attention("channel_attention_mix C=5 cb=9", 5, 9, 12)
_channel_attention("channel_attention_mix C=5 cb=9 T=8", 5, 9, 8)


def _temporal_attention(name, N, T, dil, K=10):
    def make(name):
        g = _gen(name)
        return dict(q=_n(g, G, N, T, scale=0.5), W1=_n(g, R, K, N, scale=N ** -0.5), W2=_n(g, R, K, N, scale=N ** -0.5))
    _add(name, "_TemporalAttentionTapsFunction", make, ("q", "W1", "W2"),
         lambda ops, t: (ops.temporal_attention_taps(t["q"], t["W1"], t["W2"], dil),),
         lambda t: (fx.temporal_attention_taps_dense(t["q"], t["W1"], t["W2"], dil),), REL4, own_launch=("q", "W1", "W2"))


_temporal_attention("temporal_attention_taps N=64 d=2", 64, 12, 2)
_temporal_attention("temporal_attention_taps N=13 d=1", 13, 12, 1)
_temporal_attention("temporal_attention_taps N=13 T=8 d=4", 13, 8, 4)


# host-side glue: torch ops in forward and backward, no library launch
def _glue(name, function, shapes, lib, dense, diff):
    def make(name):
        g = _gen(name)
        return {k: _n(g, *s) for k, s in shapes.items()}
    _add(name, function, make, diff, lib, dense, REL4, own_launch=tuple(diff))


_glue("assemble_rows 9 + 5 rows of 13", "_AssembleRowsFunction", dict(a=(G, 9, 13), b=(R, 5, 13)),
      lambda ops, t: (ops.assemble_rows(t["a"], t["b"]),), lambda t: (assemble_rows_dense(t["a"], t["b"]),), ("a", "b"))
_glue("bias_join 24 + 9", "_BiasJoinFunction", dict(a=(R, 24), b=(R, 9)),
      lambda ops, t: (ops.bias_join(t["a"], t["b"]),), lambda t: (bias_join_dense(t["a"], t["b"]),), ("a", "b"))
_glue("relayout [2,9,5,2] -> (0,3,1,2)", "_Relayout", dict(a=(R, 9, 5, 2)),
      lambda ops, t: (ops.relayout(t["a"], (0, 3, 1, 2)),), lambda t: (relayout_dense(t["a"], (0, 3, 1, 2)),), ("a",))


# the graph attention: both backward entry points compute every gradient regardless of the needs (ops.py
# _GACNFunction.backward, _AttentionCoreFunction.backward), which these rows pin: equal bits in every run
def _adjacency(N):
    import ms_gat_amd
    return ms_gat_amd.synthetic_adjacency(N, N + 7, seed=5)


def _attention_core(name, Cu, N, T):
    def make(name):
        g = _gen(name)
        return dict(u=_n(g, G, Cu, N, T), q=_n(g, G, N, T), Wg=_n(g, R, T, T, scale=0.3), adj=_adjacency(N))
    _add(name, "_AttentionCoreFunction", make, ("u", "q", "Wg"),
         lambda ops, t: (ops.attention_core(t["u"], t["q"], t["Wg"], t["adj"]),),
         lambda t: (attention_core_dense(t["u"], t["q"], t["Wg"], t["adj"]),), REL4, own_launch=("u", "q", "Wg"))


_attention_core("attention_core Cu=24 N=64", 24, 64, 12)
_attention_core("attention_core Cu=9 N=13 T=8", 9, 13, 8)


GACN_MODES = {"gacn AGG_FIRST 5->9 N=13": 1, "gacn PROJ_FIRST 72->24 N=64": 2, "gacn AGG_FIRST 5->9 N=13 T=8": 1}


def _gacn(name, C, Co, N, T):
    def make(name):
        g = _gen(name)
        return dict(x=_n(g, G, C, N, T), alpha=_n(g, R, C, scale=C ** -0.5), Wg=_n(g, R, T, T, scale=0.3),
                    W=_n(g, R, Co, C, scale=C ** -0.5), adj=_adjacency(N))
    diff = ("x", "alpha", "Wg", "W")
    _add(name, "_GACNFunction", make, diff, lambda ops, t: (ops.gacn(t["x"], t["alpha"], t["Wg"], t["W"], t["adj"]),),
         lambda t: (gacn_dense(t["x"], t["alpha"], t["Wg"], t["W"], t["adj"]),), REL4, own_launch=diff)


_gacn("gacn AGG_FIRST 5->9 N=13", 5, 9, 13, 12)
_gacn("gacn PROJ_FIRST 72->24 N=64", 72, 24, 64, 12)
_gacn("gacn AGG_FIRST 5->9 N=13 T=8", 5, 9, 13, 8)


# need_weights: test_gpu_attention_weights.py runs every combination of the two outputs with every input a leaf; what is
# left is the masked weights beside the output with part of the inputs frozen.  No output sweep is intended for these rows
# (`out_subsets` stays empty): both outputs carry a cotangent in every run
def masked_weights_dense(q, Wg, adj):
    """att * adjacency [G,N,N] (attention.py:34,:36), relation by relation"""
    Rw, Bg = Wg.shape[0], q.shape[0] // Wg.shape[0]
    return torch.cat([torch.softmax(q[r * Bg:(r + 1) * Bg] @ Wg[r] @ q[r * Bg:(r + 1) * Bg].transpose(1, 2), dim=-1) * adj
                      for r in range(Rw)])


def _with_weights(pair):
    z, w = pair
    return z, w.to_dense()


def _gacn_weights(name, C, Co, N, T):
    def make(name):
        g = _gen(name)
        return dict(x=_n(g, G, C, N, T), alpha=_n(g, R, C, scale=C ** -0.5), Wg=_n(g, R, T, T, scale=0.3),
                    W=_n(g, R, Co, C, scale=C ** -0.5), adj=_adjacency(N))
    diff = ("x", "alpha", "Wg", "W")
    _add(name, "_GACNFunction", make, diff,
         lambda ops, t: _with_weights(ops.gacn(t["x"], t["alpha"], t["Wg"], t["W"], t["adj"], need_weights=True)),
         lambda t: (gacn_dense(t["x"], t["alpha"], t["Wg"], t["W"], t["adj"]),
                    masked_weights_dense(torch.einsum("gcnt,gc->gnt", t["x"], _rows(t["alpha"], G)), t["Wg"], t["adj"])),
         REL4, own_launch=diff)


def _attention_core_weights(name, Cu, N, T):
    def make(name):
        g = _gen(name)
        return dict(u=_n(g, G, Cu, N, T), q=_n(g, G, N, T), Wg=_n(g, R, T, T, scale=0.3), adj=_adjacency(N))
    _add(name, "_AttentionCoreFunction", make, ("u", "q", "Wg"),
         lambda ops, t: _with_weights(ops.attention_core(t["u"], t["q"], t["Wg"], t["adj"], need_weights=True)),
         lambda t: (attention_core_dense(t["u"], t["q"], t["Wg"], t["adj"]), masked_weights_dense(t["q"], t["Wg"], t["adj"])),
         REL4, own_launch=("u", "q", "Wg"))


_gacn_weights("gacn PROJ_FIRST 72->24 N=64 with masked weights", 72, 24, 64, 12)
_gacn_weights("gacn AGG_FIRST 5->9 N=13 with masked weights", 5, 9, 13, 12)
_attention_core_weights("attention_core Cu=9 N=13 with masked weights", 9, 13, 12)

ROW_IDS = [r.name.replace(" ", "_") for r in ROWS]

# every other torch.autograd.Function subclass of ops.py, and where its frozen-input cases are
EXCLUDED = {
    "_EdgeTimeWeightsFunction": "test_gpu_edge_time.py has its frozen-input case",
    "_EdgeSignalWeightsFunction": "test_gpu_edge_signal.py has its frozen-input case",
    "_EdgeDropoutFunction": "one differentiable input (the weights): no subset besides the full set",
    "_EdgeValidityFunction": "one differentiable input (the weights): no subset besides the full set",
    "_TailMetricsFunction": "one differentiable input (the prediction): no subset besides the full set",
}


# ---- subsets and their float64 (or fp32) reference ----------------------------------------------------------------------

def subsets(names):
    """Every single input, every leave-one-out, the full set: at most 2k + 1 tuples, each once, in the order of `names`"""
    names = tuple(names)
    seen = []
    for s in [(n,) for n in names] + [tuple(m for m in names if m != n) for n in names] + [names]:
        if s and s not in seen:
            seen.append(s)
    return seen


def output_subsets(row):
    """The subsets of output indices that carry a cotangent: all of them first, then the row's own"""
    return (None,) + tuple(row.out_subsets)


def _cast(v, dtype):
    return v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v


@functools.lru_cache(maxsize=None)
def problem(name, seed=0, cot_seed=None):
    """-> (row, inputs on the CPU in fp32, cotangents in fp32): seeded by the row's name (and `seed`, for a second problem
    of the same shapes); the cotangent of a ReLU row is zero within MARGIN of the kink and, for a premasked row, wherever
    the output is zero.  `cot_seed` (default: `seed`): the cotangent drawn as problem `cot_seed` draws it, masked for the
    inputs of problem `seed` -- another cotangent for the same forward"""
    row = ROWS[[r.name for r in ROWS].index(name)]
    inputs = row.make(seed)
    with torch.no_grad():
        t64 = {k: _cast(v, torch.float64) for k, v in inputs.items()}
        outs = row.dense(t64)
        pres = row.pre(t64) if row.pre else None
    g = _gen(seed_name(name, seed if cot_seed is None else cot_seed) + " cotangent")
    cots = []
    for i, o in enumerate(outs):
        c = torch.randn(o.shape, generator=g)
        if pres is not None:
            c = c * (pres[i].abs() > MARGIN)
            if row.premasked:
                c = c * (pres[i] > 0)
        cots.append(c)
    return row, inputs, tuple(cots)


def leaves(inputs, subset, dtype=None, device=None):
    """The row's inputs with exactly `subset` requiring grad"""
    out = {}
    for k, v in inputs.items():
        if torch.is_tensor(v):
            v = _cast(v, dtype) if dtype is not None else v
            v = v.to(device) if device is not None else v.clone()
            if k in subset:
                v.requires_grad_(True)
        out[k] = v
    return out


def differentiable(outs, outsel=None):
    """The indices among `outsel` (None: all) of the outputs that depend on an input that requires grad: the tee's second
    output is x itself and carries no cotangent where x is frozen"""
    return [i for i in (range(len(outs)) if outsel is None else outsel) if outs[i].requires_grad]


@functools.lru_cache(maxsize=None)
def reference(name, subset, outsel=None, dtype=torch.float64, seed=0, cot_seed=None):
    """-> (outputs, {input name: gradient | None}) of the restatement by autograd on the CPU in `dtype`, exactly `subset`
    requiring grad, a cotangent at the outputs `outsel` (None: all); `seed`, `cot_seed`: which problem (see `problem`)"""
    row, inputs, cots = problem(name, seed, cot_seed)
    t = leaves(inputs, subset, dtype)
    outs = row.dense(t)
    sel = differentiable(outs, outsel)
    grads = torch.autograd.grad([outs[i] for i in sel], [t[k] for k in subset], [cots[i].to(dtype) for i in sel],
                                allow_unused=True)
    return tuple(o.detach() for o in outs), dict(zip(subset, grads))


# ---- the whole model with part of it frozen ----------------------------------------------------------------------------
MODEL_CASES = (("msgat72", 3), ("msgat48", 1))          # (factory, input channels); N = 23, B = 3, R = 2, T = 12 as in
MODEL_N, MODEL_B, MODEL_R, MODEL_T = 23, 3, 2, 12      # test_whole_model_matches_the_dense_op_sequence
SCENARIOS = ("input attribution", "head only", "biases frozen", "time embedding frozen")


def model_problem(factory, cin, seed=0):
    """-> (model on the CPU, X, H, D, dout), drawn as test_whole_model_matches_the_dense_op_sequence draws them; `seed`: a
    second model and batch of the same shapes on the same graph"""
    import ms_gat_amd
    from ms_gat_amd import model
    torch.manual_seed(7 + seed)
    gen = torch.Generator().manual_seed(11 + seed)
    N, B, Rm, T = MODEL_N, MODEL_B, MODEL_R, MODEL_T
    net = getattr(model, factory)(n_components=Rm, in_channels=cin, in_timesteps=T, out_timesteps=T, use_te=True,
                                  adj=ms_gat_amd.synthetic_adjacency(N, N + 7, seed=5))
    X = torch.randn(B, Rm, cin, N, T, generator=gen)
    H = torch.randint(0, 24, (B,), generator=gen)
    D = torch.randint(0, 7, (B,), generator=gen)
    return net, X, H, D, torch.randn(B, N, T, generator=gen)


def head_parameter(name):
    """fc.* and the last ln.* of a component (not the LayerNorm of a block, tpcs.r.tgacns.l.ln.*)"""
    parts = name.split(".")
    return len(parts) == 4 and parts[0] == "tpcs" and parts[2] in ("fc", "ln")


def freeze(net, scenario):
    """Freezes what the scenario freezes; -> whether the input X requires grad in it"""
    trainable = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    if scenario == "input attribution":            # eval(), every parameter frozen, the gradient at the input wanted
        net.eval()
        for _, p in trainable:
            p.requires_grad_(False)
        return True
    keep = {"head only": head_parameter, "biases frozen": lambda n: not n.endswith(".bias"),
            "time embedding frozen": lambda n: not n.startswith("te.")}[scenario]
    for n, p in trainable:
        p.requires_grad_(keep(n))
    return False


def model_reference(net, X, H, D, dout, dtype, x_grad):
    """-> (prediction, {trainable parameter name: gradient}, gradient at X or None) of branch_edge_fixtures.msgat_dense with
    the parameters of `net`, in `dtype` on X's device; frozen parameters are no leaves"""
    P = {k: v.detach().to(X.device, dtype) for k, v in net.state_dict().items()}
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    params = {k: v.clone().requires_grad_(k in names) for k, v in P.items() if k != "adj"}
    Xl = X.to(dtype).clone().requires_grad_(x_grad)
    out = fx.msgat_dense(params, P["adj"], [m.dilations for m in net.tpcs[0].tgacns], Xl, H, D)
    grads = torch.autograd.grad(out, [params[n] for n in names] + ([Xl] if x_grad else []), dout.to(dtype), allow_unused=True)
    return out.detach(), {n: g for n, g in zip(names, grads) if g is not None}, (grads[-1] if x_grad else None)
