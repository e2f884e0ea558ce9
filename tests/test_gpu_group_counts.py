"""GPU: the kernels that re-create the softmax map P = 2^(S log2 e - lse) from what the forward saved, at training
group counts, through the C ABI: msgat_adjacency_grad, msgat_edge_weight_grad{,_sets}, msgat_edge_softmax_grad,
msgat_attention_map and msgat_softmax_map_grad on torch buffers, against float64 restatements that use the fp32 lse
values that are passed in (tests/group_fixtures.py).  The module-level suites run B = 2, R <= 3: at most 8 groups, one
group per split.  Here the groups of a block cross group boundaries inside its staging pipeline, last splits are
ragged, sets interleave, the reductions take more than 16 partials, and more than four groups share a value set.

Outputs and workspace start as NaN (targets that are added to: as known values), every call runs twice and the two
results must agree bit for bit.  Each case asserts from the workspace size the split it is meant to take."""
import ctypes as C_
import functools

import pytest
import torch

from conftest import assert_parity, record_err, rel_err
import group_fixtures as F

import ms_gat_amd
from ms_gat_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WHAT = "group_counts"
T12 = 12


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _same_bits(outs, what):
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()), f"{what}: an element was never written"
    assert torch.equal(outs[0], outs[1]), f"{what}: two runs differ"
    return outs[0]


@functools.lru_cache(maxsize=None)
def _graph(N, E):
    """(structure, device struct, rows, cols of its CSR edges on the device)"""
    graph = ms_gat_amd.SparseGraph(ms_gat_amd.synthetic_adjacency(N, E, 3))
    assert graph.nnz == F.nnz_of(N, E)
    gs, keep = graph.on(DEV)
    return graph, gs, keep["erow"][:graph.nnz].long(), keep["col"][:graph.nnz].long()


# ---- msgat_adjacency_grad ------------------------------------------------------------------------------------------

def _adjacency_grad(N, V, G, Cu, T, nsplit, seed, wide=0):
    """-> (dadj of the kernel, float64 dadj).  wide > Cu: dv is the channel slice [2 : 2 + Cu] of a [G,wide,N,T] tensor."""
    L = _lib.lib()
    Bg = V if V > 1 else 1
    shape = _lib.Shape(G // Bg, Bg, Cu, Cu, N, T)
    nbytes = int(L.msgat_adjacency_grad_workspace_bytes(C_.byref(shape), Cu, V))
    assert nbytes == (4 * V * nsplit * N * N if nsplit > 1 else 0), "the case left its branch"
    q, kW, lse, dv, feat = F.draw(G, Cu, N, T, seed, DEV)
    dv_arg, dv_ptr = dv, dv.data_ptr()
    if wide:
        dv_arg = torch.randn(G, wide, N, T, device=DEV)
        dv_arg[:, 2:2 + Cu] = dv
        dv_ptr = dv_arg.data_ptr() + 4 * 2 * N * T
    outs = []
    for _ in range(2):
        dadj, ws = _nan(V, N, N), _nan(max(nbytes // 4, 1))
        _lib.check(L.msgat_adjacency_grad(C_.byref(shape), Cu, dv_ptr, wide, feat.data_ptr(), q.data_ptr(), kW.data_ptr(),
                                          lse.data_ptr(), V, dadj.data_ptr(), ws.data_ptr() if nbytes else None, nbytes,
                                          _stream()), "msgat_adjacency_grad")
        outs.append(dadj)
    return _same_bits(outs, "dadj"), F.dense_adjacency_grad(q, kW, lse, dv, feat, V)


_AG_CASES = [c + (T,) for c in F.ADJACENCY_GRAD_CASES for T in ((4, 8, 16) if c[0] == 70 else (T12,))]


@pytest.mark.parametrize("N,V,G,Cu,nsplit,per,why,T", _AG_CASES, ids=[f"N{c[0]}-V{c[1]}-G{c[2]}-T{c[7]}" for c in _AG_CASES])
def test_adjacency_grad_at_group_counts(N, V, G, Cu, nsplit, per, why, T):
    got, want = _adjacency_grad(N, V, G, Cu, T, nsplit, seed=N + G + T)
    assert_parity(got, want, WHAT, f"adjacency_grad N{N} V{V} G{G} Cu{Cu} T{T} nsplit{nsplit} per{per}:dadj")


def test_adjacency_grad_reads_a_channel_slice_across_group_boundaries():
    """dv_group_channels > 0 with two groups per block: the stride from one group's slice to the next is the wider tensor's"""
    N, V, G, Cu, nsplit, per = F.ADJACENCY_GRAD_CASES[2][:6]
    got, want = _adjacency_grad(N, V, G, Cu, T12, nsplit, seed=7, wide=9)
    assert_parity(got, want, WHAT, f"adjacency_grad N{N} G{G} Cu{Cu} slice of 9 channels:dadj")


# ---- msgat_edge_weight_grad ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,E,G,Cu,nsplit,per,why", F.EDGE_WEIGHT_GRAD_CASES,
                         ids=[f"N{c[0]}-G{c[2]}" for c in F.EDGE_WEIGHT_GRAD_CASES])
def test_edge_weight_grad_at_group_counts(N, E, G, Cu, nsplit, per, why):
    L = _lib.lib()
    graph, gs, rows, cols = _graph(N, E)
    nnz = graph.nnz
    shape = _lib.Shape(G, 1, Cu, Cu, N, T12)
    nbytes = int(L.msgat_edge_weight_grad_workspace_bytes(C_.byref(shape), C_.byref(gs), Cu))
    assert nbytes == (4 * nsplit * nnz if nsplit > 1 else 0), "the case left its branch"
    q, kW, lse, dv, feat = F.draw(G, Cu, N, T12, N + G, DEV)
    outs = []
    for _ in range(2):
        dval, ws = _nan(nnz), _nan(max(nbytes // 4, 1))
        _lib.check(L.msgat_edge_weight_grad(C_.byref(shape), C_.byref(gs), Cu, dv.data_ptr(), 0, feat.data_ptr(),
                                            q.data_ptr(), kW.data_ptr(), lse.data_ptr(), dval.data_ptr(),
                                            ws.data_ptr() if nbytes else None, nbytes, _stream()), "msgat_edge_weight_grad")
        outs.append(dval)
    got = _same_bits(outs, "dval")
    want = F.edge_adjacency_grad(q, kW, lse, dv, feat, 1, rows, cols)[0]
    assert_parity(got, want, WHAT, f"edge_weight_grad N{N} nnz{nnz} G{G} nsplit{nsplit} per{per}:dval")


# ---- msgat_edge_weight_grad_sets -----------------------------------------------------------------------------------

def _edge_weight_grad_sets(R, Bg, V, extra):
    L = _lib.lib()
    N, E, Cu = 64, 70, 3
    graph, gs, rows, cols = _graph(N, E)
    nnz, G = graph.nnz, R * Bg
    shape = _lib.Shape(R, Bg, Cu, Cu, N, T12)
    assert int(L.msgat_edge_weight_grad_sets_workspace_bytes(C_.byref(shape), C_.byref(gs), Cu, V)) == 0
    q, kW, lse, dv, feat = F.draw(G, Cu, N, T12, 100 * R + Bg, DEV)
    dEx = torch.randn(G, nnz, generator=torch.Generator().manual_seed(R + Bg)).to(DEV) if extra else None
    outs = []
    for _ in range(2):
        dval = _nan(V, nnz)
        _lib.check(L.msgat_edge_weight_grad_sets(C_.byref(shape), C_.byref(gs), Cu, dv.data_ptr(), 0, feat.data_ptr(),
                                                 q.data_ptr(), kW.data_ptr(), lse.data_ptr(), _ptr(dEx), V, dval.data_ptr(),
                                                 None, 0, _stream()), "msgat_edge_weight_grad_sets")
        outs.append(dval)
    return _same_bits(outs, "dval"), F.edge_adjacency_grad(q, kW, lse, dv, feat, V, rows, cols, dEx)


# groups per set -> the kernel's NG form (csrc/edge_weight_grad.hip: up to 4 a template parameter, 0 = four at a
# time with the slots past the last group skipped): 4; then 4 + 1, 4 + 4 and 4 + 4 + 1 groups per trip
_NG_FORM = {4: 4, 5: 0, 8: 0, 9: 0}


@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("Bg", [3, 9])     # 3 and 9 sets: the last round over the 8 XCD labels is not full
@pytest.mark.parametrize("R", sorted(_NG_FORM))
def test_edge_weight_grad_sets_with_many_groups_per_set(R, Bg, extra):
    assert (R * Bg) // Bg == R and _NG_FORM[R] == (R if R <= 4 else 0)
    got, want = _edge_weight_grad_sets(R, Bg, Bg, extra)
    assert_parity(got, want, WHAT, f"edge_weight_grad_sets R{R} Bg{Bg} NG{_NG_FORM[R]} extra{int(extra)}:dval")


def test_edge_weight_grad_sets_one_set_per_group():
    got, want = _edge_weight_grad_sets(5, 3, 15, True)
    assert_parity(got, want, WHAT, "edge_weight_grad_sets R5 Bg3 V15 NG1 extra1:dval")


# ---- msgat_edge_softmax_grad ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,Bg,V,dense", [(35, 1, 1, True), (35, 1, 1, False), (5, 3, 3, True)])
def test_edge_softmax_grad_adds_to_its_target(R, Bg, V, dense):
    L = _lib.lib()
    N, E = 64, 70
    graph, gs, rows, cols = _graph(N, E)
    nnz, G = graph.nnz, R * Bg
    shape = _lib.Shape(R, Bg, 1, 0, N, T12)
    q, kW, lse, _, _ = F.draw(G, 1, N, T12, 300 + G + V, DEV)
    gen = torch.Generator().manual_seed(G)
    dEx = torch.randn(G, nnz, generator=gen).to(DEV)
    before = torch.randn((V, N, N) if dense else (nnz,), generator=gen).to(DEV)
    outs = []
    for _ in range(2):
        dst = before.clone()
        _lib.check(L.msgat_edge_softmax_grad(C_.byref(shape), C_.byref(gs), q.data_ptr(), kW.data_ptr(), lse.data_ptr(),
                                             dEx.data_ptr(), V, _ptr(dst if dense else None), _ptr(None if dense else dst),
                                             _stream()), "msgat_edge_softmax_grad")
        outs.append(dst)
    got = _same_bits(outs, "target").double() - before.double()
    share = torch.zeros(V, nnz, dtype=torch.float64, device=DEV)
    for g in range(G):
        share[g % V] += F.edge_softmax(q, kW, lse, g, rows, cols) * dEx[g].double()
    if dense:
        want = torch.zeros(V, N, N, dtype=torch.float64, device=DEV)
        want[:, rows, cols] = share
        off = torch.ones(N, N, dtype=torch.bool, device=DEV)
        off[rows, cols] = False
        assert torch.equal(outs[0][:, off], before[:, off]), "an entry outside the structure changed"
    else:
        want = share[0]
    assert_parity(got, want, WHAT, f"edge_softmax_grad G{G} V{V} {'dense' if dense else 'values'}:added")


def test_edge_softmax_grad_refuses_value_sets_on_a_values_target():
    """the [nnz] target of the sparse form is one value set (include/msgat_hip.h): V = Bg = 3 is a shape error, not a launch"""
    graph, gs, _, _ = _graph(64, 70)
    shape = _lib.Shape(5, 3, 1, 0, 64, T12)
    buf = torch.zeros(15 * 64 * T12, device=DEV)
    dst = torch.zeros(3 * graph.nnz, device=DEV)
    st = _lib.lib().msgat_edge_softmax_grad(C_.byref(shape), C_.byref(gs), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                            buf.data_ptr(), 3, None, dst.data_ptr(), _stream())
    assert st == -2


# ---- msgat_attention_map and msgat_softmax_map_grad ----------------------------------------------------------------

def _hold(got, want, key, floor=0.0):
    """assert_parity; `floor` > 0: a quantity whose exact value is 0 is held to the bar on that absolute scale instead"""
    if floor > 0.0:
        e = min(rel_err(got, want), float((got.double() - want).abs().max()) / floor)
        record_err(WHAT, key, e, 1e-4)
        assert e < 1e-4, f"{key}: {e:.3e}"
    else:
        assert_parity(got, want, WHAT, key)


# 1, 3: less than a 16-tile; 17: one row past it; 31: the second wave of a 32-row block has 15 rows; 65: a remainder of 1
# on both 64-tile axes; 68, 100: N % 4 == 0 but N % 16 != 0, the 16-byte forms with a partial 16-tile.
# (3, 32, 130): 96 groups, 96 partials per relation in the dWg sum
@pytest.mark.parametrize("R,Bg,N", [(2, 2, N) for N in (1, 3, 17, 31, 65, 68, 100)] + [(3, 32, 130)])
def test_attention_map_and_its_gradient(R, Bg, N):
    L = _lib.lib()
    G, T = R * Bg, T12
    shape = _lib.Shape(R, Bg, 1, 0, N, T)
    q, kW, lse, _, _ = F.draw(G, 1, N, T, 500 + N, DEV)
    gen = torch.Generator().manual_seed(N)
    Wg = (torch.randn(R, T, T, generator=gen) * 0.3).to(DEV)
    dP = torch.randn(G, N, N, generator=gen).to(DEV)
    dq0, dWg0 = torch.randn(G, N, T, generator=gen).to(DEV), torch.randn(R, T, T, generator=gen).to(DEV)
    nbytes = int(L.msgat_softmax_map_grad_workspace_bytes(C_.byref(shape)))
    assert nbytes > 0
    maps, dqs, dWgs = [], [], []
    for _ in range(2):
        out, ws = _nan(G, N, N), _nan(nbytes // 4)
        dq, dWg = dq0.clone(), dWg0.clone()
        _lib.check(L.msgat_attention_map(C_.byref(shape), q.data_ptr(), kW.data_ptr(), lse.data_ptr(), out.data_ptr(),
                                         _stream()), "msgat_attention_map")
        _lib.check(L.msgat_softmax_map_grad(C_.byref(shape), q.data_ptr(), kW.data_ptr(), lse.data_ptr(), Wg.data_ptr(),
                                            dP.data_ptr(), dq.data_ptr(), dWg.data_ptr(), ws.data_ptr(), nbytes, _stream()),
                   "msgat_softmax_map_grad")
        maps.append(out), dqs.append(dq), dWgs.append(dWg)
    key = f"map R{R} Bg{Bg} N{N}"
    assert_parity(_same_bits(maps, "map"), F.softmax_map(q, kW, lse), WHAT, key + ":P")
    want_dq, want_dWg = F.softmax_map_grad(q, kW, lse, Wg, dP, Bg)
    # one node: P is 1 and dS is 0 exactly; held on the O(1) scale of the inputs
    floor = 1.0 if N == 1 else 0.0
    _hold(_same_bits(dqs, "dq").double() - dq0.double(), want_dq, key + ":dq_added", floor)
    _hold(_same_bits(dWgs, "dWg").double() - dWg0.double(), want_dWg, key + ":dWg_added", floor)
