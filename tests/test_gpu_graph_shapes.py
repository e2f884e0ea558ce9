"""GPU: the core graph attention on skewed, directed and hollow graphs (tests/graph_shape_fixtures.py).

Every other GPU test of the attention hot path builds its graph with `synthetic_adjacency`: a symmetric pattern (the rows
form and the columns form of the SELL layout coincide, and so do CSR and CSC up to `cperm`), a self loop on every node (no
empty row or column, no SELL slice of width 0), degrees within ~3x of the mean, and -- but for one case -- `pair_trips`
far from the 12 | 13 at which the SDDMM leaves its registers, and row blocks far from the 1024 | 1025 edges at which the
score kernels stop caching their tail.  Here the same kernels run on hand-built graphs that are none of that; what each
fixture is, and that the library's builder lays it out as claimed, is asserted on the host (test_graph_shapes_cpu.py),
which also shows that the reference's own fp32 arithmetic sits a factor ten under the bar on every one of them.

All comparisons are against float64 at the bar of 1e-4 with the per-entry rule of `assert_close`; the achieved errors go
on record through `record_err` (MSGAT_PARITY_LOG; profiles/graph_shapes/parity_rel_err.tsv).
"""
import ctypes

import numpy as np
import pytest
import torch

import graph_shape_fixtures as F
from conftest import assert_parity, record_err, rel_err
from test_gpu_parity import assert_close, oracle_f64, run_ours

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_WANT, _GOT = {}, {}


def _seed(C):
    return 300 + C          # the seed of the host-side yardstick (test_graph_shapes_cpu.py)


def _want(name, C, Co, T=12, Bg=2, R=2):
    """the float64 oracle of one problem, computed once"""
    key = (name, C, Co, T, Bg, R)
    if key not in _WANT:
        _WANT[key] = oracle_f64(*F.problem(name, C, Co, T, Bg, R, _seed(C)))
    return _WANT[key]


def _got(name, C, Co, sell, T=12, Bg=2, R=2):
    """one forward + backward of ops.gacn on `name` with the edge layout `sell` (None: the library's own choice for a dense
    tensor), run twice: no float atomics anywhere, so the second run must repeat the first bit for bit"""
    key = (name, C, Co, T, Bg, R, sell)
    if key not in _GOT:
        prob = F.problem(name, C, Co, T, Bg, R, _seed(C))
        first, second = run_ours(*prob, sell=sell), run_ours(*prob, sell=sell)
        for k in first:
            assert np.array_equal(first[k], second[k]), f"{name} {sell} {k}: the second run differs from the first"
        _GOT[key] = first
    return _GOT[key]


def _assert_empty_rows_are_exact_zeros(name, z):
    """a node without an entry in its row aggregates nothing, and no mode adds a bias: exactly 0, not 1e-30, not NaN"""
    row_deg, _ = F.degrees(name)
    empty = np.flatnonzero(row_deg == 0)
    assert (z[:, :, empty, :] == 0).all(), f"{name}: rows without an entry are not exact zeros in z"
    assert np.isfinite(z).all()


def _mode(C, Co):
    return "PLAIN" if Co == 0 else "PROJ_FIRST" if C > Co else "AGG_FIRST"


# ---- a + f: the whole layer on both edge layouts ------------------------------------------------------------------------

_LAYER_CASES = [(name, *F.MODES[mode]) for name in F.LAYER for mode in F.MODES] + \
    [("hub130", 72, 24)] + \
    [(name, *F.WIDE[mode]) for name in F.WIDE_NAMES for mode in F.WIDE] + \
    [(name, *F.MODES[mode]) for name in F.SMALL for mode in ("AGG_FIRST", "PROJ_FIRST")]


@pytest.mark.parametrize("name,C,Co", _LAYER_CASES, ids=[f"{n}-{_mode(c, o)}-{c}to{o}" for n, c, o in _LAYER_CASES])
def test_whole_layer_on_the_csr_and_on_the_sell_kernels(name, C, Co):
    """ops.gacn forward + backward (z, dx, dWg, dalpha, dW) with sell="never" -- the CSR aggregate, the CSC gather or, in
    PROJ_FIRST, the fused k_agg_sddmm, k_sddmm on erow / col -- and with sell="always" -- k_agg_sell on the rows form forward and
    on the columns form backward, k_sddmm_sellreg / k_sddmm_sell on the rows form, the partials mapped back through
    sell.pos -- against float64, and against each other at the 5e-6 of
    test_sell_edge_layout_agrees_with_the_csr_kernels_and_the_oracle.  On these directed patterns the rows form and the
    columns form differ, so reading the wrong one of a pair does not go unnoticed; `hub130` has an odd slice count whose
    widest slice is paired with one of width 0, `hollow200` three slices of width 0, `lonely65_*` a slice of one row,
    `edge70` a single stored entry (fewer than the 8 edges several kernels window over), `cross64` / `cross65` a full row and
    a full column and nothing else.  (hub130, 72 -> 24) is the fused k_agg_sddmm with a column of 123 entries against its
    eight register slots.  With at most 4 channels under the attention the backward forms the edge gradient in its row pass
    and launches no SDDMM, so at C = 3 only PROJ_FIRST reaches one; the C = 6 cases (graph_shape_fixtures.WIDE) put PLAIN and
    AGG_FIRST behind k_sddmm (CSR) and the SELL forms on C channels."""
    want = _want(name, C, Co)
    what = f"graph shapes {name} {_mode(C, Co)} C={C}->{Co}"
    csr, sell = _got(name, C, Co, "never"), _got(name, C, Co, "always")
    assert_close(csr, want, what=what + " CSR")
    assert_close(sell, want, what=what + " SELL")
    assert_close(sell, csr, tol=5e-6, what=what + " SELL vs CSR kernels")
    for got in (csr, sell):
        _assert_empty_rows_are_exact_zeros(name, got["z"])


@pytest.mark.parametrize("mode", ["AGG_FIRST", "PROJ_FIRST"])
@pytest.mark.parametrize("T", [4, 16])
@pytest.mark.parametrize("name", ["hub130", "hollow200"])
def test_sell_kernels_at_the_other_timestep_counts(name, T, mode):
    C, Co = F.MODES[mode]
    got = _got(name, C, Co, "always", T=T)
    assert_close(got, _want(name, C, Co, T=T), what=f"graph shapes {name} {mode} T={T} SELL")
    _assert_empty_rows_are_exact_zeros(name, got["z"])


@pytest.mark.parametrize("mode", ["AGG_FIRST", "PROJ_FIRST"])
def test_csr_kernels_at_eight_timesteps(mode):
    """`hub130` with sell="never" at T = 8: the CSR / CSC forms (the ring's neighbours k_agg_lds and k_agg_proj, the fused
    k_agg_sddmm in PROJ_FIRST) at a timestep count that the other cases reach on the SELL forms only."""
    C, Co = F.MODES[mode]
    got = _got("hub130", C, Co, "never", T=8)
    assert_close(got, _want("hub130", C, Co, T=8), what=f"graph shapes hub130 {mode} T=8 CSR")
    _assert_empty_rows_are_exact_zeros("hub130", got["z"])


# ---- a': the CSR forms of graphs whose [N,T] slab does not fit the LDS ------------------------------------------------------

_LDS_MAX = 160 * 1024       # kLdsMax (common.hpp); a kernel's dynamic LDS may take all of it but 1 KiB
_DIRECT_MAX = 4             # bwd_rows_direct_max_channels() (scores.hip): up to here the row pass forms the edge gradient itself


def _oracle_f64_gpu(x, adj, Wg, alpha, W, dz):
    """oracle/dense_torch.py in float64 with autograd on the GPU (the numpy oracle's dense [N,N] passes take minutes here)"""
    from oracle import dense_torch
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(DEV)  # noqa: E731
    R = Wg.shape[0]
    Bg = x.shape[0] // R
    outs = dict(z=[], dx=[], dWg=[], dalpha=[], dW=[])
    for r in range(R):
        xt, Wgt, at, Wt = (f(v).requires_grad_(True) for v in (x[r * Bg:(r + 1) * Bg], Wg[r], alpha[r], W[r]))
        z = dense_torch.gacn_dense(xt, f(adj), Wgt, at, Wt)
        z.backward(f(dz[r * Bg:(r + 1) * Bg]))
        for k, v in (("z", z.detach()), ("dx", xt.grad), ("dWg", Wgt.grad), ("dalpha", at.grad), ("dW", Wt.grad)):
            outs[k].append(v.cpu().numpy())
    return dict(z=np.concatenate(outs["z"]), dx=np.concatenate(outs["dx"]), dWg=np.stack(outs["dWg"]),
                dalpha=np.stack(outs["dalpha"]), dW=np.stack(outs["dW"]))


@pytest.mark.parametrize("name,C,Co,form", [("wide2545", 6, 3, "k_agg_cols"), ("few2545", 6, 3, "k_agg_glb"),
                                            ("wide2545", 10, 5, "k_sddmm<T4, false>")],
                         ids=["agg_cols", "agg_glb", "sddmm_no_slab"])
def test_csr_forms_without_a_slab(name, C, Co, form):
    """PROJ_FIRST at T = 16, R = 1, Bg = 2, sell="never", N = 2545: the smallest N whose [N,16] slab does not fit the LDS
    (launch_aggregate_t, launch_sddmm_t: slab_channels() == 0), so that the aggregate -- forward on the CSR, backward on the
    CSC, the backward cannot fuse -- runs one 4-timestep column at a time (k_agg_cols: nnz >= 8, a row of 20 and a column of
    15 entries against the 8-slot window) or, on the graph of five entries, gathers from memory with the scalar walk of
    gather_row (k_agg_glb).  On Cu = 3 channels the row pass forms the edge gradient itself (direct_c) and no SDDMM is launched
    at all; the third case has Cu = 5 and reaches k_sddmm<T4, false>, the SDDMM without a slab.  The conditions of each form
    are asserted here as the launchers state them, so a threshold that moves fails the test.  Against float64; two runs
    with equal bits (_got); rows without an entry exact zeros."""
    import ms_gat_amd
    T, Bg, R = 16, 2, 1
    adj = F.adjacency(name)
    N = adj.shape[0]
    graph = ms_gat_amd.SparseGraph(torch.from_numpy(adj), sell="never")
    row_deg, col_deg = F.degrees(name)
    assert not graph.has_sell
    assert N * T * 4 > _LDS_MAX - 1024 and N * 16 <= _LDS_MAX - 1024      # no slab (nor a fused backward); a column fits
    if form == "k_agg_glb":
        assert graph.nnz < 8
    else:
        assert graph.nnz >= 8 and row_deg.max() > 8 and col_deg.max() > 8
    assert (row_deg == 0).any()
    assert (Co > _DIRECT_MAX) == form.startswith("k_sddmm")
    prob = F.problem(name, C, Co, T, Bg, R, _seed(C))
    got = _got(name, C, Co, "never", T=T, Bg=Bg, R=R)
    assert_close(got, _oracle_f64_gpu(*prob), what=f"graph shapes {name} PROJ_FIRST C={C}->{Co} T={T} {form}")
    _assert_empty_rows_are_exact_zeros(name, got["z"])


# ---- b: both sides of the SDDMM's register form -------------------------------------------------------------------------

_SDDMM_WIDTHS = [(mode, *F.MODES[mode]) for mode in F.MODES] + [(mode, *F.WIDE[mode]) for mode in F.WIDE]


@pytest.mark.parametrize("mode,C,Co", _SDDMM_WIDTHS, ids=[f"{m}-{c}to{o}" for m, c, o in _SDDMM_WIDTHS])
@pytest.mark.parametrize("lo,hi", [("trips12", "trips13"), ("pair12", "pair13")])
def test_both_sides_of_the_sddmm_register_threshold(lo, hi, mode, C, Co):
    """`pair_trips` 12 runs k_sddmm_sellreg (the per-edge sums in kRegTrips = 12 float4 registers per lane), 13 runs
    k_sddmm_sell (read-modify-write partials per channel chunk); once through one slice (`trips*`) and once through a pair
    of slices of 7 + 5 resp. 7 + 6 trips (`pair*`); on Co = 8 channels in PROJ_FIRST and on C = 6 in PLAIN / AGG_FIRST (at C = 3
    those two form the edge gradient in the row pass, without an SDDMM: they run here all the same).  Both must meet the
    bar.  The two graphs differ in one entry of one row, so they check each other too: the softmax is taken over all nodes
    before the mask, so every other row of z is the same sum of the same products on either graph (in an order the layout
    is free to choose: held to the 5e-6 between layouts).  The gradients are not row-local -- the touched row's delta
    moves its whole row of dS and with it every dq, so dx differs in every row -- and are held to float64 only."""
    import ms_gat_amd
    mode = f"{mode} C={C}->{Co}"
    for name, trips in ((lo, 12), (hi, 13)):
        graph = ms_gat_amd.SparseGraph(torch.from_numpy(F.adjacency(name)), sell="always")
        assert graph._sell["sell_rows"]["pair_trips"] == trips
        assert_close(_got(name, C, Co, "always"), _want(name, C, Co), what=f"SDDMM threshold {name} pair_trips={trips} {mode}")
    others = np.setdiff1d(np.arange(F.CLAIMS[lo]["n"]), [F.touched_row(hi)])
    z_lo, z_hi = (_got(name, C, Co, "always")["z"][:, :, others, :] for name in (lo, hi))
    e = rel_err(z_hi, z_lo)
    record_err(f"SDDMM threshold {hi} vs {lo} {mode}", "z[untouched rows]", e, 5e-6)
    assert e < 5e-6


# ---- c: both sides of the cached tail ------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", ["onerow1024", "onerow1025"])
def test_both_sides_of_the_cached_tail_threshold(name, C):
    """AGG_FIRST with the layer finished in the score kernels (C = 1: q computed in the kernel; C = 3): the first row block
    holds all 1024 resp. 1025 edges of the graph in its one row -- the last size whose tail columns and coefficients are
    cached in LDS (kTailEdges) and the first that reads them from memory -- and every other block has none."""
    got = _got(name, C, 24, None, Bg=1, R=1)
    assert_close(got, _want(name, C, 24, Bg=1, R=1), what=f"tail threshold {name} AGG_FIRST C={C}")
    _assert_empty_rows_are_exact_zeros(name, got["z"])
    assert (got["z"][:, :, 0, :] != 0).any()


@pytest.mark.parametrize("sell", ["never", "always"])
@pytest.mark.parametrize("name", ["onerow1024_T", "onerow1025_T"])
def test_one_column_stored_by_a_thousand_rows(name, sell):
    """PROJ_FIRST on the transposes: one column of degree 1024 / 1025 in the CSC gather of the backward (sell="never") and as a
    columns-form SELL slice of 256 / 257 trips beside sixteen of width 0 (sell="always")."""
    C, Co = F.MODES["PROJ_FIRST"]
    got = _got(name, C, Co, sell, Bg=1, R=1)
    assert_close(got, _want(name, C, Co, Bg=1, R=1), what=f"tail threshold {name} PROJ_FIRST sell={sell}")
    _assert_empty_rows_are_exact_zeros(name, got["z"])


# ---- d: stage level, the LDS-DMA ring -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ladder64", "hub130", "hollow200"])
def test_aggregate_ring_on_rows_of_every_degree(name):
    """msgat_stage_aggregate as test_aggregate_ring_against_float64 calls it, at G Cu = 16 x 32 = 512 slabs of N T / 4 <= 600
    float4: the persistent LDS-DMA ring (k_agg_ring), whose lanes hold an 8-edge window per slot, loop over the rest of a
    longer row, and recompute a slab's last slot where a lane has none.  Rows of every degree 0 .. 63, a row of 126, 160
    rows of degree 0 (their window reads other rows' edges, masked): against float64, three runs with equal bits, the
    output started from NaN, rows without an edge exact zeros."""
    import ms_gat_amd
    from ms_gat_amd import _lib
    L = _lib.lib()
    R, Bg, Cu, T = 2, 8, 32, 12
    G = R * Bg
    adj = F.adjacency(name)
    N = adj.shape[0]
    graph = ms_gat_amd.SparseGraph(torch.from_numpy(adj))
    nnz = graph.nnz
    # launch_aggregate_t's condition for the ring (aggregate.hip)
    assert not graph.has_sell and nnz >= 8 and N * (T // 4) <= 3 * 1024 and G * Cu >= 512
    gs, _keep = graph.on(DEV)
    g = torch.Generator().manual_seed(29)
    u = torch.randn(G, Cu, N, T, generator=g).to(DEV)
    Ee = torch.rand(G, nnz, generator=g).to(DEV)
    shape = _lib.Shape(R, Bg, Cu, Cu, N, T)
    nscr = int(L.msgat_edge_scratch_floats(ctypes.byref(shape), ctypes.byref(gs)))
    escr = torch.empty(max(nscr, 1), device=DEV)
    outs = []
    for _ in range(3):
        v = torch.full((G, Cu, N, T), float("nan"), device=DEV)
        st = L.msgat_stage_aggregate(ctypes.byref(shape), ctypes.byref(gs), Cu, u.data_ptr(), Ee.data_ptr(), v.data_ptr(),
                                     escr.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "msgat_stage_aggregate")
        outs.append(v)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    rowptr = graph.rowptr.long()
    col = graph.col[:nnz].long().to(DEV)
    rows = torch.repeat_interleave(torch.arange(N), rowptr[1:] - rowptr[:-1]).to(DEV)
    want = torch.zeros(G, Cu, N, T, device=DEV, dtype=torch.float64)
    want.index_add_(2, rows, u.double()[:, :, col, :] * Ee.double()[:, None, :, None])
    err = rel_err(outs[0], want)
    record_err(f"aggregate ring on {name} G={G} Cu={Cu} T={T}", "v", err, 1e-5)
    assert err < 1e-5
    empty = torch.from_numpy(np.flatnonzero(F.degrees(name)[0] == 0)).to(DEV)
    assert empty.numel() > 0 and (outs[0][:, :, empty, :] == 0).all()


# ---- e: the gradient at the stored entries ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["AGG_FIRST", "PROJ_FIRST"])
@pytest.mark.parametrize("name,layout", [("hub130", "coo"), ("hub130", "csr"), ("hollow200_T", "coo"), ("ladder64", "coo"),
                                         ("trips13", "coo")])
def test_gradient_at_the_stored_entries_of_a_directed_pattern(name, layout, mode):
    """The adjacency as a torch sparse tensor (COO; CSR too on `hub130`) whose values require grad, through ops.gacn:
    `values.grad` against float64 autograd of the dense op sequence with the adjacency as a leaf, read at the stored
    positions (`stored_entry_grad_f64`; checked against a finite difference on the host).  The per-edge partials of the
    backward come out in CSC order or through the SDDMM's own order and are mapped back to the caller's entries: on a
    directed pattern a partial mapped through the wrong permutation lands on another edge.  (A sparse adjacency takes the
    library's own choice of layout: CSR / CSC at these sizes.)"""
    from ms_gat_amd import ops
    C, Co = F.MODES[mode]
    x, adj, Wg, alpha, W, dz = F.problem(name, C, Co, 12, 2, 2, _seed(C))
    rows, cols, want = F.stored_entry_grad_f64(x, adj, Wg, alpha, W, dz)
    dev = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)  # noqa: E731
    vals = torch.nn.Parameter(dev(adj[rows, cols]))
    N = adj.shape[0]
    if layout == "coo":
        a = torch.sparse_coo_tensor(dev(np.stack([rows, cols]), torch.int64), vals, (N, N), is_coalesced=True)
    else:
        crow = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))])
        a = torch.sparse_csr_tensor(dev(crow, torch.int64), dev(cols, torch.int64), vals, (N, N))
    xt = dev(x).requires_grad_(True)
    z = ops.gacn(xt, dev(alpha), dev(Wg), dev(W), a)
    z.backward(dev(dz))
    torch.cuda.synchronize()
    what = f"stored-entry gradient {name} {layout} {mode}"
    oracle = _want(name, C, Co)
    assert_parity(z, oracle["z"], what, "z")
    assert_parity(xt.grad, oracle["dx"], what, "dx")
    assert_parity(vals.grad, want, what, "dval")
