"""CPU: a per-sample adjacency [B,N,N] (attention.py:22 documents `adjacency: [..., n_nodes, n_nodes]`).

The reference's fixtures of tests/golden/make_golden_batched.py against the dense restatement (its `* adj` broadcasts
over the batch); the host side of `BatchedGraph` -- one union structure, values per object; the refusals of
`graph.graph_for`; and the library's argument checks of the value sets, none of which needs a device.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import dense_torch

import ms_gat_amd
from ms_gat_amd import _lib
from ms_gat_amd.graph import BatchedGraph, graph_for

GACN_FIXTURES = ["batched_gacn_b3c1n64.npz", "batched_gacn_b3c3n64.npz", "batched_gacn_b2c72n47.npz"]


def _inputs(g):
    if "x_q32" in g:
        return g["x_q32"].astype(np.float32) / 32, g["dz_q32"].astype(np.float32) / 32
    return g["x"].astype(np.float32), g["dz"].astype(np.float32)


def test_fixtures_have_a_different_pattern_per_sample():
    for name in ["batched_gatt_b3c3n64.npz", "batched_meam_72to72_n32.npz"] + GACN_FIXTURES:
        adj = load_golden(name)["adj"]
        assert adj.ndim == 3 and adj.shape[0] >= 2, name
        masks = adj != 0
        assert not np.array_equal(masks[0], masks[1]), name
        assert not np.allclose(adj[0][masks[0] & masks[1]], adj[1][masks[0] & masks[1]]), name


def test_graph_attention_fixture_against_dense_restatement():
    g = load_golden("batched_gatt_b3c3n64.npz")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    x = t(g["x"].astype(np.float32)).requires_grad_(True)
    Wg, alpha = t(g["Wg"]).requires_grad_(True), t(g["alpha"]).requires_grad_(True)
    y = dense_torch.graph_attention_dense(x, t(g["adj"]), Wg, alpha)
    y.backward(t(g["dy"].astype(np.float32)))
    for got, key in ((y.detach(), "y"), (x.grad, "dx"), (Wg.grad, "dWg"), (alpha.grad, "dalpha")):
        assert rel_err(got, g[key]) < 5e-6, key


@pytest.mark.parametrize("name", GACN_FIXTURES)
def test_gacn_fixtures_against_dense_restatement(name):
    g = load_golden(name)
    xn, dzn = _inputs(g)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    x = t(xn).requires_grad_(True)
    Wg, alpha, W = (t(g[k]).requires_grad_(True) for k in ("Wg", "alpha", "W"))
    z = dense_torch.gacn_dense(x, t(g["adj"]), Wg, alpha, W)
    z.backward(t(dzn))
    for got, key in ((z.detach(), "z"), (x.grad, "dx"), (Wg.grad, "dWg"), (alpha.grad, "dalpha"), (W.grad, "dW")):
        assert rel_err(got, g[key]) < 5e-6, (name, key)


def test_meam_fixture_against_dense_restatement():
    g = load_golden("batched_meam_72to72_n32.npz")
    p = {k[2:]: torch.from_numpy(v).requires_grad_(True) for k, v in g.items() if k.startswith("p.")}
    x = torch.from_numpy(g["x"].astype(np.float32)).requires_grad_(True)
    out = dense_torch.meam_dense(x, torch.from_numpy(g["adj"]), p, [1, 2])
    out.backward(torch.from_numpy(g["dout"].astype(np.float32)))
    assert rel_err(out.detach(), g["out"]) < 5e-6
    assert rel_err(x.grad, g["dx"]) < 5e-6
    for k, v in p.items():
        assert rel_err(v.grad, g[f"g.{k}"]) < 5e-5, k


def _random_batch(V, N, seed, density=0.08):
    rng = np.random.default_rng(seed)
    a = (rng.random((V, N, N)) < density) * rng.uniform(0.1, 1.0, (V, N, N))
    return torch.from_numpy(a.astype(np.float32))


def test_union_structure_is_the_csr_of_the_or_of_the_masks():
    adj = _random_batch(4, 37, 0)
    bg = BatchedGraph(adj)
    mask = (adj.numpy() != 0).any(0)
    rows, cols = np.nonzero(mask)                       # row-major: the CSR order
    assert bg.nnz == len(rows) and bg.n_sets == 4 and bg.n_nodes == 37
    s = bg.structure
    np.testing.assert_array_equal(s.rowptr.numpy(), np.concatenate([[0], np.cumsum(mask.sum(1))]))
    np.testing.assert_array_equal(s.col[: bg.nnz].numpy(), cols)
    np.testing.assert_array_equal(s.erow[: bg.nnz].numpy(), rows)
    np.testing.assert_array_equal(bg.val[:, : bg.nnz].numpy(), adj.numpy()[:, rows, cols])
    assert torch.equal(bg.dense(), adj)
    bg.check()                                          # nothing outside the union
    s.validate()


def test_pattern_is_shared_and_values_are_not():
    a = _random_batch(3, 29, 1)
    b = a * 2.0                                         # same pattern, other weights
    ga, gb = BatchedGraph(a), BatchedGraph(b)
    assert ga.structure is gb.structure                 # one structure (and its device copies) per pattern
    assert ga.val.data_ptr() != gb.val.data_ptr()
    assert torch.equal(gb.val, 2.0 * ga.val)
    assert ga.on("cpu")[0].val != gb.on("cpu")[0].val
    assert ga.on("cpu")[0].val_sets == 3
    assert ga.on("cpu")[0].rowptr == gb.on("cpu")[0].rowptr


def test_update_refills_in_place_and_check_catches_edges_outside_the_pattern():
    a = _random_batch(2, 23, 2)
    g = BatchedGraph(a)
    ptr = g.val.data_ptr()
    a2 = a * 0.5
    g.update_(a2)
    assert g.val.data_ptr() == ptr and torch.equal(g.dense(), a2)
    g.check()
    a3 = a2.clone()
    r, c = np.argwhere(~(a.numpy() != 0).any(0))[0]
    a3[1, r, c] = 1.0                                   # an edge the union structure lacks
    g.update_(a3)
    with pytest.raises(_lib.MsgatError, match="outside"):
        g.check()


def test_nan_counts_as_an_edge_like_the_shared_path():
    a = _random_batch(2, 16, 3)
    a[0, 3, 4], a[1, 3, 4] = float("nan"), 0.0
    g = BatchedGraph(a)
    assert bool(((g.structure.erow[: g.nnz] == 3) & (g.structure.col[: g.nnz] == 4)).any())


def test_graph_for_shapes():
    a = _random_batch(4, 12, 4)
    assert isinstance(graph_for(a, 4, 1), BatchedGraph)           # [B,N,N], one relation
    assert graph_for(a, 12, 3).n_sets == 4                         # [B,N,N] shared by R = 3 relations
    assert graph_for(_random_batch(12, 12, 5), 12, 3).n_sets == 12   # [R*B,N,N]
    one = graph_for(a[:1], 4, 1)
    assert isinstance(one, ms_gat_amd.SparseGraph)                 # [1,N,N] is [N,N]
    assert torch.equal(one.dense(), a[0])
    for bad, groups, rel, allowed in ((a, 6, 1, "[1, 6]"), (a, 6, 3, "[1, 2, 6]"), (a[:3], 4, 1, "[1, 4]")):
        with pytest.raises(ValueError, match="leading size") as e:
            graph_for(bad, groups, rel)
        assert allowed in str(e.value) and str(tuple(bad.shape)) in str(e.value)


def test_batched_adjacency_that_requires_grad_is_refused_while_recording():
    a = _random_batch(2, 10, 6).requires_grad_(True)
    with pytest.raises(ValueError, match="requires grad"):
        graph_for(a, 2, 1)
    with torch.no_grad():
        assert isinstance(graph_for(a, 2, 1), BatchedGraph)
    assert isinstance(graph_for(a.detach(), 2, 1), BatchedGraph)


def test_library_checks_value_sets_and_edge_value_arguments():
    L = _lib.lib()
    g = BatchedGraph(_random_batch(3, 20, 7))
    hs, _ = g.on("cpu")
    for R, Bg, sets, ok in ((1, 3, 3, True), (2, 3, 3, True), (2, 3, 6, True), (1, 3, 0, True), (1, 3, 1, True),
                            (1, 3, 2, False), (2, 3, 4, False), (1, 3, -1, False)):
        hs.val_sets = sets
        sh = _lib.Shape(R, Bg, 3, 0, 20, 12)
        got = L.msgat_bwd_workspace_bytes(C.byref(sh), C.byref(hs))   # 0 when check_graph refuses the graph
        assert (got > 0) == ok, (R, Bg, sets)
    hs.val_sets = 3
    out = torch.zeros(1, dtype=torch.int32)
    assert L.msgat_graph_edge_values(None, 1, 3, g.val.data_ptr(), out.data_ptr(), None) == _lib.MSGAT_OK - 1
    assert L.msgat_graph_edge_values(C.byref(hs), None, 3, g.val.data_ptr(), out.data_ptr(), None) == -1
    assert L.msgat_graph_edge_values(C.byref(hs), 1, 3, g.val.data_ptr(), None, None) == -1
    assert L.msgat_graph_edge_values(C.byref(hs), 1, 0, g.val.data_ptr(), out.data_ptr(), None) == -2
    assert L.msgat_graph_edge_values(C.byref(hs), 1, 1 << 30, g.val.data_ptr(), out.data_ptr(), None) == -3
