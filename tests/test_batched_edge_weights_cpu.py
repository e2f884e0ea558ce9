"""CPU: a per-sample sparse adjacency [V,N,N] -- the argument checks of msgat_edge_weight_grad_sets (the gradient of its
stored values, one value set per sample or per group) and the host mapping from the samples' stored entries to the
union structure's [V, nnz_union] value buffer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

from ms_gat_amd import _lib, ops
from ms_gat_amd import graph as G
from ms_gat_amd.graph import SparseGraph


def test_symbols_declared_prototyped_and_exported():
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "msgat_hip.h")).read()
    for name in ("msgat_edge_weight_grad_sets", "msgat_edge_weight_grad_sets_workspace_bytes"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib._PROTOTYPES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().msgat_abi_version() == 10


def test_argument_checks_launch_nothing():
    L = _lib.lib()
    g = SparseGraph.from_indices(torch.tensor([0, 2, 3, 3]), torch.tensor([0, 2, 1]), 3)
    hs = g.host_struct()
    sh = _lib.Shape(3, 2, 3, 0, 3, 12)          # R = 3, Bg = 2: n_sets in {1, 2, 6}
    fake = 16   # never dereferenced: every call below must fail its checks before any launch
    names = ["shape", "graph", "Cu", "dv", "dv_gc", "feat", "q", "kW", "lse", "dE", "n_sets", "dval", "ws", "ws_bytes",
             "stream"]

    def call(**kw):
        a = [C.byref(sh), C.byref(hs), 3, fake, 0, fake, fake, fake, fake, None, 2, fake, None, 0, None]
        for k, v in kw.items():
            a[names.index(k)] = v
        return L.msgat_edge_weight_grad_sets(*a)

    assert call(shape=None) == -1
    assert call(graph=None) == -1
    assert call(Cu=0) == -2
    assert call(Cu=257) == -3
    assert call(dv_gc=2) == -2               # a slice of fewer channels than Cu
    assert call(dv_gc=-1) == -2
    for bad in (0, -1, 3, 4, 5, 7, 12):
        assert call(n_sets=bad) == -2, bad
        assert L.msgat_edge_weight_grad_sets_workspace_bytes(C.byref(sh), C.byref(hs), 3, bad) == 0
    for name in ("dv", "feat", "q", "kW", "lse", "dval"):
        assert call(**{name: None}) == -1, name
        assert call(**{name: None, "n_sets": 6}) == -1, name
    bad_t = _lib.Shape(3, 2, 3, 0, 3, 10)
    assert call(shape=C.byref(bad_t)) == -3
    other_n = _lib.Shape(3, 2, 3, 0, 4, 12)
    assert call(shape=C.byref(other_n)) == -2   # graph of 3 nodes, signals of 4
    assert L.msgat_edge_weight_grad_sets_workspace_bytes(C.byref(other_n), C.byref(hs), 3, 2) == 0
    # every (set, edge) has one owner: no workspace; one set is msgat_edge_weight_grad and has its workspace and checks
    assert L.msgat_edge_weight_grad_sets_workspace_bytes(C.byref(sh), C.byref(hs), 3, 2) == 0
    assert L.msgat_edge_weight_grad_sets_workspace_bytes(C.byref(sh), C.byref(hs), 3, 6) == 0
    need = L.msgat_edge_weight_grad_sets_workspace_bytes(C.byref(sh), C.byref(hs), 3, 1)
    assert need == L.msgat_edge_weight_grad_workspace_bytes(C.byref(sh), C.byref(hs), 3) > 0
    assert call(n_sets=1, ws=None, ws_bytes=need) == -1
    assert call(n_sets=1, ws=fake, ws_bytes=need - 1) == -4
    # a graph without edges launches nothing and reads nothing
    empty = SparseGraph.from_indices(torch.tensor([0, 0, 0, 0]), torch.tensor([], dtype=torch.int64), 3)
    es = empty.host_struct()
    assert call(graph=C.byref(es), dval=None) == 0


def _fixture_coo():
    adj = load_golden("adjgrad_gacn_b3c3n64_bnn.npz")["adj"]
    V, N = adj.shape[0], adj.shape[1]
    v, i, j = np.nonzero(adj)
    coo = torch.sparse_coo_tensor(torch.from_numpy(np.stack([v, i, j])), torch.from_numpy(adj[v, i, j]), (V, N, N),
                                  is_coalesced=True)
    return adj, coo


def test_coo_union_structure_and_flat_map_reproduce_numpy():
    adj, coo = _fixture_coo()
    V, N = adj.shape[0], adj.shape[1]
    per_sample = [int((adj[v] != 0).sum()) for v in range(V)]
    union = (adj != 0).any(0)
    common = (adj != 0).all(0)
    # the differing-pattern path must really be exercised
    assert all(n < int(union.sum()) for n in per_sample), (per_sample, int(union.sum()))
    assert (per_sample, int(union.sum()), int(common.sum())) == ([127, 126, 127], 254, 63)

    sets = G.sparse_sets_of(coo)
    s = sets.structure
    assert sets.n_sets == V and s.n_nodes == N and s.nnz == int(union.sum()) and sets.flat is not None
    s.validate()
    erow, col = s.erow[: s.nnz].numpy(), s.col[: s.nnz].numpy()
    ur, uc = np.nonzero(union)                                  # row-major = CSR order
    assert np.array_equal(erow, ur) and np.array_equal(col, uc)
    g = sets.graph(coo._values())
    assert g.n_sets == V and g.nnz == s.nnz and g.structure is s
    buf = g.val.view(V, -1).numpy()
    assert buf.shape == (V, s.nnz)
    assert np.array_equal(buf, adj[:, erow, col])               # everywhere: an edge a sample lacks is an explicit 0
    assert int((buf == 0).sum()) == V * s.nnz - sum(per_sample)
    assert np.array_equal(g.dense().numpy(), adj)
    # the flat map, entry by entry
    v, i, j = coo._indices().numpy()
    flat = sets.flat.numpy()
    assert np.array_equal(flat // s.nnz, v)
    assert np.array_equal(erow[flat % s.nnz], i) and np.array_equal(col[flat % s.nnz], j)
    # the gradient's way back: entry k reads [v_k, position_k]
    d = torch.arange(V * s.nnz, dtype=torch.float32).view(V, s.nnz)
    assert torch.equal(sets.to_input_order(d), d.view(-1)[sets.flat])
    # the same index tensors hit the cache; other values on them share the object
    assert G.sparse_sets_of(coo) is sets
    again = torch.sparse_coo_tensor(coo._indices(), coo._values() * 2, coo.shape, is_coalesced=True)
    assert G.sparse_sets_of(again) is sets


def test_batched_csr_on_the_union_pattern_is_read_in_place():
    adj, _ = _fixture_coo()
    V, N = adj.shape[0], adj.shape[1]
    ur, uc = np.nonzero((adj != 0).any(0))
    crow = np.concatenate([[0], np.cumsum(np.bincount(ur, minlength=N))])
    vals = torch.from_numpy(np.ascontiguousarray(adj[:, ur, uc]))            # explicit zeros where a sample lacks an edge
    csr = torch.sparse_csr_tensor(torch.from_numpy(crow).repeat(V, 1), torch.from_numpy(uc).repeat(V, 1), vals, (V, N, N))
    sets = G.sparse_sets_of(csr)
    assert sets.flat is None and sets.structure.nnz == len(ur)
    g = G.graph_for(csr, 3, 1)
    assert g.val == csr.values().data_ptr() and g.n_sets == V
    # the same union as the COO form: one structure for both
    assert sets.structure is G.sparse_sets_of(_fixture_coo()[1]).structure
    # samples with their own rows: csr with different columns per sample goes through the map
    own = torch.sparse_csr_tensor(torch.tensor([[0, 1, 2], [0, 1, 2]]), torch.tensor([[0, 1], [1, 0]]),
                                  torch.tensor([[1., 2.], [3., 4.]]), (2, 2, 2))
    so = G.sparse_sets_of(own)
    assert so.structure.nnz == 4 and so.flat.tolist() == [0, 3, 5, 6]
    assert torch.equal(so.graph(own.values()).dense(), own.to_dense())


def test_edge_adjacency_with_per_sample_weights():
    crow, col = torch.tensor([0, 2, 3, 3, 4]), torch.tensor([0, 2, 1, 3])
    w = torch.arange(12.).view(3, 4).requires_grad_(True)
    a = ops.edge_adjacency(crow, col, w)
    assert tuple(a.shape) == (3, 4, 4) and G.is_sparse_adjacency(a)
    dense = torch.zeros(3, 4, 4)
    dense[:, [0, 0, 1, 3], [0, 2, 1, 3]] = w.detach()
    assert torch.equal(a.to_dense(), dense)
    g = G.graph_for(a, 6, 2)                                          # V = Bg = 3, shared by 2 relations
    assert g.val == w.data_ptr() and g.n_sets == 3                    # read in place
    # columns reversed inside a row: gathered into library order
    col_r = torch.tensor([2, 0, 1, 3])
    wr = w.detach()[:, [1, 0, 2, 3]].contiguous()
    gr = G.graph_for(ops.edge_adjacency(crow, col_r, wr), 3, 1)
    assert isinstance(gr.val, torch.Tensor) and torch.equal(gr.val, w.detach())
    # not contiguous: copied into the pattern's own buffer
    wide = torch.arange(24.).view(3, 8)
    gs = G.graph_for(ops.edge_adjacency(crow, col, wide[:, ::2]), 3, 1)
    assert isinstance(gs.val, torch.Tensor) and torch.equal(gs.val, wide[:, ::2])
    # the library is handed a bare pointer: values that do not cover every stored entry are refused
    for wrong in (torch.zeros(3, 3), torch.zeros(2, 4), torch.zeros(13)):
        with pytest.raises(ValueError, match="stores"):
            G.sparse_sets_of(a).graph(wrong)
    with pytest.raises(ValueError, match="stores 5 values"):
        G.sparse_sets_of(_fixture_coo()[1]).graph(torch.zeros(5))
    with pytest.raises(ValueError, match=r"weight must be \[nnz\] or \[V, nnz\]"):
        ops.edge_adjacency(crow, col, torch.zeros(1, 3, 4))


def test_errors_name_what_is_allowed():
    _, coo = _fixture_coo()                                            # V = 3
    with pytest.raises(ValueError, match=r"leading size in \[1, 2, 4\]"):
        G.graph_for(coo, 4, 2)
    assert G.graph_for(coo, 6, 2).n_sets == 3 and G.graph_for(coo, 3, 1).n_sets == 3
    hybrid = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.ones(2, 3), (2, 3, 3))     # a dense last dimension
    with pytest.raises(ValueError, match="hybrid"):
        G.graph_for(hybrid, 2, 1)
    with pytest.raises(TypeError, match="float32"):
        G.graph_for(coo.double(), 3, 1)
    twice = torch.sparse_csr_tensor(torch.tensor([[0, 2, 2]]), torch.tensor([[1, 1]]), torch.ones(1, 2), (1, 2, 2))
    with pytest.raises(ValueError, match="stored twice"):
        G.graph_for(twice, 1, 1)
    one = G.graph_for(torch.sparse_coo_tensor(torch.tensor([[0, 0], [0, 1], [1, 0]]), torch.ones(2), (1, 2, 2),
                                              is_coalesced=True), 4, 2)     # [1,N,N] is [N,N]: one set for every group
    assert one.n_sets == 1
