"""CPU: a graph structure from the indices of a sparse adjacency (msgat_graph_build_indices) and the argument checks of
msgat_edge_weight_grad, the gradient of a sparse adjacency's stored values."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ms_gat_amd import _lib
from ms_gat_amd.graph import SparseGraph


def _random_pattern(n, density, seed, empty_rows=()):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < density            # asymmetric
    mask[list(empty_rows)] = False
    return mask


def _csr(mask):
    rows, cols = np.nonzero(mask)
    rowptr = np.zeros(mask.shape[0] + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return torch.from_numpy(np.cumsum(rowptr)), torch.from_numpy(cols.astype(np.int64))


_ARRAYS = ("rowptr", "col", "erow", "colptr", "crow", "cperm", "cpos")


@pytest.mark.parametrize("n,density,seed", [(37, 0.15, 0), (100, 0.05, 1), (130, 0.02, 2)])
def test_indices_build_equals_dense_build(n, density, seed):
    mask = _random_pattern(n, density, seed, empty_rows=(0, n // 2, n - 1))
    dense = torch.from_numpy(np.where(mask, np.random.default_rng(seed).uniform(0.5, 1.5, mask.shape), 0.0)).float()
    a = SparseGraph(dense, sell="always")
    rowptr, col = _csr(mask)
    b = SparseGraph.from_indices(rowptr, col, n, sell="always")
    assert a.nnz == b.nnz == int(mask.sum())
    for name in _ARRAYS:
        assert torch.equal(getattr(a, name)[: a.nnz if name not in ("rowptr", "colptr") else None],
                           getattr(b, name)[: b.nnz if name not in ("rowptr", "colptr") else None]), name
    assert torch.equal(b.order[: b.nnz], torch.arange(b.nnz, dtype=torch.int32))
    for form in ("sell_rows", "sell_cols"):
        for key, va in a._sell[form].items():
            vb = b._sell[form][key]
            assert (torch.equal(va, vb) if torch.is_tensor(va) else va == vb), (form, key)
    b.validate()


def test_explicit_zero_edges_are_kept_and_columns_sorted():
    # row 0 stores columns 3, 1 (unsorted) with a 0 weight at (0, 1); row 1 is empty; row 2 stores (2, 0)
    rowptr = torch.tensor([0, 2, 2, 3, 3])
    col = torch.tensor([3, 1, 0])
    g = SparseGraph.from_indices(rowptr, col, 4)
    assert g.nnz == 3
    assert g.col[:3].tolist() == [1, 3, 0] and g.erow[:3].tolist() == [0, 0, 2]
    assert g.order[:3].tolist() == [1, 0, 2]        # library edge k <- input position
    g.validate()


def test_large_graph_builds_without_dense_matrix():
    n = 200_000
    rng = np.random.default_rng(3)
    deg = rng.integers(0, 6, n)
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(deg)]))
    col = torch.from_numpy(rng.integers(0, n, int(deg.sum())))
    # drop duplicate columns inside a row: one edge per (row, column)
    rows = np.repeat(np.arange(n), deg)
    keys = np.unique(rows.astype(np.int64) * n + col.numpy())
    r, c = keys // n, keys % n
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]))
    g = SparseGraph.from_indices(rowptr, torch.from_numpy(c), n, sell="never")   # [N,N] floats would be 160 GB
    assert g.nnz == len(keys)
    assert torch.equal(g.col[: g.nnz], torch.from_numpy(c.astype(np.int32)))
    g.validate()


def _build_status(rowptr, col, n):
    L = _lib.lib()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(col, dtype=np.int32)
    nnz = len(ci)
    m = max(nnz, 1)
    outs = [np.zeros(n + 1, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(n + 1, np.int32)] + \
        [np.zeros(m, np.int32) for _ in range(4)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return L.msgat_graph_build_indices(p(rp), p(ci), n, nnz, *[p(o) for o in outs])


def test_bad_indices_are_status_codes():
    assert _build_status([0, 1, 2], [0, 1], 2) == 0
    assert _build_status([0, 1, 2], [0, 2], 2) == -5       # column out of range
    assert _build_status([0, 1, 2], [0, -1], 2) == -5
    assert _build_status([0, 2, 2], [1, 1], 2) == -5       # a column stored twice in a row
    assert _build_status([0, 2, 1], [0, 1], 2) == -5       # decreasing row pointer
    assert _build_status([1, 1, 2], [0, 1], 2) == -5       # rowptr[0] != 0
    assert _build_status([0, 1, 2], [0, 1], 0) == -2       # n <= 0
    with pytest.raises(_lib.MsgatError):
        SparseGraph.from_indices(torch.tensor([0, 2, 2]), torch.tensor([1, 1]), 2)


def test_edge_weight_grad_argument_checks_launch_nothing():
    L = _lib.lib()
    g = SparseGraph.from_indices(torch.tensor([0, 2, 3, 3]), torch.tensor([0, 2, 1]), 3)
    hs = g.host_struct()
    sh = _lib.Shape(1, 2, 3, 0, 3, 12)
    fake = 16   # never dereferenced: every call below must fail its checks before any launch
    ok_args = lambda: [C.byref(sh), C.byref(hs), 3, fake, 0, fake, fake, fake, fake, fake, None, 0, None]  # noqa: E731

    def call(**kw):
        a = ok_args()
        names = ["shape", "graph", "Cu", "dv", "dv_gc", "feat", "q", "kW", "lse", "dval", "ws", "ws_bytes", "stream"]
        for k, v in kw.items():
            a[names.index(k)] = v
        return L.msgat_edge_weight_grad(*a)

    assert call(shape=None) == -1
    assert call(graph=None) == -1
    assert call(Cu=0) == -2
    assert call(Cu=257) == -3
    assert call(dv_gc=2) == -2               # a slice of fewer channels than Cu
    assert call(dv_gc=-1) == -2
    for name in ("dv", "feat", "q", "kW", "lse", "dval"):
        assert call(**{name: None}) == -1, name
    bad_t = _lib.Shape(1, 2, 3, 0, 3, 10)
    assert call(shape=C.byref(bad_t)) == -3
    other_n = _lib.Shape(1, 2, 3, 0, 4, 12)
    assert call(shape=C.byref(other_n)) == -2   # graph of 3 nodes, signals of 4
    assert L.msgat_edge_weight_grad_workspace_bytes(C.byref(other_n), C.byref(hs), 3) == 0
    # the workspace: split partial sums of one group split over blocks (G = 2, 3 edges: 2 splits)
    need = L.msgat_edge_weight_grad_workspace_bytes(C.byref(sh), C.byref(hs), 3)
    assert need == 4 * 2 * 3
    assert call(ws=None, ws_bytes=need) == -1
    assert call(ws=fake, ws_bytes=need - 1) == -4


def test_edge_weight_grad_symbols_declared_and_exported():
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "msgat_hip.h")).read()
    for name in ("msgat_edge_weight_grad", "msgat_edge_weight_grad_workspace_bytes", "msgat_graph_build_indices"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib._PROTOTYPES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().msgat_abi_version() == 10
