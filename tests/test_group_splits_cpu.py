"""Host only: the workspace sizes of msgat_adjacency_grad and msgat_edge_weight_grad say how the groups are split over
blocks.  The tables of test_gpu_group_counts.py (tests/group_fixtures.py) are checked here without a device, so that a
change of the split constants shows on a machine without a GPU too."""
import ctypes as C

import pytest

import group_fixtures as F


@pytest.fixture(scope="module")
def L():
    from ms_gat_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _shape(G, V, Cu, N, T=12):
    from ms_gat_amd import _lib
    Bg = V if V > 1 else 1            # n_sets is 1, Bg or R*Bg
    return _lib.Shape(G // Bg, Bg, Cu, Cu, N, T)


@pytest.mark.parametrize("N,V,G,Cu,nsplit,per,why", F.ADJACENCY_GRAD_CASES,
                         ids=[f"N{c[0]}-V{c[1]}-G{c[2]}" for c in F.ADJACENCY_GRAD_CASES])
def test_adjacency_grad_split_table(L, N, V, G, Cu, nsplit, per, why):
    assert (G // V + per - 1) // per == nsplit, "the table itself: nsplit splits of `per` groups cover a set"
    nbytes = int(L.msgat_adjacency_grad_workspace_bytes(C.byref(_shape(G, V, Cu, N)), Cu, V))
    assert nbytes == (4 * V * nsplit * N * N if nsplit > 1 else 0), why


@pytest.mark.parametrize("N,E,G,Cu,nsplit,per,why", F.EDGE_WEIGHT_GRAD_CASES,
                         ids=[f"N{c[0]}-G{c[2]}" for c in F.EDGE_WEIGHT_GRAD_CASES])
def test_edge_weight_grad_split_table(L, N, E, G, Cu, nsplit, per, why):
    from ms_gat_amd import _lib
    assert (G + per - 1) // per == nsplit
    gr = _lib.Graph()                 # the size needs the counts only
    gr.n_nodes, gr.nnz = N, F.nnz_of(N, E)
    nbytes = int(L.msgat_edge_weight_grad_workspace_bytes(C.byref(_shape(G, 1, Cu, N)), C.byref(gr), Cu))
    assert nbytes == (4 * nsplit * gr.nnz if nsplit > 1 else 0), why
    # one value set goes the same way through the per-set entry point; more sets have one owner per (set, edge)
    assert int(L.msgat_edge_weight_grad_sets_workspace_bytes(C.byref(_shape(G, 1, Cu, N)), C.byref(gr), Cu, 1)) == nbytes


@pytest.mark.parametrize("R,Bg", [(4, 3), (5, 9), (9, 3)])
def test_per_set_edge_weight_grad_needs_no_workspace(L, R, Bg):
    from ms_gat_amd import _lib
    gr = _lib.Graph()
    gr.n_nodes, gr.nnz = 64, F.nnz_of(64, 70)
    sh = _lib.Shape(R, Bg, 3, 3, 64, 12)
    for n_sets in (Bg, R * Bg):
        assert int(L.msgat_edge_weight_grad_sets_workspace_bytes(C.byref(sh), C.byref(gr), 3, n_sets)) == 0
