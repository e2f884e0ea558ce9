"""CPU: the interface of reading the graph attention (`need_weights`): the library's new entry points, the ABI that stays
at 10, the keyword arguments of the ops and modules, and the refusal of a dense softmax map under autograd."""
import inspect

import pytest
import torch

import ms_gat_amd
from ms_gat_amd import _lib, ops
from ms_gat_amd.model import MSGAT

NEW = ("msgat_attention_map", "msgat_gacn_backward_edge_grad", "msgat_attention_backward_edge_grad",
       "msgat_edge_softmax_grad")


def test_library_exports_the_readout_entry_points_at_abi_10():
    L = _lib.lib()
    assert L.msgat_abi_version() == 10 == _lib.ABI_VERSION
    for name in NEW:
        assert hasattr(L, name) and name in _lib.exported_symbols()


def test_header_documents_the_new_entry_points():
    import os
    header = open(os.path.join(os.path.dirname(_lib.PKG), "include", "msgat_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header
    assert "#define MSGAT_ABI_VERSION 10" in header


def test_keyword_arguments():
    for fn in (ops.gacn, ops.attention_core, ops.graph_attention, ms_gat_amd.GraphAttention.forward,
               ms_gat_amd.GACN.forward, ms_gat_amd.StackedGACN.forward):
        params = inspect.signature(fn).parameters
        assert params["need_weights"].default is False, fn
        assert params["weights"].default == "masked", fn
    assert inspect.signature(MSGAT.attention_maps).parameters["weights"].default == "masked"


def test_softmax_weights_under_grad_raise():
    x = torch.randn(2, 3, 8, 12, requires_grad=True)
    alpha, Wg, adj = torch.randn(3), torch.randn(12, 12), torch.eye(8)
    with pytest.raises(ValueError, match="masked"):
        ops.gacn(x, alpha, Wg, None, adj, need_weights=True, weights="softmax")
    with pytest.raises(ValueError, match="no_grad"):
        ops.attention_core(torch.randn(2, 4, 8, 12), torch.randn(2, 8, 12), torch.randn(1, 12, 12, requires_grad=True),
                           adj, need_weights=True, weights="softmax")
    with pytest.raises(ValueError, match="'masked' or 'softmax'"):
        ops.gacn(x, alpha, Wg, None, adj, need_weights=True, weights="dense")


def test_softmax_weights_outside_grad_pass_the_check():
    """Under no_grad the check lets the call through to the device checks (no GPU here: the CPU tensor is refused)."""
    x = torch.randn(2, 3, 8, 12, requires_grad=True)
    with torch.no_grad(), pytest.raises(_lib.MsgatError):
        ops.gacn(x, torch.randn(3), torch.randn(12, 12), None, torch.eye(8), need_weights=True, weights="softmax")


def test_weight_indices_are_row_major_per_group():
    g = ms_gat_amd.SparseGraph(torch.tensor([[0., 1., 0.], [2., 0., 3.], [0., 0., 0.]]))
    idx = ops._weight_indices(g, torch.device("cpu"), (2, 2))
    assert idx.tolist() == [[0] * 6 + [1] * 6, [0, 0, 0, 1, 1, 1] * 2, [0, 1, 1] * 4, [1, 0, 2] * 4]
    w = torch.sparse_coo_tensor(idx, torch.arange(12.), (2, 2, 3, 3), is_coalesced=True)
    assert torch.equal(w.coalesce().indices(), idx)


# ---- the reference's fixtures (tests/golden/make_golden_attention.py) against a dense restatement --------------------

import numpy as np  # noqa: E402

from conftest import load_golden  # noqa: E402

ATTW = ["attw_gatt_b2c3n64.npz", "attw_gacn_b2c3n64.npz", "attw_gacn_b2c72n47.npz", "attw_gacn_b3c3n64_bnn.npz"]


def _fixture_inputs(g):
    if "x_q32" in g:
        return g["x_q32"].astype(np.float64) / 32, g["dy_q32"].astype(np.float64) / 32
    return g["x"].astype(np.float64), g["dy"].astype(np.float64)


@pytest.mark.parametrize("name", ATTW)
def test_attention_fixtures_agree_with_dense_restatement(name):
    g = load_golden(name)
    x, dy = _fixture_inputs(g)
    W = g.get("W")
    t = {k: torch.from_numpy(g[k].astype(np.float64)).requires_grad_(True) for k in ("alpha", "Wg") + (("W",) if W is not None else ())}
    xt = torch.from_numpy(x).requires_grad_(True)
    at = torch.from_numpy(g["adj"].astype(np.float64)).requires_grad_(True)
    q = torch.einsum("c,bcnt->bnt", t["alpha"], xt)
    att = torch.softmax(q @ t["Wg"] @ q.transpose(1, 2), dim=-1)
    M = att * at
    y = torch.einsum("bnm,bcmt->bcnt", M, xt)
    if W is not None:
        y = torch.einsum("oc,bcnt->bont", t["W"], y)
    ((y * torch.from_numpy(dy)).sum() + (M * torch.from_numpy(g["dM"].astype(np.float64))).sum()).backward()
    for key, got in (("att", att), ("M", M), ("y", y), ("dx", xt.grad), ("dadj", at.grad), ("dalpha", t["alpha"].grad),
                     ("dWg", t["Wg"].grad)) + ((("dW", t["W"].grad),) if W is not None else ()):
        want = g[key].astype(np.float64)
        got = got.detach().numpy()
        assert np.abs(got - want).max() <= 1e-5 * max(np.abs(want).max(), 1e-30), (name, key)
    # dM lives on the graph's structure only, and att is a row softmax
    mask = (g["adj"] != 0) if g["adj"].ndim == 2 else (g["adj"] != 0).any(axis=0)
    assert not np.any(g["dM"][:, ~mask])
    assert np.allclose(g["att"].sum(-1), 1.0, atol=1e-5)


def test_meam_attention_fixture_is_consistent():
    g = load_golden("attw_meam_72to72_n32.npz")
    att, M, adj = g["att"].astype(np.float64), g["M"].astype(np.float64), g["adj"].astype(np.float64)
    assert att.shape == M.shape == (2, 32, 32)
    assert np.allclose(att.sum(-1), 1.0, atol=1e-5)
    assert np.abs(M - att * adj).max() <= 1e-7
