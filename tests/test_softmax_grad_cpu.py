"""CPU: the interface of a gradient at the dense softmax map (`weights="softmax_grad"`): the library's new entry points at
an ABI that stays 10, the form check, the unchanged keyword defaults, and the reference's fixtures
(tests/golden/make_golden_softmax_grad.py) against a float64 restatement of attention.py:33-36."""
import inspect
import os

import numpy as np
import pytest
import torch

import ms_gat_amd
from conftest import load_golden
from ms_gat_amd import _lib, ops
from ms_gat_amd.model import MSGAT

NEW = ("msgat_softmax_map_grad", "msgat_softmax_map_grad_workspace_bytes", "msgat_gacn_backward_map_grad")
ATTP = ["attp_gatt_b2c3n64.npz", "attp_gacn_b2c72n47.npz"]


def test_library_exports_the_map_gradient_at_abi_10():
    L = _lib.lib()
    assert L.msgat_abi_version() == 10 == _lib.ABI_VERSION
    for name in NEW:
        assert hasattr(L, name) and name in _lib.exported_symbols()


def test_header_declares_the_map_gradient():
    header = open(os.path.join(os.path.dirname(_lib.PKG), "include", "msgat_hip.h")).read()
    assert "size_t msgat_softmax_map_grad_workspace_bytes(" in header
    assert "int msgat_softmax_map_grad(" in header
    assert "int msgat_gacn_backward_map_grad(" in header
    assert "#define MSGAT_ABI_VERSION 10" in header


def test_form_check_and_defaults():
    assert ops._check_weights("softmax_grad") == "softmax_grad"
    assert ops._WEIGHT_FORMS[:2] == ("masked", "softmax")
    assert ops.collect_weights("softmax_grad").form == "softmax_grad"
    with pytest.raises(ValueError, match="'masked' or 'softmax'"):
        ops._check_weights("dense")
    for fn in (ops.gacn, ops.attention_core, ops.graph_attention, ms_gat_amd.GraphAttention.forward,
               ms_gat_amd.GACN.forward, ms_gat_amd.StackedGACN.forward):
        params = inspect.signature(fn).parameters
        assert params["need_weights"].default is False, fn
        assert params["weights"].default == "masked", fn
    assert inspect.signature(MSGAT.attention_maps).parameters["weights"].default == "masked"


def test_softmax_grad_under_grad_reaches_the_device_check():
    """Grad mode on, inputs that require grad: the form is accepted (no softmax refusal) and the CPU tensors are then
    refused by the device check."""
    x = torch.randn(2, 3, 8, 12, requires_grad=True)
    alpha, Wg, adj = torch.randn(3, requires_grad=True), torch.randn(12, 12, requires_grad=True), torch.eye(8)
    with pytest.raises(_lib.MsgatError):
        ops.gacn(x, alpha, Wg, None, adj, need_weights=True, weights="softmax_grad")
    with pytest.raises(_lib.MsgatError):
        ops.graph_attention(x, alpha, Wg, adj, need_weights=True, weights="softmax_grad")
    with pytest.raises(_lib.MsgatError):
        ops.attention_core(torch.randn(2, 4, 8, 12), torch.randn(2, 8, 12, requires_grad=True),
                           torch.randn(1, 12, 12, requires_grad=True), adj, need_weights=True, weights="softmax_grad")
    with pytest.raises(_lib.MsgatError):
        ms_gat_amd.GraphAttention(3, 12)(x, adj, need_weights=True, weights="softmax_grad")


def _fixture_inputs(g):
    if "x_q32" in g:
        return g["x_q32"].astype(np.float64) / 32, g["dy_q32"].astype(np.float64) / 32
    return g["x"].astype(np.float64), g["dy"].astype(np.float64)


@pytest.mark.parametrize("name", ATTP)
def test_map_gradient_fixtures_agree_with_dense_restatement(name):
    g = load_golden(name)
    x, dy = _fixture_inputs(g)
    W = g.get("W")
    t = {k: torch.from_numpy(g[k].astype(np.float64)).requires_grad_(True) for k in ("alpha", "Wg") + (("W",) if W is not None else ())}
    xt = torch.from_numpy(x).requires_grad_(True)
    at = torch.from_numpy(g["adj"].astype(np.float64))
    q = torch.einsum("c,bcnt->bnt", t["alpha"], xt)
    att = torch.softmax(q @ t["Wg"] @ q.transpose(1, 2), dim=-1)
    y = torch.einsum("bnm,bcmt->bcnt", att * at, xt)
    if W is not None:
        y = torch.einsum("oc,bcnt->bont", t["W"], y)
    dP = g["dP"].astype(np.float64)
    ((y * torch.from_numpy(dy)).sum() + (att * torch.from_numpy(dP)).sum()).backward()
    for key, got in (("att", att), ("y", y), ("dx", xt.grad), ("dalpha", t["alpha"].grad),
                     ("dWg", t["Wg"].grad)) + ((("dW", t["W"].grad),) if W is not None else ()):
        want = g[key].astype(np.float64)
        got = got.detach().numpy()
        assert np.abs(got - want).max() <= 1e-5 * max(np.abs(want).max(), 1e-30), (name, key)
    # dP is dense: it weighs the mass off the graph's structure too, and att is a row softmax
    assert np.count_nonzero(dP[:, g["adj"] == 0]) > 0
    assert np.allclose(g["att"].sum(-1), 1.0, atol=1e-5)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """The host checks of msgat_softmax_map_grad: both targets are required, Wg and dq_add must be 16-byte aligned, the
    workspace large enough and 256-byte aligned, T supported.  Nothing is enqueued, so made-up addresses are never read."""
    import ctypes as C
    L = _lib.lib()
    ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3, -4      # include/msgat_hip.h
    header = open(os.path.join(os.path.dirname(_lib.PKG), "include", "msgat_hip.h")).read()
    for name, value in (("NULL", ERR_NULL), ("SHAPE", ERR_SHAPE), ("UNSUPPORTED", ERR_UNSUPPORTED), ("WORKSPACE", ERR_WORKSPACE)):
        assert f"MSGAT_ERR_{name} = {value}," in header
    shape = _lib.Shape(2, 2, 3, 0, 47, 12)
    nbytes = int(L.msgat_softmax_map_grad_workspace_bytes(C.byref(shape)))
    assert nbytes >= 4 * (4 * 47 * 12 + 4 * 47 + 4 * 1 * 144) and nbytes % 256 == 0
    a = 0x10000                                                             # any 256-byte aligned address

    def call(sh=shape, Wg=a, dq=a, dWg=a, ws=a, wsb=nbytes):
        return L.msgat_softmax_map_grad(C.byref(sh), a, a, a, Wg, a, dq, dWg, ws, wsb, None)

    assert call(dq=None) == ERR_NULL and call(dWg=None) == ERR_NULL
    assert call(dq=a + 4) == ERR_SHAPE and call(Wg=a + 8) == ERR_SHAPE
    assert call(wsb=nbytes - 256) == ERR_WORKSPACE and call(ws=a + 16) == ERR_WORKSPACE
    assert call(sh=_lib.Shape(2, 2, 3, 0, 47, 5)) == ERR_UNSUPPORTED
    assert call(sh=_lib.Shape(1, 1, 1, 0, 46341, 12)) == ERR_UNSUPPORTED     # N * N >= 2^31
    io = _lib.Bwd()
    graph = _lib.Graph()
    assert L.msgat_gacn_backward_map_grad(C.byref(shape), C.byref(graph), C.byref(io), None, a, None) == ERR_NULL
    assert L.msgat_gacn_backward_map_grad(C.byref(shape), C.byref(graph), C.byref(io), a, None, None) == ERR_NULL
