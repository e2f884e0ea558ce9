"""CPU: the gradient of the adjacency (attention.py:36 with an adjacency that requires grad).

The reference's fixtures of tests/golden/make_golden_adjacency.py against float64 autograd through the dense
restatement (this pins the oracle the GPU tests compare with at sizes the fixtures do not cover), the ABI version, and
the argument checks of `msgat_adjacency_grad`, none of which launches anything.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import dense_torch

from ms_gat_amd import _lib

GACN_FIXTURES = ["adjgrad_gacn_b2c3n64.npz", "adjgrad_gacn_b2c72n47.npz", "adjgrad_gacn_b3c3n64_bnn.npz"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _inputs(g):
    if "x_q32" in g:
        return g["x_q32"].astype(np.float32) / 32, g["dz_q32"].astype(np.float32) / 32
    return g["x"].astype(np.float32), g["dz"].astype(np.float32)


def test_fixture_adjacencies_are_asymmetric_with_zeros_and_an_empty_row():
    for name in ["adjgrad_gatt_b2c3n64.npz", "adjgrad_meam_72to72_n32.npz"] + GACN_FIXTURES:
        g = load_golden(name)
        adj, dadj = g["adj"], g["dadj"]
        assert adj.shape == dadj.shape, name
        a = adj if adj.ndim == 3 else adj[None]
        assert (a == 0).any() and not np.array_equal(a, a.transpose(0, 2, 1)), name
        assert (a[:, 5] == 0).all(), name
        # the gradient is dense: clearly non-zero where the adjacency is 0
        off = np.abs(dadj[(adj == 0)])
        assert np.mean(off > 1e-5 * np.abs(dadj).max()) > 0.9, name


def test_graph_attention_fixture_against_float64_oracle():
    g = load_golden("adjgrad_gatt_b2c3n64.npz")
    x, adj = _t(g["x"].astype(np.float32)), _t(g["adj"]).requires_grad_(True)
    y = dense_torch.graph_attention_dense(x, adj, _t(g["Wg"]), _t(g["alpha"]))
    y.backward(_t(g["dy"].astype(np.float32)))
    assert rel_err(y.detach(), g["y"]) < 5e-6
    assert rel_err(adj.grad, g["dadj"]) < 5e-6


@pytest.mark.parametrize("name", GACN_FIXTURES)
def test_gacn_fixtures_against_float64_oracle(name):
    g = load_golden(name)
    xn, dzn = _inputs(g)
    adj = _t(g["adj"]).requires_grad_(True)
    z = dense_torch.gacn_dense(_t(xn), adj, _t(g["Wg"]), _t(g["alpha"]), _t(g["W"]))
    z.backward(_t(dzn))
    assert rel_err(z.detach(), g["z"]) < 5e-6, name
    assert rel_err(adj.grad, g["dadj"]) < 5e-6, name


def test_meam_fixture_against_float64_oracle():
    g = load_golden("adjgrad_meam_72to72_n32.npz")
    p = {k[2:]: _t(v) for k, v in g.items() if k.startswith("p.")}
    adj = _t(g["adj"]).requires_grad_(True)
    out = dense_torch.meam_dense(_t(g["x"].astype(np.float32)), adj, p, [1, 2])
    out.backward(_t(g["dout"].astype(np.float32)))
    assert rel_err(out.detach(), g["out"]) < 5e-6
    assert rel_err(adj.grad, g["dadj"]) < 5e-5


def test_abi_version_is_10():
    assert _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10


def test_adjacency_grad_argument_checks_launch_nothing():
    L = _lib.lib()
    sh = _lib.Shape(2, 3, 72, 24, 47, 12)       # R = 2, Bg = 3: G = 6; GACN 72 -> 24
    p = C.c_void_p(16)                           # never dereferenced: every call below fails its checks on the host
    ws_need = int(L.msgat_adjacency_grad_workspace_bytes(C.byref(sh), 24, 1))
    assert ws_need > 0                           # one [N,N] summed over 6 groups: split over blocks, partials in the workspace

    def call(shape=sh, Cu=24, dv=p, gc=0, feat=p, q=p, kW=p, lse=p, n_sets=1, dadj=p, ws=p, nbytes=ws_need):
        return L.msgat_adjacency_grad(shape if shape is None else C.byref(shape), Cu, dv, gc, feat, q, kW, lse, n_sets,
                                      dadj, ws, nbytes, None)

    assert call(shape=None) == -1                                 # MSGAT_ERR_NULL
    for kw in ("dv", "feat", "q", "kW", "lse", "dadj", "ws"):
        assert call(**{kw: None}) == -1, kw                       # MSGAT_ERR_NULL
    for n_sets in (0, 2, 4, 5, 7):
        assert call(n_sets=n_sets) == -2, n_sets                  # MSGAT_ERR_SHAPE: not in {1, Bg = 3, R*Bg = 6}
    assert call(Cu=0) == -2
    assert call(gc=12) == -2                                      # a channel slice narrower than Cu
    assert call(Cu=257) == -3                                     # MSGAT_ERR_UNSUPPORTED: Cu > 256
    for T in (3, 6, 20):
        assert call(shape=_lib.Shape(2, 3, 72, 24, 47, T)) == -3, T
    assert call(nbytes=ws_need - 1) == -4                         # MSGAT_ERR_WORKSPACE
    # the query answers 0 for what the call refuses
    assert L.msgat_adjacency_grad_workspace_bytes(C.byref(sh), 24, 4) == 0
    assert L.msgat_adjacency_grad_workspace_bytes(C.byref(sh), 0, 1) == 0
