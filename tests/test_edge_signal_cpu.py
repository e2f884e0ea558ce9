"""CPU: signal-dependent edge weights (`msgat_edge_signal_weights{,_backward}`, `MSGAT(learn_edge_weights="signal")`,
`model.EdgeSignalWeights`): the two entry points in the header, the ctypes table and the built library; their argument
checks, which launch nothing; and the parameters and state-dict keys of a "signal" model.  No device compute is called here.
"""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

NAMES = ("msgat_edge_signal_weights", "msgat_edge_signal_weights_backward")


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


def test_entry_points_are_declared_prototyped_and_exported_and_the_abi_version_is_still_10():
    from ms_gat_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in zip(NAMES, (7, 8)):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, f"{name} is not declared in include/msgat_hip.h"
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == n_args and args[0] == "const msgat_graph_t* graph" and args[-1] == "void* stream", args
        assert args[3:5] == ["int32_t B", "int32_t d"], args
        assert name in _lib.exported_symbols() and len(_lib._PROTOTYPES[name][1]) == n_args
        assert _lib._PROTOTYPES[name][1][0] is C.POINTER(_lib.Graph)
        assert hasattr(h, name), f"{name} is not exported by the library"
    assert "edge_signal.hip" in build.SOURCES
    assert "#define MSGAT_ABI_VERSION 10\n" in header and _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10


def _host_graph(nnz=9, n=5):
    """A host-side msgat_graph_t with dummy index pointers: nothing below dereferences them."""
    from ms_gat_amd import _lib
    g = _lib.Graph()
    g.n_nodes, g.nnz = n, nnz
    for name in ("rowptr", "col", "val", "erow", "colptr", "crow", "cperm", "cpos"):
        setattr(g, name, 1)
    return g


def test_argument_checks_launch_nothing():
    from ms_gat_amd import _lib
    L = _lib.lib()
    p = 1      # never dereferenced: every call below returns before a launch
    fwd, bwd = L.msgat_edge_signal_weights, L.msgat_edge_signal_weights_backward
    g = C.byref(_host_graph())
    assert fwd(None, p, p, 4, 8, p, None) == -1 and bwd(None, p, p, 4, 8, p, p, None) == -1      # no graph
    assert fwd(g, p, p, 4, 0, p, None) == -2 and bwd(g, p, p, 4, 0, p, p, None) == -2            # d = 0
    assert fwd(g, p, p, 4, -4, p, None) == -2 and fwd(g, p, p, -1, 8, p, None) == -2
    assert bwd(g, p, p, -1, 8, p, p, None) == -2
    for d in (6, 36):
        assert fwd(g, p, p, 4, d, p, None) == -3 and bwd(g, p, p, 4, d, p, p, None) == -3, d
    assert fwd(g, p, p, 0, 8, p, None) == 0 and bwd(g, p, p, 0, 8, p, p, None) == 0              # B = 0
    assert fwd(g, None, p, 4, 8, p, None) == -1 and fwd(g, p, None, 4, 8, p, None) == -1
    assert fwd(g, p, p, 4, 8, None, None) == -1
    assert bwd(g, None, p, 4, 8, p, p, None) == -1 and bwd(g, p, None, 4, 8, p, p, None) == -1
    assert bwd(g, p, p, 4, 8, None, None, None) == 0                                             # no output asked for
    empty = C.byref(_host_graph(nnz=0))
    assert fwd(empty, p, p, 4, 8, p, None) == 0                                                  # no edge: nothing to write
    assert bwd(empty, p, p, 4, 8, p, None, None) == 0                                            # dbase of no edge


def test_op_refuses_cpu_tensors():
    from ms_gat_amd import _lib, ops
    crow, col = torch.tensor([0, 1, 2, 3]), torch.tensor([1, 2, 0])
    with pytest.raises(_lib.MsgatError, match="no CPU path"):
        ops.edge_signal_weights(torch.zeros(3), torch.zeros(2, 3, 16), crow, col)


def _models(n=32, edges=40):
    import ms_gat_amd
    from ms_gat_amd import model
    adj = ms_gat_amd.synthetic_adjacency(n, edges, seed=5)
    make = lambda learn, **kw: model.msgat48(n_components=3, in_channels=1, in_timesteps=12, out_timesteps=12,  # noqa: E731
                                             use_te=True, adj=adj, learn_edge_weights=learn, **kw)
    return adj, make


def test_signal_model_parameters_and_keys():
    adj, make = _models()
    torch.manual_seed(0)
    static = make(True)
    torch.manual_seed(0)
    signal = make("signal")
    state = signal.state_dict()
    assert set(state) == set(static.state_dict()) | {"edge_proj.weight"}
    assert tuple(state["edge_proj.weight"].shape) == (16, 12) and signal.edge_proj.weight.requires_grad   # [2 * 8, C * T_in]
    assert torch.count_nonzero(signal.edge_proj.weight[8:]) == 0             # the column side: a fresh model is the static one
    assert torch.count_nonzero(signal.edge_proj.weight[:8]) == 8 * 12        # the row side keeps its Xavier values
    assert torch.equal(signal.edge_weight.detach(), adj[adj != 0])           # re-copied after reset_parameters
    assert torch.equal(signal.edge_crow, static.edge_crow) and torch.equal(signal.edge_col, static.edge_col)
    assert signal.learn_edge_weights == "signal" and signal.edge_rank == 8
    assert tuple(make("signal", edge_rank=4).state_dict()["edge_proj.weight"].shape) == (8, 12)
    # a True model's checkpoint continues from the same function: everything but the projection is taken over
    with torch.no_grad():
        for p in static.parameters():
            if p.requires_grad:
                p.add_(0.125)
    result = signal.load_state_dict(static.state_dict(), strict=False)
    assert result.missing_keys == ["edge_proj.weight"] and not result.unexpected_keys
    for key, value in static.state_dict().items():
        assert torch.equal(signal.state_dict()[key], value), key
    assert torch.count_nonzero(signal.edge_proj.weight[8:]) == 0


def test_edge_features_layout():
    from ms_gat_amd import model
    X = torch.arange(2 * 3 * 2 * 5 * 4, dtype=torch.float32).reshape(2, 3, 2, 5, 4)      # [B,R,C,N,T]
    f = model.MSGAT.edge_features(X)
    assert tuple(f.shape) == (2, 5, 8)
    for b, n, c, t in ((0, 0, 0, 0), (1, 4, 1, 3), (1, 2, 0, 3), (0, 3, 1, 1)):
        assert f[b, n, c * 4 + t] == X[b, 0, c, n, t]


def test_adjacency_needs_the_inputs_and_the_rank_is_checked():
    adj, make = _models()
    with pytest.raises(ValueError, match="X"):
        make("signal").adjacency()
    with pytest.raises(ValueError, match="X"):
        make("signal").adjacency(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
    for bad in (6, 0, 36, -8, 8.0):
        with pytest.raises(ValueError, match="rank"):
            make("signal", edge_rank=bad)


def test_other_values_of_the_option_behave_as_before():
    adj, make = _models()
    for bad in ("hourly", "Time", "Signal", 1, None):
        with pytest.raises(ValueError, match="learn_edge_weights"):
            make(bad)
    frozen = make(False)
    assert not any(k.startswith("edge_") for k in frozen.state_dict()) and frozen.adjacency() is frozen.adj
    static = make(True)
    assert {k for k in static.state_dict() if k.startswith("edge_")} == {"edge_crow", "edge_col", "edge_weight"}
    timed = make("time")
    assert {k for k in timed.state_dict() if k.startswith("edge_")} == {"edge_crow", "edge_col", "edge_weight",
                                                                        "edge_h_ebd.weight", "edge_d_ebd.weight"}
    with pytest.raises(ValueError, match="H and D"):
        timed.adjacency()


def test_edge_signal_weights_module():
    from ms_gat_amd import model
    adj, _ = _models()
    csr = adj.to_sparse_csr()
    crow, col, val = csr.crow_indices(), csr.col_indices(), csr.values()
    m = model.EdgeSignalWeights(crow, col, val, in_features=12)
    assert set(m.state_dict()) == {"crow", "col", "weight", "proj.weight"}
    assert torch.equal(m.weight.detach(), val) and m.weight.requires_grad
    assert tuple(m.proj.weight.shape) == (16, 12) and m.proj.bias is None
    assert torch.count_nonzero(m.proj.weight[8:]) == 0 and torch.count_nonzero(m.proj.weight[:8]) == 8 * 12
    assert tuple(model.EdgeSignalWeights(crow, col, val, in_features=5, rank=32).proj.weight.shape) == (64, 5)
    with pytest.raises(ValueError, match="EdgeSignalWeights"):
        model.EdgeSignalWeights(crow, col[:-1], val, in_features=12)
    with pytest.raises(ValueError, match="rank"):
        model.EdgeSignalWeights(crow, col, val, in_features=12, rank=6)
    for bad in (torch.zeros(2, 32, 11), torch.zeros(2, 31, 12), torch.zeros(32, 12)):
        with pytest.raises(ValueError, match="EdgeSignalWeights"):
            m.weights(bad)
