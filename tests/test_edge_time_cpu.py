"""CPU: hour- and day-dependent edge weights (`msgat_edge_time_weights{,_backward}`, `MSGAT(learn_edge_weights="time")`):
the two entry points in the header, the ctypes table and the built library; their argument checks, which launch nothing;
and the parameters and state-dict keys of a "time" model.  No device compute is called here.
"""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

NAMES = ("msgat_edge_time_weights", "msgat_edge_time_weights_backward")


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


def test_entry_points_are_declared_prototyped_and_exported_and_the_abi_version_is_still_10():
    from ms_gat_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, f"{name} is not declared in include/msgat_hip.h"
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == 11 and args[-1] == "void* stream", args
        assert [a.rsplit(" ", 1)[0] for a in args[6:10]] == ["int32_t", "int64_t", "int32_t", "int32_t"]   # B, nnz, nh, nd
        assert name in _lib.exported_symbols() and len(_lib._PROTOTYPES[name][1]) == 11
        assert _lib._PROTOTYPES[name][1][7] is C.c_int64
        assert hasattr(h, name), f"{name} is not exported by the library"
    assert "edge_time.hip" in build.SOURCES
    assert "#define MSGAT_ABI_VERSION 10\n" in header and _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10


def test_argument_checks_launch_nothing():
    from ms_gat_amd import _lib
    L = _lib.lib()
    p = 1      # never dereferenced: every call below returns before a launch
    fwd, bwd = L.msgat_edge_time_weights, L.msgat_edge_time_weights_backward
    assert fwd(p, p, p, p, p, p, 4, 0, 24, 7, None) == 0 and fwd(p, p, p, p, p, p, 0, 9, 24, 7, None) == 0
    assert bwd(p, p, p, p, p, p, 4, 0, 24, 7, None) == 0
    assert bwd(p, p, p, None, None, None, 4, 9, 24, 7, None) == 0          # no output asked for
    for bad in ((-1, 9, 24, 7), (4, -1, 24, 7), (4, 9, -1, 7), (4, 9, 24, -1)):
        assert fwd(p, p, p, p, p, p, *bad, None) == -2, bad
        assert bwd(p, p, p, p, p, p, *bad, None) == -2, bad
    assert fwd(None, p, p, p, p, p, 4, 9, 24, 7, None) == -1
    assert fwd(p, p, p, p, p, None, 4, 9, 24, 7, None) == -1
    assert fwd(p, p, p, p, None, p, 4, 9, 24, 7, None) == -2               # d_w without D
    assert fwd(p, p, None, p, p, p, 4, 9, 24, 7, None) == -2               # D without d_w
    assert fwd(p, p, p, p, p, p, 4, 9, 0, 7, None) == -2                   # an empty hour table cannot be read
    assert bwd(None, p, p, p, p, p, 4, 9, 24, 7, None) == -1
    assert bwd(p, None, p, p, p, p, 4, 9, 24, 7, None) == -1               # dh_w without H
    assert bwd(p, p, None, p, p, p, 4, 9, 24, 7, None) == -1               # dd_w without D


def test_op_refuses_cpu_tensors_and_mismatched_operands():
    from ms_gat_amd import _lib, ops
    base, h, d = torch.zeros(5), torch.zeros(24, 5), torch.zeros(7, 5)
    H = D = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.MsgatError, match="no CPU path"):
        ops.edge_time_weights(base, h, d, H, D)


def _models(n=32, edges=40):
    import ms_gat_amd
    from ms_gat_amd import model
    adj = ms_gat_amd.synthetic_adjacency(n, edges, seed=5)
    make = lambda learn: model.msgat48(n_components=3, in_channels=1, in_timesteps=12, out_timesteps=12, use_te=True,  # noqa: E731
                                       adj=adj, learn_edge_weights=learn)
    return adj, make


def test_time_model_parameters_and_keys():
    adj, make = _models()
    torch.manual_seed(0)
    static = make(True)
    torch.manual_seed(0)
    timed = make("time")
    nnz = int((adj != 0).sum())
    tables = {"edge_h_ebd.weight": (24, nnz), "edge_d_ebd.weight": (7, nnz)}
    state = timed.state_dict()
    assert set(state) == set(static.state_dict()) | set(tables)
    for key, shape in tables.items():
        assert tuple(state[key].shape) == shape and torch.count_nonzero(state[key]) == 0, key
        assert timed.get_parameter(key).requires_grad
    assert torch.equal(timed.edge_weight.detach(), adj[adj != 0])          # re-copied after reset_parameters
    assert torch.equal(timed.edge_crow, static.edge_crow) and torch.equal(timed.edge_col, static.edge_col)
    assert timed.learn_edge_weights == "time" and static.learn_edge_weights is True
    # a True model's checkpoint continues from the same function: everything but the (zero) tables is taken over
    with torch.no_grad():
        for p in static.parameters():
            if p.requires_grad:
                p.add_(0.125)
    result = timed.load_state_dict(static.state_dict(), strict=False)
    assert sorted(result.missing_keys) == sorted(tables) and not result.unexpected_keys
    for key, value in static.state_dict().items():
        assert torch.equal(timed.state_dict()[key], value), key
    assert all(torch.count_nonzero(timed.state_dict()[k]) == 0 for k in tables)
    # reset_parameters alone leaves Xavier values in the tables; the constructor zeroes them after it
    timed.reset_parameters()
    assert torch.count_nonzero(timed.edge_h_ebd.weight) > 0


def test_other_values_of_the_option_are_refused_and_the_old_ones_are_unchanged():
    adj, make = _models()
    for bad in ("hourly", "Time", 1, None):
        with pytest.raises(ValueError, match="learn_edge_weights"):
            make(bad)
    frozen = make(False)
    assert not any(k.startswith("edge_") for k in frozen.state_dict()) and frozen.adjacency() is frozen.adj
    static = make(True)
    assert {k for k in static.state_dict() if k.startswith("edge_")} == {"edge_crow", "edge_col", "edge_weight"}
    with pytest.raises(ValueError, match="H and D"):
        make("time").adjacency()


def test_edge_time_embedding_module():
    from ms_gat_amd import model
    adj, _ = _models()
    csr = adj.to_sparse_csr()
    m = model.EdgeTimeEmbedding(csr.crow_indices(), csr.col_indices(), csr.values())
    assert set(m.state_dict()) == {"crow", "col", "weight", "h_ebd.weight", "d_ebd.weight"}
    assert torch.equal(m.weight.detach(), csr.values()) and m.weight.requires_grad
    assert tuple(m.h_ebd.weight.shape) == (24, csr.values().numel()) and tuple(m.d_ebd.weight.shape) == (7, csr.values().numel())
    assert torch.count_nonzero(m.h_ebd.weight) == 0 and torch.count_nonzero(m.d_ebd.weight) == 0
    with pytest.raises(ValueError, match="EdgeTimeEmbedding"):
        model.EdgeTimeEmbedding(csr.crow_indices(), csr.col_indices()[:-1], csr.values())
