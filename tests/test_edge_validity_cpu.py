"""CPU: validity-gated edges (`msgat_edge_validity{,_backward}`, `ops.edge_validity`, `model.EdgeValidity`,
`MSGAT(missing_edges=...)`).  The two entry points in the header, the ctypes table and the built library; their argument
checks, which launch nothing; the tables of every mode; the refusals; the options, buffers and state-dict keys of the models;
the torch restatement the op runs for CPU tensors, alone, inside a tiny CPU `MSGAT` and on a synthetic series with outages.
No device compute is called here.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import edge_validity_ref as ref

NAMES = {"msgat_edge_validity": 11, "msgat_edge_validity_backward": 11}


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


# ---- the library -----------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_prototyped_and_exported_and_the_abi_version_is_still_10():
    import ms_gat_amd
    from ms_gat_amd import _lib, build, model
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, f"{name} is not declared in include/msgat_hip.h"
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == n_args and args[-1] == "void* stream" and args[0] == "const msgat_graph_t* graph", args
        assert [a.rsplit(" ", 1)[0] for a in args[4:10]] == ["int64_t", "const float*", "float*", "int32_t", "int32_t", "int32_t"]
        assert name in _lib.exported_symbols() and len(_lib._PROTOTYPES[name][1]) == n_args
        assert _lib._PROTOTYPES[name][1][0] is C.POINTER(_lib.Graph)
        assert _lib._PROTOTYPES[name][1][4:6] == [C.c_int64, _lib.c_float_p]
        assert _lib._PROTOTYPES[name][1][7:10] == [C.c_int32] * 3
        assert hasattr(h, name), f"{name} is not exported by the library"
    assert "msgat_edge_validity{,_backward}" in header.split("#define MSGAT_ABI_VERSION")[0]     # in the version's history
    assert "edge_validity.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "edge_validity.hip"))
    assert "#define MSGAT_ABI_VERSION 10\n" in header and _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10
    assert "EdgeValidity" in ms_gat_amd.__all__ and ms_gat_amd.EdgeValidity is model.EdgeValidity


def _graph(n=5, nnz=9, col=1):
    from ms_gat_amd import _lib
    g = _lib.Graph()
    g.n_nodes, g.nnz, g.col = n, nnz, col        # col: never dereferenced, every call below returns before a launch
    return g


def test_argument_checks_launch_nothing():
    from ms_gat_amd import _lib
    L = _lib.lib()
    p = 1      # never dereferenced
    table = (C.c_float * 17)(*([0.0] * 16 + [1.0]))
    fwd, bwd = L.msgat_edge_validity, L.msgat_edge_validity_backward
    g = C.byref(_graph())
    for fn in (fwd, bwd):
        # empty sizes: OK, nothing launched
        assert fn(g, p, p, p, 60, table, p, 0, 12, 0, None) == 0
        assert fn(C.byref(_graph(nnz=0)), p, p, p, 60, table, p, 4, 12, 1, None) == 0
        assert fn(C.byref(_graph(nnz=0)), None, None, None, 60, None, None, 4, 12, 1, None) == 0
        # negative sizes
        assert fn(g, p, p, p, 60, table, p, -1, 12, 0, None) == -2
        assert fn(g, p, p, p, -4, table, p, 4, 12, 0, None) == -2
        assert fn(g, p, p, p, 60, table, p, 4, -12, 0, None) == -2
        assert fn(C.byref(_graph(nnz=-1)), p, p, p, 60, table, p, 4, 12, 0, None) == -2
        assert fn(C.byref(_graph(n=-1)), p, p, p, 60, table, p, 4, 12, 0, None) == -2
        # T outside the package's T_in set, with and without work to do
        for T in (5, 0, 1, 3, 20, 24):
            assert fn(g, p, p, p, 60, table, p, 4, T, 0, None) == -3, T
        assert fn(g, p, p, p, 60, table, p, 0, 5, 0, None) == -3
        for T in ref.T_SET:
            assert fn(g, p, p, p, 60, table, p, 0, T, 0, None) == 0, T
        # no graph
        assert fn(None, p, p, p, 60, table, p, 4, 12, 0, None) == -1
        assert fn(C.byref(_graph(col=None)), p, p, p, 60, table, p, 4, 12, 0, None) == -1
    for missing in (1, 3, 5, 6):                 # w, val, table, out; exempt (2) is optional
        args = [g, p, p, p, 60, table, p]
        args[missing] = None
        assert fwd(*args, 4, 12, 0, None) == -1, missing
    for missing in (1, 3, 5):                    # dout, val, table
        args = [g, p, p, p, 60, table, p]
        args[missing] = None
        assert bwd(*args, 4, 12, 0, None) == -1, missing
    assert bwd(g, p, p, p, 60, table, None, 4, 12, 0, None) == 0            # no output asked for
    assert bwd(g, p, p, p, 60, table, None, 4, 12, 1, None) == 0


def test_status_codes_are_the_headers():
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    for name, value in (("MSGAT_ERR_NULL", -1), ("MSGAT_ERR_SHAPE", -2), ("MSGAT_ERR_UNSUPPORTED", -3)):
        assert re.search(r"%s\s*=?\s*\(?%d\)?" % (name, value), header), name


# ---- the tables ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", ref.T_SET)
def test_tables_of_every_mode(T):
    from ms_gat_amd import ops
    for mode in ["scale", "drop"] + list(range(1, T + 1)):
        got = ops.edge_validity_table(mode, T)
        assert len(got) == T + 1 and all(isinstance(x, float) for x in got)
        assert got[T] == 1.0, (mode, T)                                   # no missing reading: the weights as they were
        assert np.array_equal(np.asarray(got, np.float32), ref.table(mode, T)), (mode, T)
        assert all(np.float32(x) == x for x in got)                       # rounded to fp32 already
    scale = ops.edge_validity_table("scale", T)
    assert scale[0] == 0.0 and all(x == float(np.float32(c / T)) for c, x in enumerate(scale))
    assert ops.edge_validity_table("drop", T) == (0.0,) * T + (1.0,)
    assert ops.edge_validity_table(T, T) == ops.edge_validity_table("drop", T)
    assert ops.edge_validity_table(1, T) == (0.0,) + (1.0,) * T
    m = T // 2
    assert ops.edge_validity_table(m, T) == (0.0,) * m + (1.0,) * (T - m + 1)


def test_bad_modes_and_window_lengths_raise():
    from ms_gat_amd import model, ops
    for bad in ("Scale", "keep", 0, -1, 13, 1.0, 0.5, None, True, False, [1]):
        with pytest.raises(ValueError, match="edge_validity"):
            ops.edge_validity_table(bad, 12)
    for bad_T in (5, 0, 3, 24, 12.0, "12", True):
        with pytest.raises(ValueError, match="edge_validity"):
            ops.edge_validity_table("scale", bad_T)
    adj, make = _models()
    for bad in ("Scale", 0, 13, 0.5, True):
        with pytest.raises(ValueError, match="edge_validity"):
            make(False, missing_edges=bad)
    csr = adj.to_sparse_csr()
    for bad in ("Scale", 0, 0.5, True, None):
        with pytest.raises(ValueError, match="EdgeValidity"):
            model.EdgeValidity(csr.crow_indices(), csr.col_indices(), mode=bad)


def test_op_refuses_bad_operands():
    from ms_gat_amd import ops
    crow, col, N = ref.pattern(5)
    crow, col = torch.from_numpy(crow), torch.from_numpy(col)
    val = torch.ones(2, N, 12)
    w = torch.ones(5)
    assert ops.edge_validity(w, val, crow, col).shape == (2, 5)
    with pytest.raises(ValueError, match="edge_validity"):
        ops.edge_validity(torch.ones(4), val, crow, col)                     # another nnz
    with pytest.raises(ValueError, match="edge_validity"):
        ops.edge_validity(torch.ones(3, 5), val, crow, col)                  # another V
    with pytest.raises(ValueError, match="edge_validity"):
        ops.edge_validity(w, val, crow, col, samples=3)
    with pytest.raises(ValueError, match="edge_validity"):
        ops.edge_validity(w, torch.ones(2, N + 1, 12), crow, col)            # another N
    with pytest.raises(ValueError, match="edge_validity"):
        ops.edge_validity(w, torch.ones(2, N, 5), crow, col)                 # T outside the set
    with pytest.raises(ValueError, match="edge_validity"):
        ops.edge_validity(w, torch.ones(N, 12), crow, col)
    with pytest.raises(TypeError, match="edge_validity"):
        ops.edge_validity(w.double(), val, crow, col)
    with pytest.raises(TypeError, match="edge_validity"):
        ops.edge_validity(w, val.bool(), crow, col)
    for bad_exempt in (torch.zeros(4, dtype=torch.uint8), torch.zeros(5), torch.zeros(5, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match="edge_validity.*exempt"):
            ops.edge_validity(w, val, crow, col, exempt=bad_exempt)


# ---- the restatement in torch ops, which the op runs for CPU tensors ----------------------------------------------------

@pytest.mark.parametrize("T", ref.T_SET)
def test_torch_restatement_has_the_bits_of_the_numpy_one(T):
    from ms_gat_amd import ops
    V, nnz = 5, 257
    crow, col, N = ref.pattern(nnz, seed=T)
    val = ref.validity(V, N, T, seed=T)
    rng = np.random.default_rng(T)
    w2 = rng.standard_normal((V, nnz)).astype(np.float32)
    ex = ref.self_loops(crow, col) | (np.arange(nnz) % 3 == 0)
    t = torch.from_numpy
    for mode in ref.modes(T):
        for w in (w2[0], w2):
            for exempt in (None, ex):
                want = ref.forward(w, val, col, mode, exempt)
                for fn in (ops.edge_validity_reference, ops.edge_validity):
                    got = fn(t(w), t(val), t(crow), t(col), mode=mode, exempt=None if exempt is None else t(exempt))
                    assert got.shape == (V, nnz) and got.dtype == torch.float32
                    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), (mode, w.ndim, exempt is not None)
    # a NaN weight on a fully gated edge is +0, on an exempt one it stays
    w = w2[0].copy()
    w[:] = np.nan
    got = ops.edge_validity(t(w), t(val), t(crow), t(col), mode="drop", exempt=t(ex)).numpy()
    gated = (ref.gates(val, col, "drop") == 0) & ~ex[None, :]
    assert gated.any() and not got[gated].view(np.int32).any() and np.isnan(got[~gated]).all()
    # and its autograd is the two backward forms (the shared form up to torch's own summation order)
    dout = rng.standard_normal((V, nnz)).astype(np.float32)
    ws = t(w2).requires_grad_(True)
    (g,) = torch.autograd.grad(ops.edge_validity(ws, t(val), t(crow), t(col), exempt=t(ex)), ws, t(dout))
    assert np.array_equal(g.numpy(), ref.backward_sets(dout, val, col, "scale", ex))
    w1 = t(w2[0]).requires_grad_(True)
    (g,) = torch.autograd.grad(ops.edge_validity(w1, t(val), t(crow), t(col), exempt=t(ex)), w1, t(dout))
    np.testing.assert_allclose(g.numpy(), ref.backward_shared(dout, val, col, "scale", ex), rtol=1e-5, atol=1e-6)


def test_restatements_own_inputs_cover_what_they_claim():
    crow, col, N = ref.pattern(257)
    degree_in_col = np.bincount(col, minlength=N)
    rows = np.repeat(np.arange(N), np.diff(crow))
    assert degree_in_col[2] == 70 and int(ref.self_loops(crow, col).sum()) == 1
    assert degree_in_col[-2:].sum() == 0 and (np.diff(crow)[-2:] == 0).all()             # nodes without any edge
    assert all((np.diff(col[crow[r]:crow[r + 1]]) > 0).all() for r in range(N)) and len(rows) == 257
    for nnz in (1, 3, 4, 5, 255, 256, 1027):
        c, k, n = ref.pattern(nnz)
        assert len(k) == nnz and c[-1] == nnz and k.max() < n - 2
    val = ref.validity(5, N, 12)
    assert np.isnan(val).any() and (val == np.float32(0.49)).any() and (val == np.float32(0.51)).any() and (val == 0.5).any()
    assert set(np.unique(val[~np.isnan(val)])) <= {np.float32(x) for x in (0.0, 0.49, 0.5, 0.51, 1.0)}
    c = ref.counts(val)
    assert (c[:, 0] == 12).all() and (c[1:, 1] == 0).all() and (c[0] == 12).all() and len(np.unique(c)) > 6
    v = np.array([[[np.nan, 0.49, 0.5, 0.51]]], np.float32)
    assert ref.counts(v).tolist() == [[1]]


# ---- the models ------------------------------------------------------------------------------------------------------

LEARN = [False, True, "time", "signal"]


def _models(n=32, edges=40, in_channels=2):
    import ms_gat_amd
    from ms_gat_amd import model
    adj = ms_gat_amd.synthetic_adjacency(n, edges, seed=5)
    make = lambda learn, **kw: model.msgat48(n_components=3, in_channels=in_channels, in_timesteps=12,   # noqa: E731
                                             out_timesteps=12, use_te=True, adj=adj, learn_edge_weights=learn, **kw)
    return adj, make


@pytest.mark.parametrize("learn", LEARN)
def test_default_is_off_and_the_option_adds_no_state_dict_key(learn):
    adj, make = _models()
    plain = make(learn)
    assert plain.missing_edges is None
    reference_names = {"edge_crow", "edge_col"} if learn else set()
    assert {n for n, _ in plain.named_buffers() if n.startswith("edge_")} == reference_names
    if learn is False:
        assert not any(k.startswith("edge_") for k in plain.state_dict())
        assert plain.adjacency() is plain.adj
        assert plain.eval().adjacency() is plain.adj
    for mode in ("scale", "drop", 6):
        gated = make(learn, missing_edges=mode)
        assert gated.missing_edges == mode
        assert set(gated.state_dict()) == set(plain.state_dict())            # checkpoints interchange
        assert [n for n, _ in gated.named_parameters()] == [n for n, _ in plain.named_parameters()]
        gated.load_state_dict(plain.state_dict())
        plain.load_state_dict(gated.state_dict())
        names = {n for n, _ in gated.named_buffers() if n.startswith("edge_")} - reference_names
        want = {"edge_valid_exempt"} | ({"edge_valid_crow", "edge_valid_col", "edge_valid_index"} if not learn else set())
        assert names == want
        H = D = torch.zeros(4, dtype=torch.long)
        for net in (gated.train(), gated.eval()):                            # a function of the input: every mode needs X
            with pytest.raises(ValueError, match="missing_edges.*X"):
                net.adjacency(H, D)
            with pytest.raises(ValueError, match="missing_edges.*X"):
                net.adjacency()
    # the stored diagonal is exempt; keep_self=False exempts nothing
    csr = adj.to_sparse_csr()
    assert torch.equal(gated.edge_valid_exempt.bool(), torch.from_numpy(ref.self_loops(csr.crow_indices().numpy(),
                                                                                       csr.col_indices().numpy())))
    assert int(gated.edge_valid_exempt.sum()) > 0 and gated.edge_valid_exempt.dtype == torch.uint8
    assert make(learn, missing_edges="scale", missing_edges_keep_self=False).edge_valid_exempt is None
    if not learn:
        assert torch.equal(adj.reshape(-1)[gated.edge_valid_index], csr.values())
    # with edge dropout too, dropout's buffers keep their names
    both = make(learn, missing_edges="scale", edge_dropout=0.2)
    drop_names = {n for n, _ in both.named_buffers() if "drop" in n}
    assert drop_names == {"edge_drop_state", "edge_drop_exempt"} | ({"edge_drop_crow", "edge_drop_col", "edge_drop_index"}
                                                                    if not learn else set())


@pytest.mark.parametrize("learn", [False, True])
@pytest.mark.parametrize("keep_self", [True, False])
def test_cpu_model_takes_a_silent_sensor_out_of_the_graph_for_that_sample_only(learn, keep_self):
    adj, make = _models(n=12, edges=14)
    N, B, j, b = 12, 3, 4, 1
    assert int((adj[:, j] != 0).sum()) > 1 and adj[j, j] != 0                # j has neighbours and a stored diagonal
    net = make(learn, missing_edges="scale", missing_edges_keep_self=keep_self)
    plain = make(learn)
    plain.load_state_dict(net.state_dict())
    g = torch.Generator().manual_seed(0)
    X = torch.randn(B, 3, 2, N, 12, generator=g)
    X[:, :, -1] = 1.0
    H = D = torch.zeros(B, dtype=torch.long)
    for net_mode in (net.train(), net.eval()):
        whole = net_mode.adjacency(H, D, X)
        assert whole.layout == torch.sparse_csr and tuple(whole.shape) == (B, N, N)
        ungated = plain.adjacency(H, D, X)
        ungated = ungated if learn is False else ungated.to_dense()
        assert torch.equal(whole.to_dense(), ungated.expand(B, N, N))        # an all-valid batch: the weights themselves
        assert torch.equal(whole.values(), adj.to_sparse_csr().values().expand(B, -1))
        Xm = X.clone()
        Xm[b, 0, -1, j] = 0.0                                                # sensor j of sample b measured nothing
        Xm[b, 1:, -1, 7] = 0.0                                               # older components' windows do not count
        A = net_mode.batch_adjacency(Xm, H, D).to_dense()
        off = torch.ones(N, dtype=torch.bool)
        off[j] = False
        assert torch.count_nonzero(A[b, off, j]) == 0                        # column j: what j sends
        assert (A[b, j, j] == adj[j, j]) if keep_self else (A[b, j, j] == 0)
        keep = torch.ones(B, N, N, dtype=torch.bool)
        keep[b, :, j] = False
        assert torch.equal(A[keep], ungated.expand(B, N, N)[keep])           # and nothing else moved
    # half a window at "scale": half the weight; the thresholds keep or drop it
    Xh = X.clone()
    Xh[b, 0, -1, j, :6] = 0.0
    i = int((adj[:, j] != 0).nonzero()[0]) if int((adj[:, j] != 0).nonzero()[0]) != j else int((adj[:, j] != 0).nonzero()[1])
    assert net.adjacency(H, D, Xh).to_dense()[b, i, j] == adj[i, j] * 0.5
    assert make(learn, missing_edges=6).adjacency(H, D, Xh).to_dense()[b, i, j] == adj[i, j]
    assert make(learn, missing_edges=7).adjacency(H, D, Xh).to_dense()[b, i, j] == 0
    assert make(learn, missing_edges="drop").adjacency(H, D, Xh).to_dense()[b, i, j] == 0


def test_edge_validity_module():
    from ms_gat_amd import model
    crow, col, N = ref.pattern(257)
    m = model.EdgeValidity(torch.from_numpy(crow), torch.from_numpy(col), mode="drop")
    assert m.state_dict() == {} and list(m.parameters()) == []
    assert np.array_equal(m.exempt.numpy().astype(bool), ref.self_loops(crow, col)) and m.exempt.dtype == torch.uint8
    assert model.EdgeValidity(torch.from_numpy(crow), torch.from_numpy(col), keep_self=False).exempt is None
    val = ref.validity(4, N, 8)
    w = np.random.default_rng(0).standard_normal(257).astype(np.float32)
    for net in (m.train(), m.eval()):                                        # a function of the input, in either mode
        got = net(torch.from_numpy(w), torch.from_numpy(val))
        assert np.array_equal(got.numpy().view(np.int32), ref.forward(w, val, col, "drop", ref.self_loops(crow, col)).view(np.int32))


def test_dead_sensors_of_a_synthetic_series_send_nothing_in_any_sample():
    from ms_gat_amd import data, ops
    torch.manual_seed(0)
    ds = data.SyntheticPEMS(n_nodes=24, n_edges=30, n_channels=2, in_hours=[1, 2], batch_size=8, days=3, missing=0.05,
                            dead_sensors=2, input_null_value=0.0)
    assert ds.input_channels == 3
    dead = (ds.raw[0] == 0).all(-1).nonzero().flatten()
    assert dead.numel() == 2
    csr = ds.adj.to_sparse_csr()
    crow, col = csr.crow_indices(), csr.col_indices()
    rows = torch.repeat_interleave(torch.arange(24), crow[1:] - crow[:-1])
    from_dead = torch.isin(col, dead)
    assert int((from_dead & (rows != col)).sum()) > 0                        # the dead sensors do have neighbours
    partial = 0
    for _, (X, H, D, Y) in zip(range(3), ds.training):
        validity = X[:, 0, -1]
        assert tuple(validity.shape) == (8, 24, 12) and set(validity.unique().tolist()) <= {0.0, 1.0}
        for mode in ("scale", "drop", 6):
            out = ops.edge_validity_reference(csr.values(), validity, crow, col, mode=mode)
            assert torch.count_nonzero(out[:, from_dead]) == 0               # in every sample
            kept = ops.edge_validity_reference(csr.values(), validity, crow, col, mode=mode, exempt=rows == col)
            assert torch.equal(kept[:, rows == col], csr.values()[rows == col].expand(8, -1))
            assert torch.equal(kept[:, rows != col], out[:, rows != col])
        counts = (validity > 0.5).sum(-1)
        partial += int(((counts > 0) & (counts < 12)).sum())
        full = (counts == 12)[:, col]                                        # a fully valid source: the weight itself
        assert torch.equal(out[full], csr.values().expand(8, -1)[full])
    assert partial > 0                                                       # the outages cut some windows in part
