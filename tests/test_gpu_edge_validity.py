"""GPU: validity-gated edges (msgat_edge_validity{,_backward}, `ops.edge_validity`, `model.EdgeValidity`,
`MSGAT(missing_edges=...)`).

The kernels through the C ABI against the numpy restatement of tests/edge_validity_ref.py, bit for bit: the forward over
sizes either side of a block, every window length, both weight forms, every mode, exempt edges, on hand-built patterns (a
hub of column degree 70, nodes without an edge, one self-loop); validity read in place from the strided view X[:, 0, -1]
and from a view one element off 16-byte alignment; both backward forms; sharding invariance; a captured forward + backward
replayed on new operands.  The model: every `learn_edge_weights` on both evaluation paths against a twin fed `w * g_ref`
through torch ops, with and without edge dropout; the masked attention weights; an all-valid batch.  The Trainer eager /
captured / "auto" on a synthetic series with outages, from device-resident windows and from a DataLoader.
"""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_err

import edge_validity_ref as ref
import ms_gat_amd
from ms_gat_amd import _lib, graph, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

NNZ = (1, 3, 4, 5, 255, 256, 257, 1027)
VS = (1, 2, 5, 33)
TILE = 64         # kEbSumSamples of csrc/edge_batch.hpp: the samples whose terms a block of a summing backward forms at a time
TILE_VS = (TILE, TILE + 1, 2 * TILE + 1)          # exactly a tile, a tile plus one, two tiles plus one
TILE_NNZ = (5, 65)                                # a partial quad; a second block that holds one edge


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32))


class Pattern:
    """A hand-built pattern on the device and the library's structure of it."""

    def __init__(self, nnz, seed=0):
        self.crow_np, self.col_np, self.N = ref.pattern(nnz, seed)
        self.nnz = nnz
        self.crow, self.col = _dev(self.crow_np, torch.int64), _dev(self.col_np, torch.int64)
        pattern = graph.edge_pattern_of(self.crow, self.col)
        assert pattern.identity                             # columns ascend inside a row: the library's own order
        self.gstruct, self.keep = pattern.structure.on(DEV)
        self.exempt_np = ref.self_loops(self.crow_np, self.col_np) | (np.arange(nnz) % 3 == 0)
        self.exempt = _dev(self.exempt_np, torch.uint8)


def _table(mode, T):
    import ctypes as C
    return (C.c_float * (T + 1))(*ops.edge_validity_table(mode, T))


def _forward_abi(pat, w, val, mode, exempt=None):
    """out pre-filled with NaN; val [V,N,T] with contiguous [N,T] rows, any sample stride"""
    V, N, T = val.shape
    assert val.stride(2) == 1 and val.stride(1) == T
    out = torch.full((V, pat.nnz), float("nan"), device=DEV)
    st = _lib.lib().msgat_edge_validity(pat.gstruct, _ptr(w), _ptr(exempt), _ptr(val), val.stride(0) if V > 1 else N * T,
                                        _table(mode, T), _ptr(out), V, T, int(w.dim() == 2), _lib.stream_handle(DEV))
    assert st == 0, st
    torch.cuda.synchronize()
    return out


def _backward_abi(pat, dout, sets, val, mode, exempt=None):
    V, N, T = val.shape
    dw = torch.full((V, pat.nnz) if sets else (pat.nnz,), float("nan"), device=DEV)
    st = _lib.lib().msgat_edge_validity_backward(pat.gstruct, _ptr(dout), _ptr(exempt), _ptr(val),
                                                 val.stride(0) if V > 1 else N * T, _table(mode, T), _ptr(dw), V, T, int(sets),
                                                 _lib.stream_handle(DEV))
    assert st == 0, st
    torch.cuda.synchronize()
    return dw


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------

@pytest.mark.parametrize("nnz", NNZ)
def test_forward_has_the_bits_of_the_restatement(nnz):
    pat = Pattern(nnz)
    if nnz >= 255:
        assert np.bincount(pat.col_np, minlength=pat.N)[2] == 70             # the hub
    rng = np.random.default_rng(nnz)
    for V in VS:
        w2 = rng.standard_normal((V, nnz)).astype(np.float32)
        for T in ref.T_SET:
            val = ref.validity(V, pat.N, T, seed=nnz + V + T)
            val_t = _dev(val)
            for w in (w2[0], w2):
                w_t = _dev(w)
                for mode in ref.modes(T):
                    for exempt, exempt_t in ((None, None), (pat.exempt_np, pat.exempt)):
                        out = _forward_abi(pat, w_t, val_t, mode, exempt_t)
                        want = ref.forward(w, val, pat.col_np, mode, exempt)
                        assert _same_bits(out, want), (V, T, w.ndim, mode, exempt is not None)
            # a window without a missing reading leaves the weights bit for bit as they were, in every mode
            ones = torch.ones(V, pat.N, T, device=DEV)
            for mode in ref.modes(T):
                assert _same_bits(_forward_abi(pat, _dev(w2), ones, mode), w2), (V, T, mode)


@pytest.mark.parametrize("T", ref.T_SET)
def test_validity_is_read_in_place_from_a_strided_and_from_a_misaligned_view(T):
    B, R, Cin, nnz = 5, 2, 3, 257
    pat = Pattern(nnz, seed=T)
    rng = np.random.default_rng(T)
    val = ref.validity(B, pat.N, T, seed=T)
    w = rng.standard_normal((B, nnz)).astype(np.float32)
    want = ref.forward(w, val, pat.col_np, "scale", pat.exempt_np)
    # X [B,R,C,N,T] contiguous, the validity channel last: the view X[:, 0, -1] has sample stride R*C*N*T
    X = torch.randn(B, R, Cin, pat.N, T, device=DEV)
    X[:, 0, -1] = _dev(val)
    view = X[:, 0, -1]
    assert not view.is_contiguous() and view.stride() == (R * Cin * pat.N * T, T, 1) and view.data_ptr() % 16 == 0
    assert _same_bits(_forward_abi(pat, _dev(w), view, "scale", pat.exempt), want)
    # one element off 16-byte alignment: the base, and (an odd sample stride) every other sample as well
    for stride in (pat.N * T, pat.N * T + 1, pat.N * T + 4):
        store = torch.full((B * stride + 8,), float("nan"), device=DEV)
        for offset in (1, 0):
            if offset == 0 and stride % 4 == 0:
                continue                                    # aligned in every respect: covered above
            off = torch.as_strided(store, (B, pat.N, T), (stride, T, 1), offset)
            off.copy_(_dev(val))
            assert (off.data_ptr() % 16 != 0) == (offset == 1)
            assert _same_bits(_forward_abi(pat, _dev(w), off, "scale", pat.exempt), want), (stride, offset)
            dw = _backward_abi(pat, _dev(w), False, off, "scale", pat.exempt)
            assert _same_bits(dw, ref.backward_shared(w, val, pat.col_np, "scale", pat.exempt_np)), (stride, offset)
            # the op hands the same views on as they are
            got = ops.edge_validity(_dev(w), off, pat.crow, pat.col, exempt=pat.exempt)
            assert _same_bits(got, want), (stride, offset)
    got = ops.edge_validity(_dev(w), view, pat.crow, pat.col, exempt=pat.exempt)
    assert _same_bits(got, want) and got.is_contiguous()
    # rows that are not contiguous (a transposed view): the op copies, the result is the same
    swapped = _dev(val).transpose(1, 2).contiguous().transpose(1, 2)
    assert swapped.stride(2) != 1
    assert _same_bits(ops.edge_validity(_dev(w), swapped, pat.crow, pat.col, exempt=pat.exempt), want)


def test_a_nan_weight_on_a_fully_gated_edge_is_plus_zero():
    V, T, nnz = 5, 12, 257
    pat = Pattern(nnz)
    val = ref.validity(V, pat.N, T)
    for w in (np.full(nnz, np.nan, np.float32), np.full((V, nnz), -np.inf, np.float32), np.full(nnz, -1.0, np.float32)):
        for mode in ("scale", "drop"):
            out = _forward_abi(pat, _dev(w), _dev(val), mode, pat.exempt).cpu().numpy()
            gated = (ref.gates(val, pat.col_np, mode) == 0) & ~pat.exempt_np[None, :]
            assert gated.any() and not out[gated].view(np.int32).any()       # +0: not -0, not NaN
            want = ref.forward(w, val, pat.col_np, mode, pat.exempt_np)
            if np.isnan(w).any():                           # everywhere else the NaN goes through (its payload is the unit's)
                assert np.isnan(out[~gated]).all() and np.isnan(want[~gated]).all()
            else:
                assert _same_bits(torch.from_numpy(out), want)
            dw = _backward_abi(pat, _dev(np.broadcast_to(w, (V, nnz))), True, _dev(val), mode, pat.exempt).cpu().numpy()
            assert not dw[gated].view(np.int32).any()


@pytest.mark.parametrize("nnz", NNZ + tuple(n for n in TILE_NNZ if n not in NNZ))
def test_backward_forms_have_the_bits_of_the_restatement(nnz):
    pat = Pattern(nnz)
    rng = np.random.default_rng(100 + nnz)
    # 70: more samples than an LDS tile of the summing form holds; the tile's own edges at TILE_NNZ
    for V in (VS + (70,) if nnz in NNZ else ()) + (TILE_VS if nnz in TILE_NNZ else ()):
        dout = rng.standard_normal((V, nnz)).astype(np.float32)
        dout_t = _dev(dout)
        for T in ref.T_SET:
            val = ref.validity(V, pat.N, T, seed=nnz + V + T)
            val_t = _dev(val)
            for mode in ref.modes(T):
                for exempt, exempt_t in ((None, None), (pat.exempt_np, pat.exempt)):
                    got = _backward_abi(pat, dout_t, True, val_t, mode, exempt_t)
                    assert _same_bits(got, ref.backward_sets(dout, val, pat.col_np, mode, exempt)), ("sets", V, T, mode)
                    got = _backward_abi(pat, dout_t, False, val_t, mode, exempt_t)
                    assert bool(torch.isfinite(got).all())                   # every entry written
                    assert _same_bits(got, ref.backward_shared(dout, val, pat.col_np, mode, exempt)), ("shared", V, T, mode)


def test_null_outputs_and_empty_sizes_write_nothing():
    L, s = _lib.lib(), _lib.stream_handle(DEV)
    pat, empty = Pattern(5), _lib.Graph()
    empty.n_nodes, empty.nnz = pat.N, 0
    one = torch.zeros(8, device=DEV)
    val = torch.ones(2, pat.N, 12, device=DEV)
    p, table = one.data_ptr(), _table("scale", 12)
    for fn in (L.msgat_edge_validity, L.msgat_edge_validity_backward):
        assert fn(pat.gstruct, p, None, val.data_ptr(), pat.N * 12, table, p, 0, 12, 0, s) == 0
        assert fn(empty, p, None, val.data_ptr(), pat.N * 12, table, p, 2, 12, 1, s) == 0
    dout = torch.ones(2, 5, device=DEV)
    for sets in (0, 1):
        assert L.msgat_edge_validity_backward(pat.gstruct, dout.data_ptr(), None, val.data_ptr(), pat.N * 12, table, None, 2,
                                              12, sets, s) == 0
    torch.cuda.synchronize()
    assert not one.cpu().numpy().view(np.int32).any()
    # the op on an empty batch
    w = torch.ones(5, device=DEV, requires_grad=True)
    out = ops.edge_validity(w, val[:0], pat.crow, pat.col)
    assert out.shape == (0, 5)
    out.sum().backward()
    assert torch.count_nonzero(w.grad) == 0


def test_two_calls_give_the_same_bits_and_the_op_agrees_with_autograd_of_its_restatement():
    V, T, nnz = 33, 12, 1027
    pat = Pattern(nnz)
    rng = np.random.default_rng(3)
    val_np = ref.validity(V, pat.N, T)
    val = _dev(val_np)
    w1_np, w2_np = rng.standard_normal(nnz).astype(np.float32), rng.standard_normal((V, nnz)).astype(np.float32)
    dout_np = rng.standard_normal((V, nnz)).astype(np.float32)
    dout = _dev(dout_np)
    for mode in ("scale", "drop", 7):
        for w_np in (w1_np, w2_np):
            runs = []
            for _ in range(2):
                w = _dev(w_np).requires_grad_(True)
                out = ops.edge_validity(w, val, pat.crow, pat.col, mode=mode, exempt=pat.exempt)
                assert out.shape == (V, nnz) and out.is_contiguous() and out.dtype == torch.float32
                (g,) = torch.autograd.grad(out, w, dout)
                runs.append((out.detach(), g))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
            assert _same_bits(runs[0][0], ref.forward(w_np, val_np, pat.col_np, mode, pat.exempt_np))
            # torch autograd of the restatement
            wr = _dev(w_np).requires_grad_(True)
            out_r = ops.edge_validity_reference(wr, val, pat.crow, pat.col, mode=mode, exempt=pat.exempt)
            (gr,) = torch.autograd.grad(out_r, wr, dout)
            assert torch.equal(runs[0][0], out_r.detach())
            if w_np.ndim == 2:
                assert torch.equal(runs[0][1], gr)
                assert _same_bits(runs[0][1], ref.backward_sets(dout_np, val_np, pat.col_np, mode, pat.exempt_np))
            else:   # torch sums the batch in an order of its own: V roundings of 2^-24 each bound the difference
                bound = V * 2.0 ** -24 * (dout.abs() * (out_r.detach() != 0)).sum(0)
                assert bool(((runs[0][1] - gr).abs() <= bound + 1e-30).all())
                assert _same_bits(runs[0][1], ref.backward_shared(dout_np, val_np, pat.col_np, mode, pat.exempt_np))
    # validity is data: no gradient reaches it, a weight without a gradient makes no backward node, bool exempt flags
    v = val.clone().requires_grad_(True)
    out = ops.edge_validity(_dev(w1_np).requires_grad_(True), v, pat.crow, pat.col, exempt=pat.exempt.bool())
    out.sum().backward()
    assert v.grad is None
    assert not ops.edge_validity(_dev(w1_np), val, pat.crow, pat.col).requires_grad
    with pytest.raises(RuntimeError, match="differentiate twice"):
        w = _dev(w1_np).requires_grad_(True)
        (g,) = torch.autograd.grad(ops.edge_validity(w, val, pat.crow, pat.col), w, dout.clone().requires_grad_(True),
                                   create_graph=True)
        g.sum().backward()


def test_op_takes_columns_in_any_order_inside_a_row():
    """(crow, col) with every row's columns reversed: weights, exempt flags, values and gradients stay in the caller's order"""
    V, T, nnz = 5, 12, 257
    pat = Pattern(nnz)
    perm = np.concatenate([np.arange(pat.crow_np[i], pat.crow_np[i + 1])[::-1] for i in range(pat.N)])
    col = _dev(pat.col_np[perm], torch.int64)
    assert not graph.edge_pattern_of(pat.crow, col).identity
    rng = np.random.default_rng(5)
    val_np, dout_np = ref.validity(V, pat.N, T), rng.standard_normal((V, nnz)).astype(np.float32)
    for w_np in (rng.standard_normal(nnz).astype(np.float32), rng.standard_normal((V, nnz)).astype(np.float32)):
        w = _dev(w_np[..., perm]).requires_grad_(True)
        out = ops.edge_validity(w, _dev(val_np), pat.crow, col, exempt=_dev(pat.exempt_np[perm], torch.uint8))
        assert _same_bits(out.detach(), ref.forward(w_np, val_np, pat.col_np, "scale", pat.exempt_np)[:, perm])
        out.backward(_dev(dout_np[:, perm]))
        back = ref.backward_shared if w_np.ndim == 1 else ref.backward_sets
        assert _same_bits(w.grad, back(dout_np, val_np, pat.col_np, "scale", pat.exempt_np)[..., perm])


@pytest.mark.parametrize("V,nnz", [(7, 257), (33, 1027)])
def test_rows_of_a_call_are_the_call_on_that_shard(V, nnz):
    T = 12
    pat = Pattern(nnz)
    rng = np.random.default_rng(V)
    val = _dev(ref.validity(V, pat.N, T, seed=V))
    w2 = _dev(rng.standard_normal((V, nnz)).astype(np.float32))
    dout = _dev(rng.standard_normal((V, nnz)).astype(np.float32))
    for w in (w2[0].contiguous(), w2):
        whole = _forward_abi(pat, w, val, "scale", pat.exempt)
        g_whole = _backward_abi(pat, dout, True, val, "scale", pat.exempt)
        for world in (2, 3):
            for rank in range(world):
                lo, hi = ms_gat_amd.parallel.shard_bounds(V, rank, world)
                part = _forward_abi(pat, w if w.dim() == 1 else w[lo:hi].contiguous(), val[lo:hi], "scale", pat.exempt)
                assert torch.equal(part, whole[lo:hi]), (world, rank)
                g = _backward_abi(pat, dout[lo:hi].contiguous(), True, val[lo:hi], "scale", pat.exempt)
                assert torch.equal(g, g_whole[lo:hi]), (world, rank)


def test_hip_graph_replays_follow_new_validity_weights_and_gradients():
    B, R, Cin, T, nnz = 32, 2, 2, 12, 1027
    pat = Pattern(nnz)
    rng = np.random.default_rng(5)
    X = torch.zeros(B, R, Cin, pat.N, T, device=DEV)
    w = torch.nn.Parameter(torch.zeros(nnz, device=DEV))
    w2 = torch.nn.Parameter(torch.zeros(B, nnz, device=DEV))
    dout = torch.zeros(B, nnz, device=DEV)
    outs = [torch.empty((B, nnz), device=DEV) for _ in range(2)]

    def fill(seed):
        val = ref.validity(B, pat.N, T, seed=seed)
        a, b = rng.standard_normal(nnz).astype(np.float32), rng.standard_normal((B, nnz)).astype(np.float32)
        d = rng.standard_normal((B, nnz)).astype(np.float32)
        with torch.no_grad():
            X[:, 0, -1] = _dev(val)
            w.copy_(_dev(a)), w2.copy_(_dev(b)), dout.copy_(_dev(d))
        return val, a, b, d

    def step():
        for q in (w, w2):
            q.grad.zero_()
        a = ops.edge_validity(w, X[:, 0, -1], pat.crow, pat.col, mode="scale", exempt=pat.exempt)
        b = ops.edge_validity(w2, X[:, 0, -1], pat.crow, pat.col, mode=7)
        outs[0].copy_(a.detach())
        outs[1].copy_(b.detach())
        (a + b).backward(dout)

    def check(val, a, b, d):
        torch.cuda.synchronize()
        assert _same_bits(outs[0], ref.forward(a, val, pat.col_np, "scale", pat.exempt_np))
        assert _same_bits(outs[1], ref.forward(b, val, pat.col_np, 7))
        assert _same_bits(w.grad, ref.backward_shared(d, val, pat.col_np, "scale", pat.exempt_np))
        # autograd ADDS into the zeroed .grad: (+0) + term turns a -0 into +0
        assert _same_bits(w2.grad, np.zeros((B, nnz), np.float32) + ref.backward_sets(d, val, pat.col_np, 7))

    w.grad, w2.grad = torch.zeros_like(w), torch.zeros_like(w2)
    fill(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for seed in (1, 2, 3):
        operands = fill(seed)
        g.replay()
        check(*operands)
    operands = fill(4)
    step()
    check(*operands)


# ---- the model -------------------------------------------------------------------------------------------------------

N_NODES, N_EDGES, R, BATCH = 32, 40, 3, 8
LEARN = [False, True, "time", "signal"]
MODE = "scale"


def _dataset(device=None):
    from ms_gat_amd import data
    torch.manual_seed(0)
    return data.SyntheticPEMS(n_nodes=N_NODES, n_edges=N_EDGES, n_channels=1, in_hours=[1, 2, 3], batch_size=BATCH, days=2,
                              missing=0.15, dead_sensors=2, input_null_value=0.0, device=device)


def _model(ds, learn, seed=0, **kwargs):
    from ms_gat_amd import model
    torch.manual_seed(seed)
    net = model.msgat48(n_components=R, in_channels=ds.input_channels, in_timesteps=12, out_timesteps=12, use_te=True,
                        adj=ds.adj, learn_edge_weights=learn, **kwargs)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                        # every sample its own weights
        if learn == "time":
            for t in (net.edge_h_ebd.weight, net.edge_d_ebd.weight):
                t.copy_(torch.randn(t.shape, generator=g) * 0.05)
        if learn == "signal":
            half = net.edge_proj.weight[net.edge_rank:]
            half.copy_(torch.randn(half.shape, generator=g) * 0.05)
    return net


def _pattern(ds):
    csr = ds.adj.to_sparse_csr()
    crow, col = csr.crow_indices(), csr.col_indices()
    rows = torch.repeat_interleave(torch.arange(N_NODES), crow[1:] - crow[:-1])
    return crow.to(DEV), col.to(DEV), rows.to(DEV), (rows == col).numpy()


def _twin(net, crow, col, rows, g_ref):
    """`net`'s parameters and dropout stream, the adjacency formed apart from `MSGAT.adjacency`: the package's ops for the
    weights and the dropout, then `w * g_ref` by torch ops, through `ops.edge_adjacency`.  A weight [nnz] that requires grad
    is repeated into a [B,nnz] leaf kept in `twin.per_sample`: torch's own batch sum promises no order, so `_ordered_sum`
    adds the leaf's gradient rows from +0 in ascending sample order, the order the kernel is specified to use."""
    twin = copy.deepcopy(net)
    twin.missing_edges = None
    twin.per_sample = []
    zero = torch.zeros((), device=DEV)

    def adjacency(H=None, D=None, X=None):
        learn = twin.learn_edge_weights
        if learn is False:
            w = twin.adj.detach()[rows, col]
        elif learn is True:
            w = twin.edge_weight
        elif learn == "time":
            w = ops.edge_time_weights(twin.edge_weight, twin.edge_h_ebd.weight, twin.edge_d_ebd.weight, H, D)
        else:
            w = ops.edge_signal_weights(twin.edge_weight, twin.edge_proj(twin.edge_features(X)), twin.edge_crow, twin.edge_col)
        if twin.edge_dropout > 0 and twin.training and torch.is_grad_enabled():
            w = ops.edge_dropout(w, twin.edge_dropout, twin.edge_drop_state, sample_offset=0, exempt=twin.edge_drop_exempt,
                                 samples=H.shape[0] if w.dim() == 1 else None)
        if w.dim() == 1 and w.requires_grad and torch.is_grad_enabled():
            w = w.detach()[None, :].repeat(g_ref.shape[0], 1).requires_grad_(True)
            twin.per_sample.append(w)
        w = w if w.dim() == 2 else w[None, :]
        return ops.edge_adjacency(crow, col, torch.where(g_ref == 0, zero, w * g_ref))
    twin.adjacency = adjacency
    twin.batch_adjacency = lambda X, H, D: adjacency(H, D, X)
    return twin


def _ordered_sum(rows: torch.Tensor) -> torch.Tensor:
    acc = torch.zeros_like(rows[0])
    for row in rows:                             # from +0, in ascending sample order, each partial sum rounded to fp32
        acc = acc + row
    return acc


def _step(net, X, H, D, dY):
    net.zero_grad(set_to_none=True)
    out = net(X, H, D)
    (out * dY).sum().backward()
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    for leaf in getattr(net, "per_sample", ()):  # the twin's shared edge weight: its gradient is the ordered batch sum
        assert "edge_weight" not in grads
        grads["edge_weight"] = _ordered_sum(leaf.grad)
    if hasattr(net, "per_sample"):
        net.per_sample.clear()
    return out.detach(), grads


@pytest.fixture(scope="module")
def batch():
    ds = _dataset()
    X, H, D, Y = (t.to(DEV) for t in next(iter(ds.training)))
    assert X.shape == (BATCH, R, 2, N_NODES, 12)
    dY = torch.randn(Y.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    crow, col, rows, diag = _pattern(ds)
    val = X[:, 0, -1].cpu().numpy()
    counts = ref.counts(val)
    assert (counts == 0).any() and ((counts > 0) & (counts < 12)).any() and (counts == 12).any()
    g_np = ref.gates(val, col.cpu().numpy(), MODE)
    g_np[:, diag] = 1.0                                     # the stored diagonal is exempt
    return ds, X, H, D, dY, (crow, col, rows, diag), g_np


@pytest.mark.parametrize("dropout", [0.0, 0.25])
@pytest.mark.parametrize("stack", [True, False])
@pytest.mark.parametrize("learn", LEARN)
def test_model_equals_its_twin_fed_the_restatements_gate(batch, learn, stack, dropout):
    ds, X, H, D, dY, (crow, col, rows, diag), g_np = batch
    net = _model(ds, learn, missing_edges=MODE, edge_dropout=dropout, edge_dropout_seed=77).to(DEV).train()
    net.stack_components = stack
    twin = _twin(net, crow, col, rows, _dev(g_np))          # a copy made before the step: the same place in the mask stream
    twin.stack_components = stack
    what = f"missing edges, learn={learn!r}, stacked={stack}, dropout={dropout}"
    for step in (0, 1):
        before = net.edge_dropout_state()
        got, got_g = _step(net, X, H, D, dY)
        if dropout:
            assert net.edge_dropout_state() == {"seed": 77, "step": step + 1}
            assert twin.edge_dropout_state() == before      # the twin draws from where the model drew
        want, want_g = _step(twin, X, H, D, dY)
        assert torch.equal(got, want), (what, step)
        assert set(got_g) == set(want_g)
        edge_keys = [k for k in want_g if k.startswith("edge_")]
        assert bool(edge_keys) == bool(learn)
        for k, v in want_g.items():
            if k in edge_keys:
                assert float(v.abs().max()) > 0, k
                print(f"{what} step {step} {k}: max |difference| {float((got_g[k] - v).abs().max()):.3e}")
            assert torch.equal(got_g[k], v), (what, step, k)
    # the gate does change the forecast, and eval mode / no_grad apply it as well
    plain = _model(ds, learn).to(DEV)
    plain.load_state_dict(net.state_dict())
    plain.stack_components = stack
    net.eval(), plain.eval(), twin.eval()
    with torch.no_grad():
        out = net(X, H, D)
        assert torch.equal(out, twin(X, H, D)) and not torch.equal(out, plain(X, H, D))


@pytest.mark.parametrize("stack", [True, False])
@pytest.mark.parametrize("learn", LEARN)
def test_an_all_valid_batch_gives_the_bits_of_the_ungated_model(batch, learn, stack):
    ds, X, H, D, dY, _, _ = batch
    net = _model(ds, learn, missing_edges="drop").to(DEV).train()
    plain = _model(ds, learn).to(DEV).train()
    plain.load_state_dict(net.state_dict())
    net.stack_components = plain.stack_components = stack
    Xv = X.clone()
    Xv[:, :, -1] = 1.0
    got, got_g = _step(net, Xv, H, D, dY)
    want, want_g = _step(plain, Xv, H, D, dY)
    assert torch.equal(got, want) and set(got_g) == set(want_g)
    for k, v in want_g.items():
        if k == "edge_weight" and learn is True:
            # [B,nnz] per-sample gradients summed by the gate's backward against the shared-weight kernel's own sum over
            # the groups: the same terms in another order, held to the package's fp32 parity bar
            assert rel_err(got_g[k].cpu(), v.cpu()) < 1e-4, k
        else:
            assert torch.equal(got_g[k], v), k


@pytest.mark.parametrize("stack", [True, False])
def test_a_gated_edge_is_exactly_zero_in_the_masked_attention_and_the_diagonal_never(batch, stack):
    ds, X, H, D, dY, (crow, col, rows, diag), _ = batch
    net = _model(ds, "time", missing_edges="drop").to(DEV).eval()
    net.stack_components = stack
    diag_t = torch.from_numpy(diag).to(DEV)
    gated = torch.from_numpy(ref.gates(X[:, 0, -1].cpu().numpy(), col.cpu().numpy(), "drop") == 0).to(DEV) & ~diag_t[None, :]
    assert gated.any() and (~gated).any()
    maps = net.attention_maps(X, H, D, weights="masked")
    assert len(maps) == R * 2
    for name, m in maps.items():
        at_edges = m.to_dense()[:, rows, col]                                 # [B,nnz]
        assert torch.count_nonzero(at_edges[gated]) == 0, name                # exactly zero, sample by sample
        assert torch.count_nonzero(at_edges[~gated]) > 0.9 * int((~gated).sum()), name
        assert torch.count_nonzero(at_edges[:, diag_t]) == BATCH * int(diag.sum()), name
    # keep_self=False: a silent sensor loses its diagonal too
    bare = _model(ds, "time", missing_edges="drop", missing_edges_keep_self=False).to(DEV).eval()
    values = bare.adjacency(H, D, X).values()
    assert torch.count_nonzero(values[:, diag_t]) < BATCH * int(diag.sum())


def test_edge_validity_module_feeds_a_gacn(batch):
    from ms_gat_amd import model
    ds, X, H, D, dY, (crow, col, rows, diag), g_np = batch
    values = ds.adj.to_sparse_csr().values().to(DEV).requires_grad_(True)
    gate = model.EdgeValidity(crow, col, mode=MODE).to(DEV)
    assert gate.exempt.device.type == "cuda" and gate.state_dict() == {}
    gacn = ms_gat_amd.GACN(3, 24, 12).to(DEV)
    with torch.no_grad():
        for q in gacn.parameters():
            q.normal_(0, 0.3)
    x = torch.randn(BATCH, 3, N_NODES, 12, device=DEV)
    w = gate(values, X[:, 0, -1])
    assert _same_bits(w.detach(), ref.terms(values.detach().cpu().numpy(), g_np))
    gacn(x, ops.edge_adjacency(crow, col, w)).sum().backward()
    assert values.grad is not None and float(values.grad.abs().max()) > 0


# ---- the Trainer -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("resident", [True, False], ids=["DeviceWindows", "DataLoader"])
@pytest.mark.parametrize("learn", [False, True])
def test_gated_model_trains_eager_captured_and_auto(tmp_path, learn, resident):
    from ms_gat_amd import engine
    ds = _dataset(device=DEV if resident else None)
    net = _model(ds, learn, missing_edges=MODE).to(DEV)
    twin, auto = copy.deepcopy(net), copy.deepcopy(net)
    batches = [b for _, b in zip(range(4), ds.training)]
    assert any(bool((b[0][:, 0, -1] == 0).any()) for b in batches)
    trainers = [engine.Trainer(m, 50.0, str(tmp_path / tag), hip_graph=hg, null_value=0.0, max_grad_norm=0.25,
                               skip_nonfinite=True)
                for m, tag, hg in ((net, "eager", False), (twin, "graph", True), (auto, "auto", "auto"))]
    for epoch in (1, 2):
        losses = [t.run_epoch(batches, gpu_id=0, epoch=epoch, mode="train") for t in trainers]
        print(f"learn={learn!r} epoch {epoch}: loss eager {losses[0]!r}, captured {losses[1]!r}, auto {losses[2]!r}")
        assert all(x == x and abs(x) < float("inf") for x in losses), losses
        for other in losses[1:]:
            assert abs(losses[0] - other) < 1e-4 * abs(losses[0]), (epoch, losses)
        for t in trainers:
            assert t.last_stats is not None and t.last_stats["skipped_steps"] == 0
            t.run_epoch([b for _, b in zip(range(2), ds.validation)], gpu_id=0, epoch=epoch, mode="validate")
    assert sum(1 for k in trainers[1]._graphs if k[0]) == 1 and sum(1 for k in trainers[2]._graphs if k[0]) == 1
    for other, tag in ((twin, "captured"), (auto, "auto")):
        worst = max((rel_err(q.detach().cpu(), p.detach().cpu()), n)
                    for (n, p), q in zip(net.named_parameters(), other.parameters()))
        print(f"{tag} vs eager: worst parameter {worst[1]} rel err {worst[0]:.3e}")
        for (name, p), q in zip(net.named_parameters(), other.parameters()):
            assert rel_err(q.detach().cpu(), p.detach().cpu()) < 2e-2, (tag, name)
