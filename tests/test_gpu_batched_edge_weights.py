"""GPU: a per-sample sparse adjacency [V,N,N] (torch COO with three sparse dimensions, torch batched CSR, or
`ops.edge_adjacency` with weights [V,nnz]) with a gradient at every sample's stored entries
(msgat_edge_weight_grad_sets).

Parity with the reference's fixtures for a per-sample adjacency (tests/golden/make_golden_adjacency.py,
make_golden_attention.py), the merged dense [V,N,N] route as the yardstick for the project-first GACN and the MEAM's
channel slice, float64 autograd of the dense restatement for every V, T and backward form, the SELL and split-operand
sizes; values read in place, gathered and strided; determinism; a HIP-graph capture of a step whose weights come from a
small network; and the frozen path bit for bit equal to the dense [V,N,N] one.
"""
import numpy as np
import pytest
import torch

from conftest import assert_parity, load_golden
from oracle import dense_torch

import ms_gat_amd
from ms_gat_amd import graph as G
from ms_gat_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _load_module(m, state):
    with torch.no_grad():
        for k, v in state.items():
            m.get_parameter(k).copy_(_dev(v))
    return m.to(DEV)


def _inputs(g, grad="dz"):
    if "x_q32" in g:
        return g["x_q32"].astype(np.float32) / 32, g[grad + "_q32"].astype(np.float32) / 32
    return g["x"].astype(np.float32), g[grad].astype(np.float32)


def _crow(rows, N):
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))])


def _sparse(adj, layout):
    """(sparse [V,N,N] adjacency on the device, its leaf values, the stored (v, i, j) in the values' order).  "coo": every
    sample stores its own non-zeros; "csr": torch wants one entry count per sample, so every sample stores the union of
    the patterns, explicit zeros where it lacks an edge."""
    V, N = adj.shape[0], adj.shape[1]
    if layout == "coo":
        v, i, j = np.nonzero(adj)
        vals = torch.nn.Parameter(_dev(adj[v, i, j]))
        a = torch.sparse_coo_tensor(_dev(np.stack([v, i, j]), torch.int64), vals, (V, N, N), is_coalesced=True)
        return a, vals, (v, i, j)
    ur, uc = np.nonzero((adj != 0).any(0))
    vals = torch.nn.Parameter(_dev(adj[:, ur, uc]))
    a = torch.sparse_csr_tensor(_dev(np.tile(_crow(ur, N), (V, 1)), torch.int64), _dev(np.tile(uc, (V, 1)), torch.int64),
                                vals, (V, N, N))
    return a, vals, (np.repeat(np.arange(V), len(ur)), np.tile(ur, V), np.tile(uc, V))


def _stored(dense, where):
    return dense[where]


# ---- the reference's fixtures ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_gacn_matches_reference_fixture(layout):
    name = "adjgrad_gacn_b3c3n64_bnn.npz"
    g = load_golden(name)
    xn, dzn = _inputs(g)
    C, O = xn.shape[1], g["W"].shape[0]
    m = _load_module(ms_gat_amd.GACN(C, O, 12), {"gatt.Wg": g["Wg"], "gatt.alpha": g["alpha"], "W": g["W"]})
    x = _dev(xn).requires_grad_(True)
    adj, vals, where = _sparse(g["adj"], layout)
    if layout == "coo":       # the samples' patterns differ: the union and the flat map are exercised
        assert G.sparse_sets_of(adj).flat is not None
    z = m(x, adj)
    z.backward(_dev(dzn))
    for got, key in ((z, "z"), (x.grad, "dx"), (m.gatt.Wg.grad, "dWg"), (m.gatt.alpha.grad, "dalpha"), (m.W.grad, "dW")):
        assert_parity(got, g[key], name + " " + layout, key)
    assert vals.grad.shape == vals.shape
    assert_parity(vals.grad.reshape(-1), _stored(g["dadj"], where), name + " " + layout, "dval")


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_weights_match_reference_fixture(layout):
    """need_weights under the fixture's loss <dY, y> + <dM, att * adjacency>: the dE_extra term of the new entry point"""
    name = "attw_gacn_b3c3n64_bnn.npz"
    g = load_golden(name)
    xn, dyn = _inputs(g, "dy")
    C, O = xn.shape[1], g["W"].shape[0]
    m = _load_module(ms_gat_amd.GACN(C, O, 12), {"gatt.Wg": g["Wg"], "gatt.alpha": g["alpha"], "W": g["W"]})
    x = _dev(xn).requires_grad_(True)
    adj, vals, where = _sparse(g["adj"], layout)
    y, w = m(x, adj, need_weights=True)
    ((y * _dev(dyn)).sum() + (w.to_dense() * _dev(g["dM"].astype(np.float32))).sum()).backward()
    what = name + " " + layout
    assert_parity(y, g["y"], what, "y")
    assert_parity(w.to_dense(), g["M"], what, "masked")
    for got, key in ((x.grad, "dx"), (m.gatt.Wg.grad, "dWg"), (m.gatt.alpha.grad, "dalpha"), (m.W.grad, "dW")):
        assert_parity(got, g[key], what, key)
    assert_parity(vals.grad.reshape(-1), _stored(g["dadj"], where), what, "dval")


# ---- project-first GACN and the MEAM's channel slice: the dense [V,N,N] route as the yardstick -----------------------

def _learned_adjacency(N, seed, V):
    """sym-normalised random graphs (a pattern per sample) times independent weights per direction"""
    rng = np.random.default_rng(seed)
    out = []
    for v in range(V):
        a = ms_gat_amd.synthetic_adjacency(N, N + 6 + 3 * v, seed + v).numpy()
        out.append(a * rng.uniform(0.25, 1.5, (N, N)).astype(np.float32))
    return np.stack(out)


def _case(B, C, O, N, T, seed, R=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R * B, C, N, T)).astype(np.float32)
    dz = rng.standard_normal((R * B, O or C, N, T)).astype(np.float32)
    Wg = (rng.standard_normal((R, T, T)) * (1.0 / T) ** 0.5).astype(np.float32)
    alpha = rng.uniform(-C ** -0.5, C ** -0.5, (R, C)).astype(np.float32)
    W = (rng.standard_normal((R, O, C)) * (2.0 / (O + C)) ** 0.5).astype(np.float32) if O else None
    return x, dz, Wg, alpha, W


def _run_gacn(x, dz, Wg, alpha, W, adjacency):
    xt = _dev(x).requires_grad_(True)
    ps = [_dev(t).requires_grad_(True) for t in (alpha, Wg)] + [None if W is None else _dev(W).requires_grad_(True)]
    z = ops.gacn(xt, ps[0], ps[1], ps[2], adjacency)
    z.backward(_dev(dz))
    return [z.detach(), xt.grad] + [p.grad for p in ps if p is not None]


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_project_first_gacn_equals_dense_route(layout):
    B, C, O, N, T = 2, 72, 24, 47, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=31)
    adj = _learned_adjacency(N, 17, B)
    dense = _dev(adj).requires_grad_(True)
    want = _run_gacn(x, dz, Wg, alpha, W, dense)
    a, vals, where = _sparse(adj, layout)
    got = _run_gacn(x, dz, Wg, alpha, W, a)
    for u, v in zip(got, want):
        assert torch.equal(u, v)          # the same union structure, the same E, the same kernels
    assert_parity(vals.grad.reshape(-1), dense.grad.cpu().numpy()[where], "proj_first " + layout, "dval")


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_meam_channel_slice_equals_dense_route(layout):
    """MEAM(72 -> 72): the attention core, whose dv is a channel slice of the block's concatenated gradient"""
    B, N, T = 2, 32, 12
    rng = np.random.default_rng(5)
    adj = _learned_adjacency(N, 23, B)
    x = rng.standard_normal((B, 72, N, T)).astype(np.float32)
    dout = rng.standard_normal((B, 72, N, T)).astype(np.float32)
    torch.manual_seed(3)
    m = ms_gat_amd.MEAM(72, 72, n_nodes=N, n_timesteps=T, dilations=[1, 2])
    with torch.no_grad():                 # a bare block's parameters are uninitialised storage: MSGAT.reset_parameters' rule
        for p in m.parameters():
            if p.dim() >= 2:
                torch.nn.init.xavier_normal_(p)
            else:
                p.uniform_(-p.size(0) ** -0.5, p.size(0) ** -0.5)
    m = m.to(DEV)

    def run(adjacency):
        m.zero_grad(set_to_none=True)
        xt = _dev(x).requires_grad_(True)
        out = m(xt, adjacency)
        out.backward(_dev(dout))
        return [out.detach(), xt.grad] + [p.grad.clone() for p in m.parameters()]

    dense = _dev(adj).requires_grad_(True)
    want = run(dense)
    a, vals, where = _sparse(adj, layout)
    got = run(a)
    assert all(bool(torch.isfinite(u).all()) for u in want) and float(dense.grad.abs().max()) > 0
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert_parity(vals.grad.reshape(-1), dense.grad.cpu().numpy()[where], "meam slice " + layout, "dval")


# ---- every V, T and backward form against float64 autograd of the dense restatement ---------------------------------

def _oracle_dadj(x, dz, Wg, alpha, W, adj, R):
    """float64 autograd of gacn_dense / graph_attention_dense, relation by relation; adj [B,N,N] (sample b shared by its R
    relations: their gradients add) or [R*B,N,N] (one per group)"""
    a = torch.from_numpy(adj).to(DEV, torch.float64).requires_grad_(True)
    f = lambda t: torch.from_numpy(t).to(DEV, torch.float64)  # noqa: E731
    Gn = x.shape[0]
    B = Gn // R
    outs = []
    for r in range(R):
        ar = a[r * B:(r + 1) * B] if adj.shape[0] == Gn and Gn != B else a
        xr = f(x[r * B:(r + 1) * B])
        if W is None:
            outs.append(dense_torch.graph_attention_dense(xr, ar, f(Wg[r]), f(alpha[r])))
        else:
            outs.append(dense_torch.gacn_dense(xr, ar, f(Wg[r]), f(alpha[r]), f(W[r])))
    z = torch.cat(outs)
    z.backward(f(dz))
    return z.detach(), a.grad


@pytest.mark.parametrize("R,B,C,O,N,T,per_group", [
    (3, 2, 72, 24, 64, 12, False),    # V = B: each value sums its 3 relations; project first, Cu = 24 (SDDMM form)
    (3, 2, 72, 24, 64, 12, True),     # V = R*B
    (3, 2, 3, 0, 64, 4, False),       # plain attention over 3 channels: the direct-row backward form
    (3, 2, 3, 24, 64, 8, True),       # aggregate first, Cu = 3
    (3, 2, 8, 0, 64, 16, False),      # Cu = 8
    (2, 2, 5, 0, 97, 8, False),
    (1, 9, 3, 0, 64, 12, False),      # 9 sets: two rounds over the XCD labels, the second with one set
    (2, 5, 8, 0, 64, 12, True),       # 10 sets of one group
    (3, 1, 2, 3, 2048, 12, False),    # the structure carries the SELL layouts
    (1, 2, 4, 0, 2048, 16, True),
    (3, 1, 72, 24, 1600, 12, False),  # split-operand dense passes form lse
])
def test_stacked_gacn_matches_float64_autograd(R, B, C, O, N, T, per_group):
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=N + T + C, R=R)
    V = R * B if per_group else B
    adj = _learned_adjacency(N, N + 1, V)
    zo, dao = _oracle_dadj(x, dz, Wg, alpha, W, adj, R)
    a, vals, where = _sparse(adj, "coo")
    xt = _dev(x).requires_grad_(True)
    if O:
        m = ms_gat_amd.StackedGACN(R, C, O, T).to(DEV)
        with torch.no_grad():
            m.Wg.copy_(_dev(Wg))
            m.alpha.copy_(_dev(alpha))
            m.W.copy_(_dev(W))
        z = m(xt.view(R, B, C, N, T), a).reshape(R * B, O, N, T)
    else:
        z = ops.gacn(xt, _dev(alpha), _dev(Wg), None, a)
    z.backward(_dev(dz))
    assert G.sparse_sets_of(a).structure.has_sell == (N >= 2048)
    what = f"sets r{R}b{B}c{C}o{O}n{N}t{T}v{V}"
    assert_parity(z, zo.cpu().numpy(), what, "z")
    assert_parity(vals.grad, dao.cpu().numpy()[where], what, "dval")


# ---- edge_adjacency with weights [V,nnz] ----------------------------------------------------------------------------

def _shared_pattern_case(seed, V, N=307):
    B, C, O, T = V, 72, 24, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=seed)
    base = ms_gat_amd.synthetic_adjacency(N, N + 6, seed).numpy()
    r, c = np.nonzero(base)
    rng = np.random.default_rng(seed)
    w = (base[r, c][None, :] * rng.uniform(0.25, 1.5, (V, len(r)))).astype(np.float32)
    adj = np.zeros((V, N, N), np.float32)
    adj[:, r, c] = w
    return x, dz, Wg, alpha, W, adj, r, c, w


def test_edge_adjacency_weights_are_read_in_place():
    V = 2
    x, dz, Wg, alpha, W, adj, r, c, w = _shared_pattern_case(51, V)
    N = adj.shape[1]
    dense = _dev(adj).requires_grad_(True)
    want = _run_gacn(x, dz, Wg, alpha, W, dense)
    wt = torch.nn.Parameter(_dev(w))
    a = ops.edge_adjacency(_dev(_crow(r, N), torch.int64), _dev(c, torch.int64), wt)
    assert torch.equal(a.to_dense(), _dev(adj))
    g = G.graph_for(a, V, 1)
    assert g.on(DEV)[0].val == wt.data_ptr() and g.n_sets == V          # no copy, nothing [N,N]
    got = _run_gacn(x, dz, Wg, alpha, W, a)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert wt.grad.shape == wt.shape and wt.grad.layout == torch.strided
    assert_parity(wt.grad, dense.grad.cpu().numpy()[:, r, c], "edge_adjacency in place", "dweight")


def test_edge_adjacency_reversed_columns_and_strided_weights():
    V = 2
    x, dz, Wg, alpha, W, adj, r, c, w = _shared_pattern_case(52, V)
    N = adj.shape[1]
    dense = _dev(adj).requires_grad_(True)
    want = _run_gacn(x, dz, Wg, alpha, W, dense)
    da = dense.grad.cpu().numpy()
    crow = _crow(r, N)
    perm = np.concatenate([np.arange(crow[i], crow[i + 1])[::-1] for i in range(N)]).astype(np.int64)
    rs, cs = r[perm], c[perm]
    wt = torch.nn.Parameter(_dev(w[:, perm]))
    a = ops.edge_adjacency(_dev(crow, torch.int64), _dev(cs, torch.int64), wt)
    assert G.sparse_sets_of(a).flat is not None                          # the gather path
    got = _run_gacn(x, dz, Wg, alpha, W, a)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert_parity(wt.grad, da[:, rs, cs], "edge_adjacency reversed", "dweight")
    # the same bits as the library's order, permuted
    ws = torch.nn.Parameter(_dev(w))
    _run_gacn(x, dz, Wg, alpha, W, ops.edge_adjacency(_dev(crow, torch.int64), _dev(c, torch.int64), ws))
    assert torch.equal(wt.grad, ws.grad[:, _dev(perm, torch.int64)])
    # weights that are every other column of a wider parameter: not contiguous, copied into the pattern's buffer
    wide = torch.nn.Parameter(torch.stack([_dev(w), _dev(w * 3)], 2).reshape(V, -1))      # [V, 2 nnz]
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    got = _run_gacn(x, dz, Wg, alpha, W, ops.edge_adjacency(_dev(crow, torch.int64), _dev(c, torch.int64), strided))
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert torch.equal(wide.grad[:, ::2], ws.grad)
    assert torch.count_nonzero(wide.grad[:, 1::2]) == 0


def test_bad_leading_size_names_the_allowed_ones():
    x, dz, Wg, alpha, W, adj, r, c, w = _shared_pattern_case(53, 3, N=40)
    a = ops.edge_adjacency(_dev(_crow(r, 40), torch.int64), _dev(c, torch.int64), _dev(w))
    with pytest.raises(ValueError, match=r"leading size in \[1, 2\]"):
        ops.gacn(_dev(x[:2]), _dev(alpha), _dev(Wg), _dev(W), a)


# ---- determinism, capture -------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits():
    R, B, C, O, N, T = 3, 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=8, R=R)
    adj = _learned_adjacency(N, 9, B)
    grads = []
    for _ in range(2):
        a, vals, _ = _sparse(adj, "coo")
        _run_gacn(x, dz, Wg, alpha, W, a)
        grads.append(vals.grad.clone())
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


class _DynamicGraph(torch.nn.Module):
    """the usual dynamic-graph module in small: per-sample edge weights [B,nnz] from the input window (an embedding of
    the sample, times a learned [16,nnz] map, gating the road graph's weights)"""

    def __init__(self, C, T, base):
        super().__init__()
        self.embed = torch.nn.Linear(C * T, 16)
        self.edges = torch.nn.Parameter(torch.randn(16, base.numel()) * 0.5)
        self.register_buffer("base", base)

    def forward(self, x):                              # x [B,C,N,T] -> [B,nnz]
        e = torch.tanh(self.embed(x.mean(dim=2).flatten(1)))                      # [B,16]
        return self.base * (0.5 + torch.sigmoid(e @ self.edges))


def test_hip_graph_capture_of_a_dynamic_graph_step():
    B, C, O, N, T = 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=12)
    base = ms_gat_amd.synthetic_adjacency(N, N + 6, 12).numpy()
    r, c = np.nonzero(base)
    crow_t, col_t = _dev(_crow(r, N), torch.int64), _dev(c, torch.int64)
    torch.manual_seed(1)
    dyn = _DynamicGraph(C, T, _dev(base[r, c])).to(DEV)
    m = _load_module(ms_gat_amd.GACN(C, O, T), {"gatt.Wg": Wg[0], "gatt.alpha": alpha[0], "W": W[0]})
    params = list(dyn.parameters()) + list(m.parameters())
    xs, dzs = _dev(x), _dev(dz)
    out = torch.empty((B, O, N, T), device=DEV)
    wout = torch.empty((B, len(r)), device=DEV)

    def step():
        for p in params:
            p.grad.zero_()
        w = dyn(xs)
        assert w.is_contiguous()
        wout.copy_(w.detach())
        z = m(xs, ops.edge_adjacency(crow_t, col_t, w))
        out.copy_(z.detach())
        z.backward(dzs)

    m(xs, ops.edge_adjacency(crow_t, col_t, dyn(xs))).backward(dzs)     # warm-up: structure, grads
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in dyn.parameters())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    rng = np.random.default_rng(6)
    # a replay cannot read anything back: a synchronising call while the stream was capturing would have failed the
    # capture above, and a replay runs only what was captured
    for _ in range(3):
        xs.copy_(_dev(rng.standard_normal(x.shape).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [out.clone(), wout.clone()] + [p.grad.clone() for p in params]
        step()
        torch.cuda.synchronize()
        eager = [out, wout] + [p.grad for p in params]
        for u, v in zip(replayed, eager):
            assert torch.equal(u, v)


def test_first_sight_inside_a_capture_raises():
    N = 40
    adj = _learned_adjacency(N, 79, 2)
    a, _, _ = _sparse(adj, "coo")
    x = torch.randn(2, 3, N, 12, device=DEV)
    m = ms_gat_amd.GraphAttention(3, 12).to(DEV)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(Exception, match="not cached yet"):
        with torch.cuda.graph(graph):
            m(x, a)


# ---- the frozen path ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["coo", "csr"])
@pytest.mark.parametrize("O", [0, 24])
def test_frozen_sparse_equals_dense_batched_graph_bit_for_bit(O, layout):
    B, C, N, T = 2, 72 if O else 3, 307, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=14)
    adj = _learned_adjacency(N, 15, B)
    want = _run_gacn(x, dz, Wg, alpha, W, _dev(adj))
    a, vals, _ = _sparse(adj, layout)
    got = _run_gacn(x, dz, Wg, alpha, W, a.detach())
    assert vals.grad is None
    for u, v in zip(got, want):
        assert torch.equal(u, v)


# ---- one value set: [1,N,N] is [N,N] --------------------------------------------------------------------------------

@pytest.mark.parametrize("need_weights", [False, True])
@pytest.mark.parametrize("form", ["coo", "edge"])
def test_one_set_equals_the_sparse_matrix_route_bit_for_bit(form, need_weights):
    """n_sets = 1 of msgat_edge_weight_grad_sets is msgat_edge_weight_grad (split kernel, reduction) followed by
    msgat_edge_softmax_grad: the launches of a sparse [N,N] adjacency, so the same bits."""
    B, C, O, N, T = 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=61)
    adj = _learned_adjacency(N, 62, 1)[0]
    r, c = np.nonzero(adj)
    dM = np.random.default_rng(63).standard_normal((B, N, N)).astype(np.float32)
    crow_t, col_t = _dev(_crow(r, N), torch.int64), _dev(c, torch.int64)

    def run(make):
        leaf = torch.nn.Parameter(_dev(adj[r, c]))
        xt = _dev(x).requires_grad_(True)
        ps = [_dev(t).requires_grad_(True) for t in (alpha, Wg, W)]
        if need_weights:
            z, w = ops.gacn(xt, ps[0], ps[1], ps[2], make(leaf), need_weights=True)
            ((z * _dev(dz)).sum() + (w.to_dense() * _dev(dM)).sum()).backward()
        else:
            z = ops.gacn(xt, ps[0], ps[1], ps[2], make(leaf))
            z.backward(_dev(dz))
        return [z.detach(), xt.grad] + [p.grad for p in ps] + [leaf.grad.reshape(-1)]

    idx2 = _dev(np.stack([r, c]), torch.int64)
    idx3 = _dev(np.stack([np.zeros_like(r), r, c]), torch.int64)
    want = run(lambda leaf: torch.sparse_coo_tensor(idx2, leaf, (N, N), is_coalesced=True))
    if form == "coo":
        got = run(lambda leaf: torch.sparse_coo_tensor(idx3, leaf, (1, N, N), is_coalesced=True))
    else:
        got = run(lambda leaf: ops.edge_adjacency(crow_t, col_t, leaf[None, :]))
    assert float(want[-1].abs().max()) > 0
    for u, v in zip(got, want):
        assert torch.equal(u, v)


# ---- an uncoalesced [V,N,N] COO tensor ------------------------------------------------------------------------------

def test_uncoalesced_coo_duplicates_add():
    """a (v, i, j) stored twice: the forward sees the sum, and both stored entries get that edge's gradient"""
    B, C, O, N, T = 2, 72, 24, 64, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=71)
    adj = _learned_adjacency(N, 72, B)
    v, i, j = np.nonzero(adj)
    dup = np.arange(0, len(v), 5)                          # every fifth entry stored twice, its weight split in two parts
    part = adj[v[dup], i[dup], j[dup]] * np.float32(0.25)
    vals_np = np.concatenate([adj[v, i, j], part]).astype(np.float32)
    vals_np[dup] = adj[v[dup], i[dup], j[dup]] - part
    summed = adj.copy()
    summed[v[dup], i[dup], j[dup]] = vals_np[dup] + part    # float32 sums, as coalesce forms them
    dense = _dev(summed).requires_grad_(True)
    want = _run_gacn(x, dz, Wg, alpha, W, dense)
    where = tuple(np.concatenate([t, t[dup]]) for t in (v, i, j))
    vals = torch.nn.Parameter(_dev(vals_np))
    a = torch.sparse_coo_tensor(_dev(np.stack(where), torch.int64), vals, (B, N, N))
    assert not a.is_coalesced()
    got = _run_gacn(x, dz, Wg, alpha, W, a)
    for u, w in zip(got, want):
        assert torch.equal(u, w)
    assert_parity(vals.grad, dense.grad.cpu().numpy()[where], "uncoalesced [V,N,N] coo", "dval")


# ---- the stress size: a dense [V,N,N] cannot exist there ------------------------------------------------------------

def _edge_list(N, n_edges, seed):
    """(rows, cols, values) of a weighted graph with self loops, row-major sorted, built without an [N,N] matrix"""
    e = G.random_edges(N, n_edges, seed)
    rows = np.concatenate([e[:, 0], e[:, 1], np.arange(N)])
    cols = np.concatenate([e[:, 1], e[:, 0], np.arange(N)])
    order = np.argsort(rows * N + cols)
    w = np.random.default_rng(seed).uniform(0.05, 0.5, len(rows)).astype(np.float32)
    return rows[order], cols[order], w


def test_stress_size_matches_float64_at_the_stored_edges():
    """N = 8192, V = B shared by R = 2 relations, a pattern per sample.  The yardstick is the float64 restatement of
    attention.py:33-36 evaluated at the stored edges only: att = softmax(q Wg q^T) over all N columns, z = (att * A) x,
    dA[b,i,j] = sum_r att_g[i,j] sum_{c,t} dz[g,c,i,t] x[g,c,j,t]."""
    R, B, C, N, T = 2, 2, 2, 8192, 12
    x, dz, Wg, alpha, _ = _case(B, C, 0, N, T, seed=81, R=R)
    samples = [_edge_list(N, N + 40 * b, 82 + b) for b in range(B)]
    v = np.concatenate([np.full(len(s[0]), b) for b, s in enumerate(samples)])
    i, j, w = (np.concatenate([s[k] for s in samples]) for k in range(3))
    vals = torch.nn.Parameter(_dev(w))
    a = torch.sparse_coo_tensor(_dev(np.stack([v, i, j]), torch.int64), vals, (B, N, N), is_coalesced=True)
    xt = _dev(x).requires_grad_(True)
    z = ops.gacn(xt, _dev(alpha), _dev(Wg), None, a)
    z.backward(_dev(dz))
    sets = G.sparse_sets_of(a)
    assert sets.flat is not None and sets.structure.has_sell and sets.structure.nnz > max(len(s[0]) for s in samples)

    f = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(DEV, torch.float64)  # noqa: E731
    zo = torch.zeros((R * B, C, N, T), device=DEV, dtype=torch.float64)
    dao = []
    for b, (rows, cols, wb) in enumerate(samples):
        ri, ci = _dev(rows, torch.int64), _dev(cols, torch.int64)
        grad = torch.zeros(len(rows), device=DEV, dtype=torch.float64)
        for r in range(R):
            g = r * B + b
            xg, dzg = f(x[g]), f(dz[g])
            q = torch.einsum("cnt,c->nt", xg, f(alpha[r]))
            score = (q @ f(Wg[r])) @ q.t()                                           # [N,N] float64
            att = torch.exp(score[ri, ci] - torch.logsumexp(score, dim=1)[ri])       # at the stored edges
            del score
            zo[g].index_add_(1, ri, (att * f(wb))[None, :, None] * xg[:, ci, :])
            grad += att * torch.einsum("cet,cet->e", dzg[:, ri, :], xg[:, ci, :])
        dao.append(grad)
    assert_parity(z, zo.cpu().numpy(), "sets n8192", "z")
    assert_parity(vals.grad, torch.cat(dao).cpu().numpy(), "sets n8192", "dval")
