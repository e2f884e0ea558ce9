"""GPU: the gradient of the adjacency (attention.py:36 with an adjacency that requires grad; msgat_adjacency_grad).

Parity with the reference's own fixtures (tests/golden/make_golden_adjacency.py) for graph attention, both GACN modes, a
per-sample adjacency and the MEAM (attention core, its gradient arriving as a channel slice); float64 autograd of the
dense restatement at the headline size, N = 307, the other T and the split-operand dense size; every adjacency shape;
the frozen path left bit for bit as it was; determinism; and a HIP-graph capture.
"""
import numpy as np
import pytest
import torch

from conftest import assert_parity, load_golden
from oracle import dense_torch

import ms_gat_amd
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


def _inputs(g):
    if "x_q32" in g:
        return g["x_q32"].astype(np.float32) / 32, g["dz_q32"].astype(np.float32) / 32
    return g["x"].astype(np.float32), g["dz"].astype(np.float32)


def _assert_dense_off_edges(dadj, adj, what):
    """An implementation that only fills the edges fails this: the gradient is P * H, non-zero where adj == 0."""
    d = dadj.detach().cpu().numpy()
    off = np.abs(d[adj == 0])
    assert off.size > 0 and np.mean(off > 1e-5 * np.abs(d).max()) > 0.9, what


# ---- the reference's fixtures -------------------------------------------------------------------------------------

def test_graph_attention_matches_reference_fixture():
    g = load_golden("adjgrad_gatt_b2c3n64.npz")
    m = _load_module(ms_gat_amd.GraphAttention(3, 12), {"Wg": g["Wg"], "alpha": g["alpha"]})
    x = _dev(g["x"]).requires_grad_(True)
    adj = _dev(g["adj"]).requires_grad_(True)
    y = m(x, adj)
    y.backward(_dev(g["dy"]))
    for got, key in ((y, "y"), (x.grad, "dx"), (m.Wg.grad, "dWg"), (m.alpha.grad, "dalpha"), (adj.grad, "dadj")):
        assert_parity(got, g[key], "adjgrad_gatt_b2c3n64", key)
    _assert_dense_off_edges(adj.grad, g["adj"], "gatt")


@pytest.mark.parametrize("name", ["adjgrad_gacn_b2c3n64.npz", "adjgrad_gacn_b2c72n47.npz", "adjgrad_gacn_b3c3n64_bnn.npz"])
def test_gacn_matches_reference_fixture(name):
    g = load_golden(name)
    xn, dzn = _inputs(g)
    C, O = xn.shape[1], g["W"].shape[0]
    m = _load_module(ms_gat_amd.GACN(C, O, 12), {"gatt.Wg": g["Wg"], "gatt.alpha": g["alpha"], "W": g["W"]})
    x = _dev(xn).requires_grad_(True)
    adj = _dev(g["adj"]).requires_grad_(True)
    z = m(x, adj)
    z.backward(_dev(dzn))
    for got, key in ((z, "z"), (x.grad, "dx"), (m.gatt.Wg.grad, "dWg"), (m.gatt.alpha.grad, "dalpha"), (m.W.grad, "dW"),
                     (adj.grad, "dadj")):
        assert_parity(got, g[key], name, key)
    assert tuple(adj.grad.shape) == g["adj"].shape
    _assert_dense_off_edges(adj.grad, g["adj"], name)


def test_meam_matches_reference_fixture():
    g = load_golden("adjgrad_meam_72to72_n32.npz")
    m = ms_gat_amd.MEAM(72, 72, n_nodes=32, n_timesteps=12, dilations=[1, 2])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")})
    m = m.to(DEV)
    x = _dev(g["x"].astype(np.float32)).requires_grad_(True)
    adj = _dev(g["adj"]).requires_grad_(True)
    out = m(x, adj)
    out.backward(_dev(g["dout"].astype(np.float32)))
    assert_parity(out, g["out"], "adjgrad_meam_72to72_n32", "out")
    assert_parity(x.grad, g["dx"], "adjgrad_meam_72to72_n32", "dx")
    assert_parity(adj.grad, g["dadj"], "adjgrad_meam_72to72_n32", "dadj")
    for k, p in m.named_parameters():
        assert_parity(p.grad, g[f"g.{k}"], "adjgrad_meam_72to72_n32", k)


# ---- float64 autograd of the dense restatement --------------------------------------------------------------------

def _learned_adjacency(N, seed, V=None):
    """sym-normalised random graph(s) times independent weights per direction: asymmetric, zeros off the pattern"""
    rng = np.random.default_rng(seed)
    out = []
    for v in range(V or 1):
        a = ms_gat_amd.synthetic_adjacency(N, N + 6 + 3 * v, seed + v).numpy()
        out.append(a * rng.uniform(0.25, 1.5, (N, N)).astype(np.float32))
    return np.stack(out) if V else out[0]


def _case(B, C, O, N, T, seed, R=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R * B, C, N, T)).astype(np.float32)
    dz = rng.standard_normal((R * B, O or C, N, T)).astype(np.float32)
    Wg = (rng.standard_normal((R, T, T)) * (1.0 / T) ** 0.5).astype(np.float32)
    alpha = rng.uniform(-C ** -0.5, C ** -0.5, (R, C)).astype(np.float32)
    W = (rng.standard_normal((R, O, C)) * (2.0 / (O + C)) ** 0.5).astype(np.float32) if O else None
    return x, dz, Wg, alpha, W


def _oracle_dadj(x, dz, Wg, alpha, W, adj, R=1):
    """float64 autograd of gacn_dense / graph_attention_dense, relation by relation; adj [N,N], [B,N,N] or [R*B,N,N]"""
    a = torch.from_numpy(adj).to(DEV, torch.float64).requires_grad_(True)
    G = x.shape[0]
    B = G // R
    outs = []
    for r in range(R):
        xr = torch.from_numpy(x[r * B:(r + 1) * B]).to(DEV, torch.float64)
        ar = a[r * B:(r + 1) * B] if adj.ndim == 3 and adj.shape[0] == G and G != B else a
        Wgr, alr = (torch.from_numpy(t[r]).to(DEV, torch.float64) for t in (Wg, alpha))
        if W is None:
            outs.append(dense_torch.graph_attention_dense(xr, ar, Wgr, alr))
        else:
            outs.append(dense_torch.gacn_dense(xr, ar, Wgr, alr, torch.from_numpy(W[r]).to(DEV, torch.float64)))
    torch.cat(outs).backward(torch.from_numpy(dz).to(DEV, torch.float64))
    return a.grad


def _ours(x, dz, Wg, alpha, W, adj, adj_grad=True, params_grad=True):
    xt = _dev(x).requires_grad_(params_grad)
    ps = [_dev(t).requires_grad_(params_grad) for t in (alpha, Wg)] + ([_dev(W).requires_grad_(params_grad)] if W is not None else [None])
    a = _dev(adj).requires_grad_(adj_grad)
    z = ops.gacn(xt, ps[0], ps[1], ps[2], a)
    z.backward(_dev(dz))
    return z, xt, ps, a


@pytest.mark.parametrize("B,C,O,N,T", [
    (2, 72, 24, 883, 12),    # the headline GACN, project first
    (2, 72, 24, 307, 12),
    (2, 3, 24, 307, 12),     # aggregate first
    (2, 3, 0, 307, 12),      # plain graph attention
    (2, 72, 24, 64, 4),
    (2, 3, 24, 64, 8),
    (2, 72, 24, 64, 16),
    (1, 72, 24, 1600, 12),   # the split-operand dense passes in the forward
])
def test_against_float64_oracle(B, C, O, N, T):
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=N + T + C)
    adj = _learned_adjacency(N, seed=N)
    _, _, _, a = _ours(x, dz, Wg, alpha, W, adj)
    assert_parity(a.grad, _oracle_dadj(x, dz, Wg, alpha, W, adj).cpu().numpy(), f"adjgrad_b{B}c{C}o{O}n{N}t{T}", "dadj")
    _assert_dense_off_edges(a.grad, adj, "oracle")


@pytest.mark.parametrize("form", ["1nn", "bnn", "rbnn"])
def test_every_adjacency_shape(form):
    R, B, C, O, N, T = 3, 2, 72, 24, 64, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=7, R=R)
    V = {"1nn": 1, "bnn": B, "rbnn": R * B}[form]
    adj = _learned_adjacency(N, seed=11, V=V)
    m = ms_gat_amd.StackedGACN(R, C, O, T).to(DEV)
    with torch.no_grad():
        m.Wg.copy_(_dev(Wg))
        m.alpha.copy_(_dev(alpha))
        m.W.copy_(_dev(W))
    a = _dev(adj).requires_grad_(True)
    z = m(_dev(x).view(R, B, C, N, T), a)
    z.backward(_dev(dz).view(R, B, O, N, T))
    assert tuple(a.grad.shape) == adj.shape
    if form == "rbnn":
        want = _oracle_dadj(x, dz, Wg, alpha, W, adj, R=R)
    else:
        # one set per sample (or one for all), shared by the R relations: the relations' gradients add
        want = sum(_oracle_dadj(x[r * B:(r + 1) * B], dz[r * B:(r + 1) * B], Wg[r:r + 1], alpha[r:r + 1], W[r:r + 1], adj)
                   for r in range(R))
    assert_parity(a.grad, want.cpu().numpy(), f"adjgrad_stacked_{form}", "dadj")


def test_frozen_results_are_bit_identical_and_only_the_adjacency_may_require_grad():
    B, C, O, N, T = 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=3)
    adj = _learned_adjacency(N, seed=5)
    z0, x0, p0, _ = _ours(x, dz, Wg, alpha, W, adj, adj_grad=False)
    z1, x1, p1, a1 = _ours(x, dz, Wg, alpha, W, adj, adj_grad=True)
    assert torch.equal(z0, z1)
    assert torch.equal(x0.grad, x1.grad)
    for u, v in zip(p0, p1):
        assert torch.equal(u.grad, v.grad)
    # parameters and signals frozen: the adjacency still gets its gradient, the same bits
    _, _, _, a2 = _ours(x, dz, Wg, alpha, W, adj, adj_grad=True, params_grad=False)
    assert a2.grad is not None and torch.equal(a2.grad, a1.grad)
    # two runs: the same bits (no atomics)
    _, _, _, a3 = _ours(x, dz, Wg, alpha, W, adj, adj_grad=True)
    assert torch.equal(a3.grad, a1.grad)
    # a [1,N,N] adjacency gets a [1,N,N] gradient, the same bits as [N,N]
    _, _, _, a4 = _ours(x, dz, Wg, alpha, W, adj[None], adj_grad=True)
    assert tuple(a4.grad.shape) == (1, N, N) and torch.equal(a4.grad[0], a1.grad)


def test_hip_graph_capture_replays_the_eager_gradient():
    B, C, O, N, T = 2, 72, 24, 307, 12
    x, dz, Wg, alpha, W = _case(B, C, O, N, T, seed=9)
    m = ms_gat_amd.GACN(C, O, T)
    m = _load_module(m, {"gatt.Wg": Wg[0], "gatt.alpha": alpha[0], "W": W[0]})
    adj = torch.nn.Parameter(_dev(_learned_adjacency(N, seed=13)))
    xs, dzs = _dev(x), _dev(dz)

    def step():
        m.zero_grad(set_to_none=False)
        adj.grad.zero_()
        m(xs, adj).backward(dzs)

    m(xs, adj).backward(dzs)             # warm-up: the graph is built, the grads exist
    eager = adj.grad.detach().clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    adj.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(adj.grad, eager)
