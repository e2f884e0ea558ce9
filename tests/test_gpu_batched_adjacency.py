"""GPU: graph attention, GACN, StackedGACN and MEAM with a per-sample adjacency [B,N,N] (attention.py:22).

Parity with the reference's own fixtures (tests/golden/make_golden_batched.py, a different pattern per sample), with a
float64 restatement on the paths those cannot reach (the split bf16 score pass, the SELL kernels, the 7 + 1 score form,
R stacked relations), the shared path bit for bit where the values coincide, and the device refresh of the values
(`BatchedGraph.update_`, the `msgat_graph_edge_values` kernel) eagerly and inside a HIP-graph capture.
"""
import numpy as np
import pytest
import torch

from conftest import assert_parity, load_golden, rel_err
from oracle import dense_torch

import ms_gat_amd
from ms_gat_amd import _lib, ops
from ms_gat_amd.graph import BatchedGraph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _load_module(m, state):
    with torch.no_grad():
        for k, v in state.items():
            m.get_parameter(k).copy_(_dev(v))
    return m.to(DEV)


def _batched_adjacency(B, N, seed, density=None, same_pattern=False):
    """[B,N,N] sym-normalised random graphs, a different edge set (unless same_pattern) and different weights per sample."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, N, N), dtype=np.float32)
    base = ms_gat_amd.synthetic_adjacency(N, N + 6, seed).numpy()
    for b in range(B):
        a = base if same_pattern else ms_gat_amd.synthetic_adjacency(N, N + 6 + 3 * b, seed + 1 + b).numpy()
        out[b] = a * rng.uniform(0.5, 1.5, (N, N)).astype(np.float32)
    return torch.from_numpy(out)


# ---- the reference's fixtures -------------------------------------------------------------------------------------

def test_graph_attention_matches_reference_fixture():
    g = load_golden("batched_gatt_b3c3n64.npz")
    m = _load_module(ms_gat_amd.GraphAttention(3, 12), {"Wg": g["Wg"], "alpha": g["alpha"]})
    x = _dev(g["x"]).requires_grad_(True)
    y = m(x, _dev(g["adj"]))
    y.backward(_dev(g["dy"]))
    for got, key in ((y, "y"), (x.grad, "dx"), (m.Wg.grad, "dWg"), (m.alpha.grad, "dalpha")):
        assert_parity(got, g[key], "batched_gatt_b3c3n64", key)


@pytest.mark.parametrize("name", ["batched_gacn_b3c1n64.npz", "batched_gacn_b3c3n64.npz", "batched_gacn_b2c72n47.npz"])
def test_gacn_matches_reference_fixture(name):
    g = load_golden(name)
    if "x_q32" in g:
        xn, dzn = g["x_q32"].astype(np.float32) / 32, g["dz_q32"].astype(np.float32) / 32
    else:
        xn, dzn = g["x"].astype(np.float32), g["dz"].astype(np.float32)
    C, O = xn.shape[1], g["W"].shape[0]
    m = _load_module(ms_gat_amd.GACN(C, O, 12), {"gatt.Wg": g["Wg"], "gatt.alpha": g["alpha"], "W": g["W"]})
    x = _dev(xn).requires_grad_(True)
    z = m(x, _dev(g["adj"]))
    z.backward(_dev(dzn))
    for got, key in ((z, "z"), (x.grad, "dx"), (m.gatt.Wg.grad, "dWg"), (m.gatt.alpha.grad, "dalpha"), (m.W.grad, "dW")):
        assert_parity(got, g[key], name, key)


def test_meam_matches_reference_fixture():
    g = load_golden("batched_meam_72to72_n32.npz")
    m = ms_gat_amd.MEAM(72, 72, n_nodes=32, n_timesteps=12, dilations=[1, 2])
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")})
    m = m.to(DEV)
    x = _dev(g["x"].astype(np.float32)).requires_grad_(True)
    out = m(x, _dev(g["adj"]))
    out.backward(_dev(g["dout"].astype(np.float32)))
    assert_parity(out, g["out"], "batched_meam_72to72_n32", "out")
    assert_parity(x.grad, g["dx"], "batched_meam_72to72_n32", "dx")
    for k, p in m.named_parameters():
        assert_parity(p.grad, g[f"g.{k}"], "batched_meam_72to72_n32", k)


# ---- float64 restatement where the fixtures do not reach ------------------------------------------------------------

def _gacn_case(B, C, O, N, seed):
    rng = np.random.default_rng(seed)
    T = 12
    x = rng.standard_normal((B, C, N, T)).astype(np.float32)
    Wg = (rng.standard_normal((T, T)) * 0.3).astype(np.float32)
    alpha = rng.uniform(-C ** -0.5, C ** -0.5, C).astype(np.float32)
    W = (rng.standard_normal((O, C)) * 0.2).astype(np.float32)
    dz = rng.standard_normal((B, O, N, T)).astype(np.float32)
    return x, Wg, alpha, W, dz


def _gacn_run(x, Wg, alpha, W, dz, adjacency):
    xs = _dev(x).requires_grad_(True)
    ps = [_dev(a).requires_grad_(True) for a in (alpha, Wg, W)]
    z = ops.gacn(xs, ps[0], ps[1], ps[2], adjacency)
    z.backward(_dev(dz))
    torch.cuda.synchronize()
    return [z.detach(), xs.grad, ps[0].grad, ps[1].grad, ps[2].grad]


def _gacn_oracle(x, Wg, alpha, W, dz, adj):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float64)  # noqa: E731
    xs, Wgs, als, Ws = (d(a).requires_grad_(True) for a in (x, Wg, alpha, W))
    z = dense_torch.gacn_dense(xs, d(adj.numpy()) if torch.is_tensor(adj) else d(adj), Wgs, als, Ws)
    z.backward(d(dz))
    return [z.detach(), xs.grad, als.grad, Wgs.grad, Ws.grad]


NAMES = ("z", "dx", "dalpha", "dWg", "dW")


@pytest.mark.parametrize("form,B,C,N,sell", [
    ("proj_first_n307", 2, 72, 307, "auto"),      # project first at PEMSD4 size (the reference's fixture is at N = 47)
    ("split_bf16_scores", 2, 72, 1536, "auto"),   # N >= 1536: the dense passes on the split bf16 / fp16 matrix core
    ("sell_kernels", 3, 72, 96, "always"),        # the SELL aggregate / SDDMM
    ("sell_kernels_aggfirst", 3, 3, 96, "always"),
    ("scores7_headline", 32, 72, 883, "auto"),    # the 7 + 1 score form at the headline size, 32 groups
])
def test_gacn_against_float64_restatement(form, B, C, N, sell):
    case = _gacn_case(B, C, 24, N, seed=N + B)
    adj = _batched_adjacency(B, N, seed=N)
    bg = BatchedGraph(adj.to(DEV), sell=sell)
    assert bg.n_sets == B and (sell != "always" or bg.has_sell)
    got = _gacn_run(*case, bg)
    want = _gacn_oracle(*case, adj)
    for name, a, b in zip(NAMES, got, want):
        assert_parity(a, b.cpu().numpy(), f"batched_{form}", name)


@pytest.mark.parametrize("per_group", [False, True])
def test_stacked_gacn_three_relations(per_group):
    R, B, C, O, N, T = 3, 2, 72, 24, 64, 12
    rng = np.random.default_rng(7)
    m = ms_gat_amd.StackedGACN(R, C, O, T)
    with torch.no_grad():
        m.Wg.copy_(torch.randn(R, T, T) * 0.3)
        m.alpha.uniform_(-C ** -0.5, C ** -0.5)
        m.W.copy_(torch.randn(R, O, C) * 0.2)
    m = m.to(DEV)
    adj = _batched_adjacency(R * B if per_group else B, N, seed=11)
    x = torch.from_numpy(rng.standard_normal((R, B, C, N, T)).astype(np.float32)).to(DEV).requires_grad_(True)
    dz = torch.from_numpy(rng.standard_normal((R, B, O, N, T)).astype(np.float32)).to(DEV)
    z = m(x, adj.to(DEV))
    z.backward(dz)
    for r in range(R):
        a = adj[r * B:(r + 1) * B] if per_group else adj
        want = _gacn_oracle(x[r].detach().cpu().numpy(), m.Wg[r].detach().cpu().numpy(), m.alpha[r].detach().cpu().numpy(),
                            m.W[r].detach().cpu().numpy(), dz[r].cpu().numpy(), a)
        got = [z[r].detach(), x.grad[r], m.alpha.grad[r], m.Wg.grad[r], m.W.grad[r]]
        for name, g_, w in zip(NAMES, got, want):
            assert_parity(g_, w.cpu().numpy(), f"batched_stacked_r{r}_{'group' if per_group else 'sample'}", name)


# ---- the shared path where the values coincide ----------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3, 72])
def test_identical_slices_equal_the_shared_path_bit_for_bit(C):
    B, N = 4, 307
    case = _gacn_case(B, C, 24, N, seed=C)
    adj = ms_gat_amd.synthetic_adjacency(N, 340, seed=C).to(DEV)
    shared = _gacn_run(*case, adj)
    batched = _gacn_run(*case, adj.expand(B, N, N))             # non-contiguous: made contiguous before the kernel reads it
    one = _gacn_run(*case, adj.unsqueeze(0).clone())            # [1,N,N] is the shared path
    for name, a, b, c in zip(NAMES, shared, batched, one):
        assert torch.equal(a, b), f"[B,N,N] of identical slices, {name}"
        assert torch.equal(a, c), f"[1,N,N], {name}"


def test_each_sample_equals_a_single_sample_call():
    B, C, N = 3, 72, 200
    x, Wg, alpha, W, dz = _gacn_case(B, C, 24, N, seed=5)
    adj = _batched_adjacency(B, N, seed=5).to(DEV)
    z = _gacn_run(x, Wg, alpha, W, dz, adj)[0]
    for b in range(B):
        zb = _gacn_run(x[b:b + 1], Wg, alpha, W, dz[b:b + 1], adj[b])[0]
        assert rel_err(z[b], zb[0]) < 1e-5, b


def test_all_zero_sample_gives_zero_output_and_finite_gradients():
    B, C, N = 3, 3, 64
    case = _gacn_case(B, C, 24, N, seed=9)
    adj = _batched_adjacency(B, N, seed=9)
    adj[1] = 0
    got = _gacn_run(*case, adj.to(DEV))
    assert torch.count_nonzero(got[0][1]) == 0
    assert torch.count_nonzero(got[1][1]) == 0                  # that sample's dx: nothing reaches it
    for name, t in zip(NAMES, got):
        assert torch.isfinite(t).all(), name
    want = _gacn_oracle(*case, adj)
    for name, a, b in zip(NAMES, got, want):
        assert_parity(a, b.cpu().numpy(), "batched_zero_sample", name)


# ---- the device refresh ---------------------------------------------------------------------------------------------

def test_edge_values_kernel_fills_values_and_counts_edges_outside_the_pattern():
    for N in (61, 64, 883):      # rows that start off a 16-B boundary, and ones that do not
        adj = _batched_adjacency(5, N, seed=N).to(DEV)
        g = BatchedGraph(adj)
        host = BatchedGraph(adj.cpu())
        assert torch.equal(g.val.cpu(), host.val)
        g.check()
        bad = adj.clone()
        free = (~(adj != 0).any(0)).nonzero()
        bad[0, free[0, 0], free[0, 1]] = 0.25
        bad[4, free[-1, 0], free[-1, 1]] = float("nan")
        g.update_(bad)
        assert g.outside() == 2
        with pytest.raises(_lib.MsgatError, match="outside"):
            g.check()


def test_batched_graph_of_rebuilds_the_pattern_when_edges_fall_outside():
    N = 50
    a = _batched_adjacency(2, N, seed=1).to(DEV)
    g1 = ms_gat_amd.batched_graph_of(a)
    b = _batched_adjacency(2, N, seed=2).to(DEV)                # another pattern: the known one misses edges
    g2 = ms_gat_amd.batched_graph_of(b)
    g2.check()
    assert torch.equal(g2.dense(), b.cpu())
    c = a * 3.0                                                 # the first pattern again: no rebuild, own values
    g3 = ms_gat_amd.batched_graph_of(c)
    assert g3.val.data_ptr() not in (g1.val.data_ptr(), g2.val.data_ptr())
    assert torch.equal(g3.dense(), c.cpu())


def test_hip_graph_capture_with_refresh_matches_eager_bit_for_bit():
    B, C, O, N = 4, 72, 24, 307
    x, Wg, alpha, W, dz = _gacn_case(B, C, O, N, seed=13)
    weightings = [_batched_adjacency(B, N, seed=13, same_pattern=True).to(DEV) for _ in range(3)]
    for k in range(3):
        weightings[k] = weightings[k] * (1.0 + 0.25 * k)
    # eager references, each through its own BatchedGraph
    eager = [_gacn_run(x, Wg, alpha, W, dz, BatchedGraph(w)) for w in weightings]

    static_adj = weightings[0].clone()
    bg = BatchedGraph(static_adj)
    xs = _dev(x).requires_grad_(True)
    ps = [_dev(a).requires_grad_(True) for a in (alpha, Wg, W)]
    dzs = _dev(dz)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                 # warm-up: plans, workspaces
        for _ in range(2):
            bg.update_(static_adj)
            ops.gacn(xs, ps[0], ps[1], ps[2], bg).backward(dzs)
    torch.cuda.current_stream().wait_stream(side)
    for t in [xs] + ps:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bg.update_(static_adj)
        z = ops.gacn(xs, ps[0], ps[1], ps[2], bg)
        z.backward(dzs)
    grads = [xs.grad] + [p.grad for p in ps]
    for w, want in zip(weightings, eager):
        static_adj.copy_(w)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(NAMES, [z] + grads, want):
            assert torch.equal(a, b), name
    assert bg.outside() == 0
