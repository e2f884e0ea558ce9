"""GPU: a gradient at the dense softmax map (`weights="softmax_grad"`, msgat_softmax_map_grad): the loss <dY, y> + <dP, att>
with a dense random dP against a float64 torch-autograd restatement of the reference (attention.py:33-36, msgat.py:25-28)
and against the reference's own fixtures (tests/golden/make_golden_softmax_grad.py), in every mode and lead shape; the
plain path left bit for bit as it was; determinism; the whole model through `collect_weights`; HIP-graph capture.
"""
import numpy as np
import pytest
import torch

from conftest import assert_parity, load_golden

import ms_gat_amd
from ms_gat_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WHAT = "softmax_grad"


def _rng(seed):
    return np.random.default_rng(seed)


def _adjacency(N, seed):
    a = ms_gat_amd.synthetic_adjacency(N, 3 * N, seed=seed).numpy().copy()
    a = a * _rng(seed + 7).uniform(0.5, 1.5, a.shape)           # asymmetric weights
    a[N // 3, :] = 0.0                                           # a row without edges
    return a.astype(np.float32)


def _params(C, Co, T, seed, R=None):
    r = _rng(seed)
    lead = () if R is None else (R,)
    p = {"Wg": (r.standard_normal(lead + (T, T)) * 0.3).astype(np.float32),
         "alpha": r.uniform(-C ** -0.5, C ** -0.5, lead + (C,)).astype(np.float32)}
    if Co:
        p["W"] = (r.standard_normal(lead + (Co, C)) * 0.2).astype(np.float32)
    return p


def _ref(x, alpha, Wg, W, adj):
    """float64 restatement of attention.py:33-36 (+ msgat.py:27) for one relation: (y, att)."""
    q = torch.einsum("c,bcnt->bnt", alpha, x)
    att = torch.softmax(torch.einsum("bnt,ts,bms->bnm", q, Wg, q), dim=-1)
    y = torch.einsum("bnm,bcmt->bcnt", att * adj, x)
    if W is not None:
        y = torch.einsum("oc,bcnt->bont", W, y)
    return y, att


def _ref_grads(x, p, adj, dY, dP):
    t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in p.items()}
    xt = torch.from_numpy(x).double().requires_grad_(True)
    y, att = _ref(xt, t["alpha"], t["Wg"], t.get("W"), torch.from_numpy(adj).double())
    ((y * torch.from_numpy(dY).double()).sum() + (att * torch.from_numpy(dP).double()).sum()).backward()
    out = {"y": y.detach().numpy(), "att": att.detach().numpy(), "dx": xt.grad.numpy()}
    for k, v in t.items():
        out["d" + k] = v.grad.numpy()
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float32)


def _module(C, Co, T, p):
    m = ms_gat_amd.GACN(C, Co, T) if Co else ms_gat_amd.GraphAttention(C, T)
    prefix = "gatt." if Co else ""
    with torch.no_grad():
        for k, v in p.items():
            m.get_parameter(("" if k == "W" else prefix) + k).copy_(torch.from_numpy(v))
    return m.to(DEV)


def _grads(m, Co):
    g = {"dWg": (m.gatt.Wg if Co else m.Wg).grad, "dalpha": (m.gatt.alpha if Co else m.alpha).grad}
    if Co:
        g["dW"] = m.W.grad
    return g


def _case(C, Co, N, B, T, seed):
    r = _rng(seed)
    p = _params(C, Co, T, seed=seed + 1)
    adj = _adjacency(N, seed=seed + 2)
    x = r.standard_normal((B, C, N, T)).astype(np.float32)
    dY = r.standard_normal((B, Co or C, N, T)).astype(np.float32)
    dP = r.standard_normal((B, N, N)).astype(np.float32)
    return p, adj, x, dY, dP


def _run(C, Co, T, p, adj, x, dY, dP, map_term=True, y_term=True, weights="softmax_grad", adj_grad=False):
    """One forward + backward of the module: (y, map, x.grad, parameter grads, adjacency grad or None)."""
    m = _module(C, Co, T, p)
    xt = _dev(x).requires_grad_(True)
    at = _dev(adj).requires_grad_(adj_grad)
    if weights is None:
        y, w = m(xt, at), None
    else:
        y, w = m(xt, at, need_weights=True, weights=weights)
    loss = 0
    if y_term:
        loss = loss + (y * _dev(dY)).sum()
    if map_term:
        loss = loss + (w * _dev(dP)).sum()
    loss.backward()
    return y, w, xt.grad, _grads(m, Co), at.grad


# ---- the reference's fixtures ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,C,Co", [("attp_gatt_b2c3n64.npz", 3, 0), ("attp_gacn_b2c72n47.npz", 72, 24)])
def test_reference_fixtures(name, C, Co):
    g = load_golden(name)
    if "x_q32" in g:
        x, dY = g["x_q32"].astype(np.float32) / 32, g["dy_q32"].astype(np.float32) / 32
    else:
        x, dY = g["x"].astype(np.float32), g["dy"].astype(np.float32)
    p = {k: g[k] for k in ("Wg", "alpha", "W") if k in g}
    y, w, dx, grads, _ = _run(C, Co, 12, p, g["adj"], x, dY, g["dP"].astype(np.float32))
    assert w.requires_grad and not w.is_sparse and tuple(w.shape) == g["att"].shape
    assert_parity(y, g["y"], WHAT, name + ":y")
    assert_parity(w, g["att"], WHAT, name + ":att")
    assert_parity(dx, g["dx"], WHAT, name + ":dx")
    for k, v in grads.items():
        assert_parity(v, g[k], WHAT, f"{name}:{k}")


# ---- float64 autograd, every mode, T and the large-N side of the lse threshold -------------------------------------

@pytest.mark.parametrize("C,Co,N,B,T", [
    (3, 0, 47, 2, 12),      # plain mode, N % 4 != 0, one partial tile
    (3, 24, 64, 2, 12),     # aggregate first
    (72, 24, 130, 2, 12),   # project first, three 64-tiles with remainders on both axes
    (3, 0, 33, 2, 4), (3, 0, 33, 2, 8), (3, 0, 33, 2, 16),   # every supported T
    (1, 0, 1600, 1, 12),    # lse from the split-operand scores (N >= 1536), N % 4 == 0: 16-byte reads of dP
])
def test_map_gradient_against_float64(C, Co, N, B, T):
    p, adj, x, dY, dP = _case(C, Co, N, B, T, seed=N + C + T)
    want = _ref_grads(x, p, adj, dY, dP)
    y, w, dx, grads, _ = _run(C, Co, T, p, adj, x, dY, dP)
    key = f"C{C}_Co{Co}_N{N}_T{T}"
    assert_parity(y, want["y"], WHAT, key + ":y")
    assert_parity(w, want["att"], WHAT, key + ":att")
    assert_parity(dx, want["dx"], WHAT, key + ":dx")
    for k, v in grads.items():
        assert_parity(v, want[k], WHAT, f"{key}:{k}")


def test_attention_core_map_gradient():
    """`dq` and `du` are outputs; dWg is reduced per relation (Wg [2,T,T], G = 4)."""
    Cu, N, G, R, T = 24, 64, 4, 2, 12
    r = _rng(77)
    u = r.standard_normal((G, Cu, N, T)).astype(np.float32)
    q = (r.standard_normal((G, N, T)) * 0.5).astype(np.float32)
    Wg = (r.standard_normal((R, T, T)) * 0.3).astype(np.float32)
    adj = _adjacency(N, seed=78)
    dY = r.standard_normal((G, Cu, N, T)).astype(np.float32)
    dP = r.standard_normal((G, N, N)).astype(np.float32)

    ud, qd, Wd = (torch.from_numpy(a).double().requires_grad_(True) for a in (u, q, Wg))
    Wgg = Wd.repeat_interleave(G // R, dim=0)                   # relation-major groups
    att = torch.softmax(torch.einsum("gnt,gts,gms->gnm", qd, Wgg, qd), dim=-1)
    y = torch.einsum("gnm,gcmt->gcnt", att * torch.from_numpy(adj).double(), ud)
    ((y * torch.from_numpy(dY).double()).sum() + (att * torch.from_numpy(dP).double()).sum()).backward()

    ut, qt, Wt = (_dev(a).requires_grad_(True) for a in (u, q, Wg))
    z, w = ops.attention_core(ut, qt, Wt, _dev(adj), need_weights=True, weights="softmax_grad")
    ((z * _dev(dY)).sum() + (w * _dev(dP)).sum()).backward()
    assert_parity(z, y.detach().numpy(), WHAT, "core:y")
    assert_parity(w, att.detach().numpy(), WHAT, "core:att")
    assert_parity(ut.grad, ud.grad.numpy(), WHAT, "core:du")
    assert_parity(qt.grad, qd.grad.numpy(), WHAT, "core:dq")
    assert_parity(Wt.grad, Wd.grad.numpy(), WHAT, "core:dWg")


def test_stacked_gacn_map_gradient():
    """Lead shape (R, Bg): the map is [R,Bg,N,N] and every relation's parameters get their own share."""
    R, Bg, C, Co, N, T = 2, 2, 3, 24, 47, 12
    r = _rng(91)
    p = _params(C, Co, T, seed=92, R=R)
    adj = _adjacency(N, seed=93)
    x = r.standard_normal((R, Bg, C, N, T)).astype(np.float32)
    dY = r.standard_normal((R, Bg, Co, N, T)).astype(np.float32)
    dP = r.standard_normal((R, Bg, N, N)).astype(np.float32)
    m = ms_gat_amd.StackedGACN(R, C, Co, T)
    with torch.no_grad():
        for k, v in p.items():
            m.get_parameter(k).copy_(torch.from_numpy(v))
    m = m.to(DEV)
    xt = _dev(x).requires_grad_(True)
    y, w = m(xt, _dev(adj), need_weights=True, weights="softmax_grad")
    assert tuple(w.shape) == (R, Bg, N, N) and w.requires_grad
    ((y * _dev(dY)).sum() + (w * _dev(dP)).sum()).backward()
    for rel in range(R):
        want = _ref_grads(x[rel], {k: v[rel] for k, v in p.items()}, adj, dY[rel], dP[rel])
        assert_parity(y[rel], want["y"], WHAT, f"stacked{rel}:y")
        assert_parity(w[rel], want["att"], WHAT, f"stacked{rel}:att")
        assert_parity(xt.grad[rel], want["dx"], WHAT, f"stacked{rel}:dx")
        for k in p:
            assert_parity(m.get_parameter(k).grad[rel], want["d" + k], WHAT, f"stacked{rel}:d{k}")


# ---- what the map's term must not touch --------------------------------------------------------------------------

def test_loss_on_the_map_alone():
    """dz is None: x, alpha, Wg get the map's term, W nothing; a dense adjacency that requires grad gets exactly what it
    gets without the term on the map."""
    C, Co, N, B, T = 3, 24, 64, 2, 12
    p, adj, x, dY, dP = _case(C, Co, N, B, T, seed=5)
    want = _ref_grads(x, p, adj, np.zeros_like(dY), dP)
    _, _, dx, grads, _ = _run(C, Co, T, p, adj, x, dY, dP, y_term=False)
    assert_parity(dx, want["dx"], WHAT, "map_only:dx")
    assert_parity(grads["dWg"], want["dWg"], WHAT, "map_only:dWg")
    assert_parity(grads["dalpha"], want["dalpha"], WHAT, "map_only:dalpha")
    assert grads["dW"] is None or not torch.any(grads["dW"])
    _, _, _, _, a_both = _run(C, Co, T, p, adj, x, dY, dP, adj_grad=True)
    _, _, _, _, a_y = _run(C, Co, T, p, adj, x, dY, dP, map_term=False, adj_grad=True)
    assert a_both is not None and torch.equal(a_both, a_y)


@pytest.mark.parametrize("C,Co,N", [(3, 0, 47), (3, 24, 64), (72, 24, 47)])
def test_plain_path_is_untouched(C, Co, N):
    """A loss on y only: the map's gradient arrives as None and backward is the plain one, bit for bit; the map is the
    `weights="softmax"` tensor, and an in-place edit of it does not reach backward.

    The two forms are compared bit for bit where both can be called, under no_grad: "softmax" refuses a recording
    forward, and a recording forward forms lse inside the payload product that also gives pq (dense.hip, WITH_PQ), in
    another summation order than the inference forward, so its map differs from a no_grad map in the last bits whatever
    the form (the test prints the figure).  Against that map the recording one is held to assert_parity."""
    B, T = 2, 12
    p, adj, x, dY, dP = _case(C, Co, N, B, T, seed=11 + C)
    y0, _, dx0, g0, _ = _run(C, Co, T, p, adj, x, dY, dP, map_term=False, weights=None)
    y1, w1, dx1, g1, _ = _run(C, Co, T, p, adj, x, dY, dP, map_term=False)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    m = _module(C, Co, T, p)
    with torch.no_grad():
        y2, w2 = m(_dev(x), _dev(adj), need_weights=True, weights="softmax")
        y3, w3 = m(_dev(x), _dev(adj), need_weights=True, weights="softmax_grad")
    assert torch.equal(w3, w2) and torch.equal(y3, y2) and not w3.requires_grad
    print(f"recording vs no_grad map, C={C} Co={Co} N={N}: max|diff| / max = {float((w1.detach() - w2).abs().max() / w2.abs().max()):.2e}")
    assert_parity(w1, w2.cpu().numpy(), WHAT, f"plain_C{C}_Co{Co}_N{N}:map_recording_vs_no_grad")
    # backward re-creates P from q, kW, lse: scribbling over the returned map changes nothing
    _, _, dx_a, g_a, _ = _run(C, Co, T, p, adj, x, dY, dP)
    m = _module(C, Co, T, p)
    xt = _dev(x).requires_grad_(True)
    y, w = m(xt, _dev(adj), need_weights=True, weights="softmax_grad")
    loss = (y * _dev(dY)).sum() + (w * _dev(dP)).sum()
    w.detach().zero_()
    loss.backward()
    assert torch.equal(xt.grad, dx_a)
    for k, v in _grads(m, Co).items():
        assert torch.equal(v, g_a[k]), k


def test_two_runs_are_bit_identical():
    C, Co, N, B, T = 72, 24, 130, 2, 12
    p, adj, x, dY, dP = _case(C, Co, N, B, T, seed=21)
    _, w0, dx0, g0, _ = _run(C, Co, T, p, adj, x, dY, dP)
    _, w1, dx1, g1, _ = _run(C, Co, T, p, adj, x, dY, dP)
    assert torch.equal(w0, w1) and torch.equal(dx0, dx1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ---- the whole model -------------------------------------------------------------------------------------------

def test_collect_weights_regulariser_on_both_paths():
    """pred.sum() + sum over every block's map of (map ** 2).sum(), on the stacked path and the component loop: the
    attention parameters of every GACN get the same gradient."""
    N, B, R, T = 32, 2, 3, 12
    adj = torch.from_numpy(_adjacency(N, seed=21))
    torch.manual_seed(0)
    model = ms_gat_amd.msgat72(n_components=R, in_channels=1, in_timesteps=T, out_timesteps=T, use_te=True, adj=adj).to(DEV)
    X = torch.randn(B, R, 1, N, T, device=DEV)
    H = torch.randint(0, 24, (B,), device=DEV)
    D = torch.randint(0, 7, (B,), device=DEV)
    keys = [f"tpcs.{r}.tgacns.{l}.gacn.gatt" for r in range(R) for l in range(2)]
    got = {}
    for stacked in (True, False):
        model.stack_components = stacked
        model.zero_grad(set_to_none=True)
        with ops.collect_weights("softmax_grad") as seen:
            pred = model(X, H, D)
        assert len(seen) > 0
        maps = [w for w, _ in seen]
        assert all(w.requires_grad and w.dim() == 3 and tuple(w.shape[1:]) == (N, N) for w in maps)
        assert sum(w.shape[0] for w in maps) == 2 * R * B
        (pred.sum() + sum((w * w).sum() for w in maps)).backward()
        got[stacked] = {k: (model.get_submodule(k).Wg.grad.clone(), model.get_submodule(k).alpha.grad.clone()) for k in keys}
    for k in keys:
        assert torch.any(got[False][k][0]) and torch.any(got[False][k][1])
        assert_parity(got[True][k][0], got[False][k][0].cpu().numpy(), WHAT, f"model:{k}.Wg")
        assert_parity(got[True][k][1], got[False][k][1].cpu().numpy(), WHAT, f"model:{k}.alpha")


# ---- HIP-graph capture -----------------------------------------------------------------------------------------

def test_hip_graph_capture_replays_the_eager_gradients():
    """One forward + backward with the map term in a captured graph, replayed twice.  The gradients dY and dP enter
    through `torch.autograd.backward`; the capture then holds the library's launches and torch's element-wise kernels,
    one after the other on one stream.  No output of the eager warm-up may outlive it: its autograd graph would keep the
    leaves' gradient accumulators, which belong to the stream they were made on, and the captured backward would then
    reach across to that stream."""
    C, Co, N, B, T = 72, 24, 130, 2, 12
    p, adj, x, dY, dP = _case(C, Co, N, B, T, seed=31)
    m = _module(C, Co, T, p)
    xs = _dev(x).requires_grad_(True)
    at, dYs, dPs = _dev(adj), _dev(dY), _dev(dP)
    leaves = [xs, m.gatt.Wg, m.gatt.alpha, m.W]

    def forward_backward():
        y, w = m(xs, at, need_weights=True, weights="softmax_grad")
        torch.autograd.backward([y, w], [dYs, dPs])

    def step():
        for t in leaves:
            t.grad.zero_()
        forward_backward()

    forward_backward()                   # warm-up: the graph is built, the grads exist
    eager = [t.grad.detach().clone() for t in leaves]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        for t in leaves:
            t.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for t, e in zip(leaves, eager):
            assert torch.equal(t.grad, e)
