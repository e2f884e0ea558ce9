"""Signal-dependent edge weights (msgat_edge_signal_weights{,_backward}) on one MI355X at the PEMSD7 training shape:
N = 883, the road graph's nnz (2615 with the synthetic graph), B = 32, rank d = 8, F = 36 node features (3 channels x 12
steps), R = 5, msgat72.  HIP events after warm-up, medians over rounds in which the variants alternate; nothing is asserted
except that the variants compute the same thing.

  kernels   w[b,e] = base[e] + <ab[b,row(e),:d], ab[b,col(e),d:]> [B,nnz] forward and its backward under dout [B,nnz] down
            to base and ab [B,N,2d], two formulations: "hip" -- `ops.edge_signal_weights`, one launch each way -- and "torch"
            -- two [B,nnz,d] gathers, a product, `sum(-1)` and an add with torch autograd (a batch sum, two products and two
            index_add_ scatters); and both again with the projection ab = f @ P.T and its backward down to P and f, which
            is torch's in either (one GEMM forward, two backward).  Each is timed
              eager     launched from Python, `calls` forward + backward pairs per event pair (host time included), and
              replayed  as ONE captured HIP graph of a forward + backward (device time: what a captured step sees),
            with cache-resident operands and, replayed only, cold: a 512 MiB buffer (twice the last-level cache) is
            overwritten before every replay and the event pair brackets that one replay.  The two C entry points alone are
            timed as well (`calls` launches per event pair, cache-resident).  Launch counts: the device kernels of one eager
            forward + backward as torch.profiler lists them.
  steps     a whole captured training step (forward, loss, backward, FlatAdam; `engine._GraphedStep`, what
            `Trainer(hip_graph=True)` replays) of msgat72 with learn_edge_weights = False, True, "signal", and "signal" with
            the weights formed by torch ops; `calls` replays per event pair.

    python tools/edge_signal_bench.py [--rounds 7] [--calls 20] [--out profiles/edge_signal] [--kernels | --steps-only]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
from edge_time_bench import LINES, alternate, capture, device_kernels, report, say  # noqa: E402
from ms_gat_amd import _lib, engine, graph, model, ops  # noqa: E402

N, EDGES, B, R, T, CHANNELS, RANK = 883, 866, 32, 5, 12, 3, 8
FEATURES = CHANNELS * T
DEV = torch.device("cuda:0")


def torch_weights(base, ab, rows, col):
    d = ab.shape[-1] // 2
    return base + (ab[:, rows, :d] * ab[:, col, d:]).sum(-1)


def kernels(rounds, calls):
    g = torch.Generator().manual_seed(0)
    pattern = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1).to_sparse_csr()
    crow, col = pattern.crow_indices().to(DEV), pattern.col_indices().to(DEV)
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), crow[1:] - crow[:-1])
    nnz = col.numel()
    base = pattern.values().clone().to(DEV).requires_grad_(True)
    P = (0.1 * torch.randn(2 * RANK, FEATURES, generator=g)).to(DEV).requires_grad_(True)
    f = torch.randn(B, N, FEATURES, generator=g).to(DEV).requires_grad_(True)
    dout = torch.randn(B, nnz, generator=g).to(DEV)
    params = (base, P, f)

    def run(make):
        for p in params:
            p.grad = None
        w = make(f @ P.T)
        w.backward(dout)
        return w

    ab_leaf = (f @ P.T).detach().contiguous().requires_grad_(True)

    def run_edges(make):
        base.grad = ab_leaf.grad = None
        w = make(ab_leaf)
        w.backward(dout)
        return w

    forms = {"hip": lambda: run_edges(lambda ab: ops.edge_signal_weights(base, ab, crow, col)),
             "torch": lambda: run_edges(lambda ab: torch_weights(base, ab, rows, col)),
             "hip, projection included": lambda: run(lambda ab: ops.edge_signal_weights(base, ab, crow, col)),
             "torch, projection included": lambda: run(lambda ab: torch_weights(base, ab, rows, col))}
    # the same thing, to rounding: torch's sum(-1) and its scatters add in no promised order
    w_hip = forms["hip, projection included"]().detach().clone()
    g_hip = [p.grad.clone() for p in params]
    w_torch = forms["torch, projection included"]().detach().clone()
    assert float((w_hip - w_torch).abs().max()) <= 1e-5 * float(w_torch.abs().max())
    for a, p in zip(g_hip, params):
        assert float((a - p.grad).abs().max()) <= 1e-4 * float(p.grad.abs().max())
    say(f"kernels at B={B} N={N} nnz={nnz} d={RANK} F={FEATURES} (ab {B * N * 2 * RANK * 4 / 1e6:.2f} MB, w and dout "
        f"{B * nnz * 4 / 1e6:.2f} MB each), {calls} calls per event pair, {os.path.basename(_lib.LIB_PATH)}")
    say("launch counts (device kernels of one eager forward + backward, torch.profiler):")
    counts = {}
    for k, fn in forms.items():
        names = device_kernels(fn)
        counts[k] = None if names is None else len(names)
        say(f"  {k}: {'not measured' if names is None else len(names)}")
        if names:
            for n in names:
                say(f"      {n[:150]}")
    report("forward + backward, eager launches (host time included), cache-resident operands:", alternate(forms, rounds, calls))
    graphs = {k: capture(fn) for k, fn in forms.items()}
    replays = {k: gr.replay for k, gr in graphs.items()}
    warm = alternate(replays, rounds, calls)
    report("forward + backward, ONE captured graph replayed (device time), cache-resident operands:", warm)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    cold = alternate(replays, max(rounds, 15), 1, warmup=3, before=lambda: flush.add_(1))
    report("forward + backward, ONE captured graph replayed, cold operands (512 MiB overwritten before each replay; one replay "
           "per event pair, so the pair's own resolution of a few us is in the figure):", cold)
    # the two entry points alone
    L, s = _lib.lib(), _lib.stream_handle(DEV)
    gstruct, keep = graph.edge_pattern_of(crow, col).structure.on(DEV)
    ab = (f @ P.T).detach().contiguous()
    out, dbase, dab = torch.empty(B, nnz, device=DEV), torch.empty(nnz, device=DEV), torch.empty_like(ab)
    b0 = base.detach()
    alone = {
        "msgat_edge_signal_weights": lambda: _lib.check(L.msgat_edge_signal_weights(
            gstruct, b0.data_ptr(), ab.data_ptr(), B, RANK, out.data_ptr(), s), "fwd"),
        "msgat_edge_signal_weights_backward": lambda: _lib.check(L.msgat_edge_signal_weights_backward(
            gstruct, dout.data_ptr(), ab.data_ptr(), B, RANK, dbase.data_ptr(), dab.data_ptr(), s), "bwd"),
    }
    single = alternate(alone, rounds, calls)
    report("the entry points alone, back-to-back launches from Python (cache-resident; launch-rate bound where the kernel is "
           "shorter than a launch):", single)
    med = lambda t: {k: round(statistics.median(v), 2) for k, v in t.items()}  # noqa: E731
    return {"B": B, "nnz": nnz, "d": RANK, "launches": counts, "replayed_warm_us": med(warm), "replayed_cold_us": med(cold),
            "entry_points_us": med(single)}


def steps(rounds, calls):
    g = torch.Generator().manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1)
    batch = [torch.randn(B, R, CHANNELS, N, T, generator=g), torch.randint(0, 24, (B,), generator=g),
             torch.randint(0, 7, (B,), generator=g), torch.randn(B, N, T, generator=g)]
    batch = [t.to(DEV) for t in batch]
    out_dir = tempfile.mkdtemp(prefix="edge_signal_bench_")

    def build(learn, torch_ops=False):
        torch.manual_seed(0)
        net = model.msgat72(n_components=R, in_channels=CHANNELS, in_timesteps=T, out_timesteps=T, use_te=True, adj=adj,
                            learn_edge_weights=learn, edge_rank=RANK).to(DEV)
        if learn == "signal":
            tg = torch.Generator().manual_seed(1)     # the same projection in both "signal" configurations
            with torch.no_grad():
                net.edge_proj.weight.copy_((0.1 * torch.randn(net.edge_proj.weight.shape, generator=tg)).to(DEV))
        if torch_ops:
            rows = torch.repeat_interleave(torch.arange(N, device=DEV), net.edge_crow[1:] - net.edge_crow[:-1])
            net.adjacency = lambda H=None, D=None, X=None: ops.edge_adjacency(
                net.edge_crow, net.edge_col, torch_weights(net.edge_weight, net.edge_proj(net.edge_features(X)), rows, net.edge_col))
        trainer = engine.Trainer(net, 50.0, out_dir, hip_graph=True)
        step = engine._GraphedStep(trainer, batch, training=True, step_in_graph=True)
        return net, trainer, step

    configs = {"learn_edge_weights=False": build(False), "learn_edge_weights=True": build(True),
               'learn_edge_weights="signal"': build("signal"), '"signal" from torch ops': build("signal", torch_ops=True)}
    times = alternate({k: v[2].graph.replay for k, v in configs.items()}, rounds, calls, warmup=5)
    say(f"captured training step (forward, loss, backward, FlatAdam) of msgat72, R={R} B={B} C={CHANNELS} N={N} T={T} "
        f"nnz={int((adj != 0).sum())} d={RANK}, {calls} replays per event pair:")
    for k, v in times.items():
        say(f"  {k}: median {statistics.median(v) / 1e3:.4f} ms, fastest {min(v) / 1e3:.4f} ms, slowest {max(v) / 1e3:.4f} ms "
            f"({len(v)} rounds)")
    losses = {k: float(v[2].loss.detach()) for k, v in configs.items()}
    say("  loss of the last replay: " + ", ".join(f"{k} {v:.6g}" for k, v in losses.items()))
    return {k: round(statistics.median(v) / 1e3, 4) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "edge_signal"))
    ap.add_argument("--kernels", action="store_true", help="the kernel timings only")
    ap.add_argument("--steps-only", action="store_true", help="the captured training steps only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_signal_bench.py needs the GPU: there is nothing to time without one")
    say(f"# tools/edge_signal_bench.py --rounds {a.rounds} --calls {a.calls} on {torch.cuda.get_device_name(0)}: HIP events, "
        "medians over rounds, variants alternated inside a round")
    result = {}
    if not a.steps_only:
        result["kernels"] = kernels(a.rounds, a.calls)
    if not a.kernels:
        result["captured_step_ms"] = steps(a.rounds, a.calls)
    say(json.dumps(result))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "edge_signal_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
