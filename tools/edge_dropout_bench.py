"""Edge dropout (msgat_edge_dropout{,_backward}) on one MI355X at the PEMSD7 training shape: N = 883, the road graph's nnz
(2615 with the synthetic graph), B = 32, R = 5, msgat72.  HIP events after warm-up, medians over rounds in which the
variants alternate; nothing is asserted except what the variants must share (shapes, the drop rate, the scale).

  kernels   out = w * m [B,nnz] forward and its backward under dout [B,nnz], for w [nnz] shared by the samples (the
            backward includes the batch sum) and for w [B,nnz], two formulations:
            "hip" -- `ops.edge_dropout`: the draw and the multiply in one launch and a one-thread launch that advances the
            step; backward one launch that re-creates the mask -- and "torch" -- `torch.rand`, a compare, a select and a
            multiply with torch autograd (the mask tensor is kept for the backward's multiply and batch sum).  Each is timed
              eager     launched from Python, `calls` forward + backward pairs per event pair (host time included), and
              replayed  as ONE captured HIP graph of a forward + backward (device time: what a captured step sees),
            with cache-resident operands and, replayed only, cold: a 512 MiB buffer (twice the last-level cache) is
            overwritten before every replay and the event pair brackets that one replay.  The two C entry points alone are
            timed as well.  Launch counts: the device kernels of one eager forward + backward as torch.profiler lists them.
  steps     a whole captured training step (forward, loss, backward, FlatAdam; `engine._GraphedStep`, what
            `Trainer(hip_graph=True)` replays) of msgat72 on the frozen graph and with learn_edge_weights=True, each with
            dropout off, with edge_dropout=0.1, and with the same mask formed by torch ops; `calls` replays per event pair.

    python tools/edge_dropout_bench.py [--rounds 7] [--calls 20] [--out profiles/edge_dropout] [--kernels | --steps-only]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
from ms_gat_amd import _lib, engine, model, ops  # noqa: E402

N, EDGES, B, R, T = 883, 866, 32, 5, 12
P = 0.1
DEV = torch.device("cuda:0")
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def event_pair(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # us per call


def alternate(fns, rounds, calls, warmup=10, before=None):
    """{name: [us per call, one figure per round]}: the variants alternate inside every round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            if before is not None:
                before()
            times[k].append(event_pair(fn, calls))
    return times


def report(title, times):
    say(title)
    for k, v in times.items():
        say(f"  {k}: median {statistics.median(v):.2f} us, fastest {min(v):.2f} us, slowest {max(v):.2f} us ({len(v)} rounds)")


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def device_kernels(fn):
    """names of the device kernels of one call of fn, or None where the profiler is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    except Exception as exc:      # noqa: BLE001 -- a count that cannot be taken is reported as such
        say(f"  torch.profiler not usable here: {type(exc).__name__}: {exc}"[:200])
        return None


def torch_mask(shape, p, exempt=None):
    """The multipliers by torch ops: a uniform draw, a compare, a select (and the exempt edges' 1)."""
    scale = 1.0 / (1.0 - p)
    m = torch.where(torch.rand(shape, device=DEV) < p, 0.0, scale)
    return m if exempt is None else torch.where(exempt, 1.0, m)


def kernels(rounds, calls):
    g = torch.Generator().manual_seed(0)
    pattern = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1).to_sparse_csr()
    nnz = pattern.values().numel()
    shared = pattern.values().clone().to(DEV).requires_grad_(True)
    sets = (pattern.values()[None, :] + 0.05 * torch.randn(B, nnz, generator=g)).to(DEV).requires_grad_(True)
    dout = torch.randn(B, nnz, generator=g).to(DEV)
    state = ops.edge_dropout_state(1, DEV)

    def run(w, make):
        w.grad = None
        out = make()
        out.backward(dout)
        return out

    forms = {
        "hip, w [nnz]": lambda: run(shared, lambda: ops.edge_dropout(shared, P, state, samples=B)),
        "torch, w [nnz]": lambda: run(shared, lambda: shared * torch_mask((B, nnz), P)),
        "hip, w [B,nnz]": lambda: run(sets, lambda: ops.edge_dropout(sets, P, state)),
        "torch, w [B,nnz]": lambda: run(sets, lambda: sets * torch_mask((B, nnz), P)),
    }
    for k, fn in forms.items():          # the same kind of thing: shape, drop rate within 5 sigma, one scale
        out = fn().detach()
        rate = float((out == 0).float().mean())
        assert out.shape == (B, nnz) and abs(rate - P) < 5 * (P * (1 - P) / (B * nnz)) ** 0.5, (k, rate)
    say(f"kernels at B={B} nnz={nnz} p={P} (out and dout {B * nnz * 4 / 1e6:.2f} MB each), {calls} calls per event pair, "
        f"{os.path.basename(_lib.LIB_PATH)}")
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
    thr, scale = ops.edge_dropout_constants(P)
    out, used = torch.empty(B, nnz, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    dshared, dsets = torch.empty(nnz, device=DEV), torch.empty(B, nnz, device=DEV)
    w1, w2 = shared.detach(), sets.detach()
    alone = {
        "msgat_edge_dropout, w [nnz] (draw + advance)": lambda: _lib.check(L.msgat_edge_dropout(
            w1.data_ptr(), None, state.data_ptr(), used.data_ptr(), out.data_ptr(), B, nnz, 0, 0, thr, scale, 1, s), "fwd"),
        "msgat_edge_dropout, w [nnz], advance = 0": lambda: _lib.check(L.msgat_edge_dropout(
            w1.data_ptr(), None, state.data_ptr(), used.data_ptr(), out.data_ptr(), B, nnz, 0, 0, thr, scale, 0, s), "fwd"),
        "msgat_edge_dropout, w [B,nnz] (draw + advance)": lambda: _lib.check(L.msgat_edge_dropout(
            w2.data_ptr(), None, state.data_ptr(), used.data_ptr(), out.data_ptr(), B, nnz, 1, 0, thr, scale, 1, s), "fwd"),
        "msgat_edge_dropout_backward, dw [nnz]": lambda: _lib.check(L.msgat_edge_dropout_backward(
            dout.data_ptr(), None, state.data_ptr(), used.data_ptr(), dshared.data_ptr(), B, nnz, 0, 0, thr, scale, s), "bwd"),
        "msgat_edge_dropout_backward, dw [B,nnz]": lambda: _lib.check(L.msgat_edge_dropout_backward(
            dout.data_ptr(), None, state.data_ptr(), used.data_ptr(), dsets.data_ptr(), B, nnz, 1, 0, thr, scale, s), "bwd"),
    }
    single = alternate(alone, rounds, calls)
    report("the entry points alone, back-to-back launches from Python (cache-resident; launch-rate bound where the kernel is "
           "shorter than a launch):", single)
    med = lambda t: {k: round(statistics.median(v), 2) for k, v in t.items()}  # noqa: E731
    return {"B": B, "nnz": nnz, "p": P, "launches": counts, "replayed_warm_us": med(warm), "replayed_cold_us": med(cold),
            "entry_points_us": med(single)}


def steps(rounds, calls):
    g = torch.Generator().manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1)
    batch = [torch.randn(B, R, 1, N, T, generator=g), torch.randint(0, 24, (B,), generator=g),
             torch.randint(0, 7, (B,), generator=g), torch.randn(B, N, T, generator=g)]
    batch = [t.to(DEV) for t in batch]
    out_dir = tempfile.mkdtemp(prefix="edge_dropout_bench_")

    def build(learn, p=0.0, torch_ops=False):
        torch.manual_seed(0)
        net = model.msgat72(n_components=R, in_channels=1, in_timesteps=T, out_timesteps=T, use_te=True, adj=adj,
                            learn_edge_weights=learn, edge_dropout=0.0 if torch_ops else p).to(DEV)
        if torch_ops:       # the same regulariser by torch ops: one [B,nnz] mask per forward, the stored diagonal exempt
            csr = adj.to_sparse_csr()
            crow, col = csr.crow_indices().to(DEV), csr.col_indices().to(DEV)
            rows = torch.repeat_interleave(torch.arange(N, device=DEV), crow[1:] - crow[:-1])
            exempt = rows == col
            frozen = csr.values().to(DEV)

            def adjacency(H=None, D=None, X=None):
                w = net.edge_weight if learn else frozen
                return ops.edge_adjacency(crow, col, w[None, :] * torch_mask((H.shape[0], w.numel()), p, exempt))
            net.adjacency = adjacency
        trainer = engine.Trainer(net, 50.0, out_dir, hip_graph=True)
        step = engine._GraphedStep(trainer, batch, training=True, step_in_graph=True)
        return net, trainer, step

    configs = {}
    for learn in (False, True):
        tag = f"learn_edge_weights={learn}"
        configs[f"{tag}, dropout off"] = build(learn)
        configs[f"{tag}, edge_dropout={P}"] = build(learn, P)
        configs[f"{tag}, mask from torch ops"] = build(learn, P, torch_ops=True)
    times = alternate({k: v[2].graph.replay for k, v in configs.items()}, rounds, calls, warmup=5)
    say(f"captured training step (forward, loss, backward, FlatAdam) of msgat72, R={R} B={B} N={N} T={T} nnz={int((adj != 0).sum())}, "
        f"{calls} replays per event pair:")
    for k, v in times.items():
        say(f"  {k}: median {statistics.median(v) / 1e3:.4f} ms, fastest {min(v) / 1e3:.4f} ms, slowest {max(v) / 1e3:.4f} ms "
            f"({len(v)} rounds)")
    losses = {k: float(v[2].loss.detach()) for k, v in configs.items()}
    say("  loss of the last replay: " + ", ".join(f"{k} {v:.6g}" for k, v in losses.items()))
    positions = {k: v[0].edge_dropout_state() for k, v in configs.items() if v[0].edge_dropout > 0}
    say("  mask stream after the replays: " + ", ".join(f"{k} step {v['step']}" for k, v in positions.items()))
    return {k: round(statistics.median(v) / 1e3, 4) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "edge_dropout"))
    ap.add_argument("--kernels", action="store_true", help="the kernel timings only")
    ap.add_argument("--steps-only", action="store_true", help="the captured training steps only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_dropout_bench.py needs the GPU: there is nothing to time without one")
    say(f"# tools/edge_dropout_bench.py --rounds {a.rounds} --calls {a.calls} on {torch.cuda.get_device_name(0)}: HIP events, "
        "medians over rounds, variants alternated inside a round")
    result = {}
    if not a.steps_only:
        result["kernels"] = kernels(a.rounds, a.calls)
    if not a.kernels:
        result["captured_step_ms"] = steps(a.rounds, a.calls)
    say(json.dumps(result))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "edge_dropout_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
