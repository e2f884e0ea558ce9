"""Validity-gated edges (msgat_edge_validity{,_backward}) on one MI355X at the PEMSD7 training shape: N = 883, the road
graph's nnz (2615 with the synthetic graph), B = 32, R = 5, T = 12, msgat72.  HIP events after warm-up, medians over rounds
in which the variants alternate; nothing is asserted except what the variants must share (the result's bits).

  kernels   out = w * g [B,nnz] forward and its backward under dout [B,nnz], for w [nnz] shared by the samples (the backward
            includes the batch sum) and for w [B,nnz]; validity is the strided view X[:, 0, -1] of a contiguous
            X [B,R,C,N,T].  Two formulations: "hip" -- `ops.edge_validity`, one launch each way -- and "torch" --
            `ops.edge_validity_reference` with torch autograd (a compare, a sum, two gathers, a compare, two selects and a
            multiply; backward through the same ops).  Each is timed
              eager     launched from Python, `calls` forward + backward pairs per event pair (host time included), and
              replayed  as ONE captured HIP graph of a forward + backward (device time: what a captured step sees),
            with cache-resident operands and, replayed only, cold: a 512 MiB buffer (twice the last-level cache) is
            overwritten before every replay and the event pair brackets that one replay.  The two C entry points alone are
            timed as well.  Launch counts: the device kernels of one eager forward + backward as torch.profiler lists them.
  steps     a whole captured training step (forward, loss, backward, FlatAdam; `engine._GraphedStep`, what
            `Trainer(hip_graph=True)` replays) of msgat72 on the frozen graph and with learn_edge_weights=True, each with the
            gate off, with missing_edges="scale", and with the same gate formed by torch ops; `calls` replays per event pair.

    python tools/edge_validity_bench.py [--rounds 7] [--calls 20] [--out profiles/edge_validity] [--kernels | --steps-only]
                                        [--pair-only]     (one forward + backward pair of each form: for a kernel trace)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
from ms_gat_amd import _lib, engine, graph, model, ops  # noqa: E402

N, EDGES, B, R, T, CIN = 883, 866, 32, 5, 12, 2
MODE = "scale"
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
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


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


def inputs(g):
    """X [B,R,CIN,N,T] with the validity channel last: a tenth of the windows cut short, one in twenty silent"""
    X = torch.randn(B, R, CIN, N, T, generator=g)
    valid = torch.ones(B, R, N, T)
    u = torch.rand(B, R, N, generator=g)
    cut = torch.randint(1, T, (B, R, N), generator=g)
    steps = torch.arange(T)
    valid[(u < 0.10)[..., None] & (steps < cut[..., None])] = 0.0
    valid[u < 0.05] = 0.0
    X[:, :, -1] = valid
    return X


def pattern_on_device():
    csr = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1).to_sparse_csr()
    crow, col = csr.crow_indices().to(DEV), csr.col_indices().to(DEV)
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), crow[1:] - crow[:-1])
    return csr, crow, col, (rows == col)


def kernels(rounds, calls, pair_only=False):
    g = torch.Generator().manual_seed(0)
    csr, crow, col, exempt = pattern_on_device()
    nnz = csr.values().numel()
    X = inputs(g).to(DEV)
    validity = X[:, 0, -1]
    shared = csr.values().clone().to(DEV).requires_grad_(True)
    sets = (csr.values()[None, :] + 0.05 * torch.randn(B, nnz, generator=g)).to(DEV).requires_grad_(True)
    dout = torch.randn(B, nnz, generator=g).to(DEV)

    def run(w, make):
        w.grad = None
        out = make()
        out.backward(dout)
        return out

    forms = {
        "hip, w [nnz]": lambda: run(shared, lambda: ops.edge_validity(shared, validity, crow, col, mode=MODE, exempt=exempt)),
        "torch, w [nnz]": lambda: run(shared, lambda: ops.edge_validity_reference(shared, validity, crow, col, mode=MODE,
                                                                                  exempt=exempt)),
        "hip, w [B,nnz]": lambda: run(sets, lambda: ops.edge_validity(sets, validity, crow, col, mode=MODE, exempt=exempt)),
        "torch, w [B,nnz]": lambda: run(sets, lambda: ops.edge_validity_reference(sets, validity, crow, col, mode=MODE,
                                                                                  exempt=exempt)),
    }
    outs = {k: fn().detach() for k, fn in forms.items()}
    assert torch.equal(outs["hip, w [nnz]"], outs["torch, w [nnz]"]) and torch.equal(outs["hip, w [B,nnz]"], outs["torch, w [B,nnz]"])
    gated = float((outs["hip, w [nnz]"] == 0).float().mean())
    if pair_only:
        torch.cuda.synchronize()
        return {}
    say(f"kernels at B={B} nnz={nnz} N={N} T={T} mode={MODE!r} (out and dout {B * nnz * 4 / 1e6:.2f} MB each, validity read in "
        f"place from X {tuple(X.shape)}; {100 * gated:.1f} % of the edges fully gated), {calls} calls per event pair, "
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
    gstruct, keep = graph.edge_pattern_of(crow, col).structure.on(DEV)
    table = (C.c_float * (T + 1))(*ops.edge_validity_table(MODE, T))
    ex = exempt.to(torch.uint8)
    out, dshared, dsets = torch.empty(B, nnz, device=DEV), torch.empty(nnz, device=DEV), torch.empty(B, nnz, device=DEV)
    w1, w2, stride = shared.detach(), sets.detach(), validity.stride(0)
    alone = {
        "msgat_edge_validity, w [nnz]": lambda: _lib.check(L.msgat_edge_validity(
            gstruct, w1.data_ptr(), ex.data_ptr(), validity.data_ptr(), stride, table, out.data_ptr(), B, T, 0, s), "fwd"),
        "msgat_edge_validity, w [B,nnz]": lambda: _lib.check(L.msgat_edge_validity(
            gstruct, w2.data_ptr(), ex.data_ptr(), validity.data_ptr(), stride, table, out.data_ptr(), B, T, 1, s), "fwd"),
        "msgat_edge_validity_backward, dw [nnz]": lambda: _lib.check(L.msgat_edge_validity_backward(
            gstruct, dout.data_ptr(), ex.data_ptr(), validity.data_ptr(), stride, table, dshared.data_ptr(), B, T, 0, s), "bwd"),
        "msgat_edge_validity_backward, dw [B,nnz]": lambda: _lib.check(L.msgat_edge_validity_backward(
            gstruct, dout.data_ptr(), ex.data_ptr(), validity.data_ptr(), stride, table, dsets.data_ptr(), B, T, 1, s), "bwd"),
    }
    single = alternate(alone, rounds, calls)
    report("the entry points alone, back-to-back launches from Python (cache-resident; launch-rate bound where the kernel is "
           "shorter than a launch):", single)
    med = lambda t: {k: round(statistics.median(v), 2) for k, v in t.items()}  # noqa: E731
    return {"B": B, "nnz": nnz, "T": T, "launches": counts, "replayed_warm_us": med(warm), "replayed_cold_us": med(cold),
            "entry_points_us": med(single)}


def steps(rounds, calls):
    g = torch.Generator().manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1)
    batch = [inputs(g), torch.randint(0, 24, (B,), generator=g), torch.randint(0, 7, (B,), generator=g),
             torch.randn(B, N, T, generator=g)]
    batch = [t.to(DEV) for t in batch]
    out_dir = tempfile.mkdtemp(prefix="edge_validity_bench_")

    def build(learn, gate=None):
        torch.manual_seed(0)
        net = model.msgat72(n_components=R, in_channels=CIN, in_timesteps=T, out_timesteps=T, use_te=True, adj=adj,
                            learn_edge_weights=learn, missing_edges=MODE if gate else None).to(DEV)
        if gate == "torch":      # the same model, the gate alone formed by torch ops in place of the launch
            net._gate_missing = lambda weights, X, crow, col: ops.edge_validity_reference(
                weights, X[:, 0, -1], crow, col, mode=MODE, exempt=net.edge_valid_exempt)
        trainer = engine.Trainer(net, 50.0, out_dir, hip_graph=True)
        step = engine._GraphedStep(trainer, batch, training=True, step_in_graph=True)
        return net, trainer, step

    configs = {}
    for learn in (False, True):
        tag = f"learn_edge_weights={learn}"
        configs[f"{tag}, gate off"] = build(learn)
        configs[f"{tag}, missing_edges={MODE!r}"] = build(learn, "hip")
        configs[f"{tag}, gate from torch ops"] = build(learn, "torch")
    times = alternate({k: v[2].graph.replay for k, v in configs.items()}, rounds, calls, warmup=5)
    say(f"captured training step (forward, loss, backward, FlatAdam) of msgat72, R={R} B={B} N={N} T={T} C_in={CIN} "
        f"nnz={int((adj != 0).sum())}, {calls} replays per event pair:")
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
                                                  "edge_validity"))
    ap.add_argument("--name", default="edge_validity_bench.txt", help="file name under --out")
    ap.add_argument("--kernels", action="store_true", help="the kernel timings only")
    ap.add_argument("--steps-only", action="store_true", help="the captured training steps only")
    ap.add_argument("--pair-only", action="store_true", help="run each form's forward + backward once and stop (for a trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_validity_bench.py needs the GPU: there is nothing to time without one")
    if a.pair_only:
        kernels(a.rounds, a.calls, pair_only=True)
        return
    say(f"# tools/edge_validity_bench.py --rounds {a.rounds} --calls {a.calls} on {torch.cuda.get_device_name(0)}: HIP events, "
        "medians over rounds, variants alternated inside a round")
    result = {}
    if not a.steps_only:
        result["kernels"] = kernels(a.rounds, a.calls)
    if not a.kernels:
        result["captured_step_ms"] = steps(a.rounds, a.calls)
    say(json.dumps(result))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
