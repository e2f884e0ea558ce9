"""Hour- and day-dependent edge weights (msgat_edge_time_weights{,_backward}) on one MI355X at the PEMSD7 training shape:
N = 883, the road graph's nnz (2615 with the synthetic graph), B = 32, R = 5, msgat72.  HIP events after warm-up, medians
over rounds in which the variants alternate; nothing is asserted except that the variants compute the same thing.

  kernels   w = (base + h_w[H]) + d_w[D] [B,nnz] forward and its backward under dout [B,nnz], two formulations:
            "hip" -- `ops.edge_time_weights`, one launch each way -- and "torch" -- the same expression in torch ops with
            torch autograd (two embedding gathers and two adds; a batch sum, two zero fills and two embedding scatters).
            Each is timed
              eager     launched from Python, `calls` forward + backward pairs per event pair (host time included), and
              replayed  as ONE captured HIP graph of a forward + backward (device time: what a captured step sees),
            with cache-resident operands (every tensor of the problem is 0.3 MB or less and is re-read from the caches by
            back-to-back launches) and, replayed only, cold: a 512 MiB buffer (twice the last-level cache) is overwritten
            before every replay and the event pair brackets that one replay.  The two C entry points alone are timed as
            well (`calls` launches per event pair, cache-resident).  Launch counts: the device kernels of one eager
            forward + backward as torch.profiler lists them.
  steps     a whole captured training step (forward, loss, backward, FlatAdam; `engine._GraphedStep`, what
            `Trainer(hip_graph=True)` replays) of msgat72 with learn_edge_weights = False, True, "time", and "time" with the
            weights formed by torch ops; `calls` replays per event pair.

    python tools/edge_time_bench.py [--rounds 7] [--calls 20] [--out profiles/edge_time] [--kernels | --steps-only]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import ms_gat_amd  # noqa: E402
from ms_gat_amd import _lib, engine, model, ops  # noqa: E402

N, EDGES, B, R, T = 883, 866, 32, 5, 12
NH, ND = 24, 7
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


def kernels(rounds, calls):
    g = torch.Generator().manual_seed(0)
    pattern = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1).to_sparse_csr()
    nnz = pattern.values().numel()
    base = pattern.values().clone().to(DEV).requires_grad_(True)
    h_w = (0.05 * torch.randn(NH, nnz, generator=g)).to(DEV).requires_grad_(True)
    d_w = (0.05 * torch.randn(ND, nnz, generator=g)).to(DEV).requires_grad_(True)
    H = torch.randint(0, NH, (B,), generator=g).to(DEV)
    D = torch.randint(0, ND, (B,), generator=g).to(DEV)
    dout = torch.randn(B, nnz, generator=g).to(DEV)
    params = (base, h_w, d_w)

    def run(make):
        for p in params:
            p.grad = None
        w = make()
        w.backward(dout)
        return w

    forms = {"hip": lambda: run(lambda: ops.edge_time_weights(base, h_w, d_w, H, D)),
             "torch": lambda: run(lambda: (base + F.embedding(H, h_w)) + F.embedding(D, d_w))}
    # the same thing: the forward bit for bit, the gradients to rounding (torch's scatter adds in no promised order)
    w_hip = forms["hip"]().detach().clone()
    g_hip = [p.grad.clone() for p in params]
    w_torch = forms["torch"]().detach().clone()
    assert torch.equal(w_hip, w_torch)
    for a, p in zip(g_hip, params):
        assert float((a - p.grad).abs().max()) <= 1e-5 * float(p.grad.abs().max())
    say(f"kernels at B={B} nnz={nnz} nh={NH} nd={ND} (w and dout {B * nnz * 4 / 1e6:.2f} MB each), {calls} calls per event pair, "
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
    out = torch.empty(B, nnz, device=DEV)
    dbase, dh, dd = torch.empty(nnz, device=DEV), torch.empty(NH, nnz, device=DEV), torch.empty(ND, nnz, device=DEV)
    b0, h0, d0 = (p.detach() for p in params)
    alone = {
        "msgat_edge_time_weights": lambda: _lib.check(L.msgat_edge_time_weights(
            b0.data_ptr(), h0.data_ptr(), d0.data_ptr(), H.data_ptr(), D.data_ptr(), out.data_ptr(), B, nnz, NH, ND, s), "fwd"),
        "msgat_edge_time_weights_backward": lambda: _lib.check(L.msgat_edge_time_weights_backward(
            dout.data_ptr(), H.data_ptr(), D.data_ptr(), dbase.data_ptr(), dh.data_ptr(), dd.data_ptr(), B, nnz, NH, ND, s), "bwd"),
    }
    single = alternate(alone, rounds, calls)
    report("the entry points alone, back-to-back launches from Python (cache-resident; launch-rate bound where the kernel is "
           "shorter than a launch):", single)
    med = lambda t: {k: round(statistics.median(v), 2) for k, v in t.items()}  # noqa: E731
    return {"B": B, "nnz": nnz, "launches": counts, "replayed_warm_us": med(warm), "replayed_cold_us": med(cold),
            "entry_points_us": med(single)}


def steps(rounds, calls):
    g = torch.Generator().manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1)
    batch = [torch.randn(B, R, 1, N, T, generator=g), torch.randint(0, NH, (B,), generator=g),
             torch.randint(0, ND, (B,), generator=g), torch.randn(B, N, T, generator=g)]
    batch = [t.to(DEV) for t in batch]
    out_dir = tempfile.mkdtemp(prefix="edge_time_bench_")

    def build(learn, torch_ops=False):
        torch.manual_seed(0)
        net = model.msgat72(n_components=R, in_channels=1, in_timesteps=T, out_timesteps=T, use_te=True, adj=adj,
                            learn_edge_weights=learn).to(DEV)
        if learn == "time":
            tg = torch.Generator().manual_seed(1)     # the same tables in both "time" configurations
            with torch.no_grad():
                for t in (net.edge_h_ebd.weight, net.edge_d_ebd.weight):
                    t.copy_((0.05 * torch.randn(t.shape, generator=tg)).to(DEV))
        if torch_ops:
            net.adjacency = lambda H, D: ops.edge_adjacency(
                net.edge_crow, net.edge_col, (net.edge_weight + net.edge_h_ebd(H)) + net.edge_d_ebd(D))
        trainer = engine.Trainer(net, 50.0, out_dir, hip_graph=True)
        step = engine._GraphedStep(trainer, batch, training=True, step_in_graph=True)
        return net, trainer, step

    configs = {"learn_edge_weights=False": build(False), "learn_edge_weights=True": build(True),
               'learn_edge_weights="time"': build("time"), '"time" from torch ops': build("time", torch_ops=True)}
    times = alternate({k: v[2].graph.replay for k, v in configs.items()}, rounds, calls, warmup=5)
    say(f"captured training step (forward, loss, backward, FlatAdam) of msgat72, R={R} B={B} N={N} T={T} nnz={int((adj != 0).sum())}, "
        f"{calls} replays per event pair:")
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
                                                  "edge_time"))
    ap.add_argument("--kernels", action="store_true", help="the kernel timings only")
    ap.add_argument("--steps-only", action="store_true", help="the captured training steps only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_time_bench.py needs the GPU: there is nothing to time without one")
    say(f"# tools/edge_time_bench.py --rounds {a.rounds} --calls {a.calls} on {torch.cuda.get_device_name(0)}: HIP events, "
        "medians over rounds, variants alternated inside a round")
    result = {}
    if not a.steps_only:
        result["kernels"] = kernels(a.rounds, a.calls)
    if not a.kernels:
        result["captured_step_ms"] = steps(a.rounds, a.calls)
    say(json.dumps(result))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "edge_time_bench.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
