"""Times `FlatAdam.step()` with the guard off and on, alternated in one process on one GPU:

    python tools/guarded_step_bench.py [--rounds 5] [--iters 100]

The parameter layout is that of msgat72 on PEMSD7 with R = 5 components (1 957 960 trainable elements, a 7.8 MB flat
gradient buffer); every parameter has a gradient, copied into the flat views by the step as in training.  Guard on =
`FlatAdam(max_grad_norm=1.0, skip_nonfinite=True)`: two more launches (sum of squares per chunk, finish) and the guarded
update.  Each round times `iters` steps of either optimizer between two device events after a warm-up -- launched one by
one (what an eager step sees: host time included) and as replays of ONE captured step (what a step inside the engine's HIP
graph sees: device time).  Prints one line per round and a JSON line with medians and the spread over the rounds.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_gat_amd  # noqa: E402
from ms_gat_amd import engine, model  # noqa: E402

CFG = dict(N=883, E=866, R=5, Cin=1, T=12)     # msgat72 / PEMSD7
N_PARAMS = 1957960


def layout(dev):
    adj = ms_gat_amd.synthetic_adjacency(CFG["N"], CFG["E"], seed=0)
    net = model.build_msgat("ms-gat72", n_components=CFG["R"], in_channels=CFG["Cin"], in_timesteps=CFG["T"],
                            out_timesteps=CFG["T"], use_te=True, adj=adj)
    shapes = [tuple(p.shape) for p in net.parameters() if p.requires_grad]
    assert sum(torch.Size(s).numel() for s in shapes) == N_PARAMS, "not the msgat72 / PEMSD7 layout"
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).to(dev)) for s in shapes]
    for p in params:
        p.grad = (0.01 * torch.randn(p.shape, generator=g)).to(dev)
    return params


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters     # us per step


def captured(opt):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                               # builds the buffers and the chunk tables
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guarded_step_bench.py needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    opts = {"off": engine.FlatAdam(layout(dev), lr=1e-3, weight_decay=5e-4),
            "on": engine.FlatAdam(layout(dev), lr=1e-3, weight_decay=5e-4, max_grad_norm=1.0, skip_nonfinite=True)}
    graphs = {k: captured(o) for k, o in opts.items()}
    runs = {"eager": {k: o.step for k, o in opts.items()}, "graph": {k: g.replay for k, g in graphs.items()}}
    times = {(mode, k): [] for mode in runs for k in opts}
    for r in range(args.rounds):
        for mode, fns in runs.items():
            for k in ("off", "on"):              # alternated: off, on, off, on, ...
                times[mode, k].append(timed(fns[k], args.iters))
            print(f"round {r + 1} {mode:5s}  guard off {times[mode, 'off'][-1]:8.2f} us/step   guard on {times[mode, 'on'][-1]:8.2f} us/step")
    stats = opts["on"].guard_stats()
    assert stats["skipped_steps"] == 0 and stats["clip_coef"] < 1.0, stats
    out = {"elements": N_PARAMS, "chunks": int(opts["on"]._guard_partials.numel()), "steps_per_figure": args.rounds * args.iters,
           "grad_norm": stats["grad_norm"], "clip_coef": stats["clip_coef"]}
    for (mode, k), v in times.items():
        out[f"{mode}_guard_{k}_us_median"] = round(statistics.median(v), 2)
        out[f"{mode}_guard_{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    for mode in runs:
        out[f"{mode}_guard_cost_us"] = round(out[f"{mode}_guard_on_us_median"] - out[f"{mode}_guard_off_us_median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
