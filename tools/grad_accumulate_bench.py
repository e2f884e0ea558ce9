"""Times gradient accumulation (`FlatAdam.accumulate`, `msgat_gather_accumulate`, `Trainer(accumulate_steps=k)`) on one GPU:

    python tools/grad_accumulate_bench.py [--rounds 5] [--iters 96] [--sets 24] [--steps 30] [--skip-step]

(1) The accumulating gather alone over the msgat72 / PEMSD7 layout (R = 5: 1 957 960 trainable elements in 202 tensors):
`flat += w * grad` for every gradient and `flat[-1] += w`, replayed from HIP graphs.  Variants, alternated within every round:
    library    `msgat_gather_accumulate` through `parallel.gather_scaled(accumulate=True)`: one launch
    foreach    torch `_foreach_add_(views of the flat buffer, gradients, alpha=w)` plus the weight's `add_`: what a user could
               write from outside the package
each COLD (every variant owns `--sets` sets of gradients and flat buffers, 15.7 MB a set, and its replays walk through them;
with the default 24 sets a set comes back after more bytes than the 256 MB last-level cache have passed) and WARM (one set,
replayed back to back).  Both read 8 and write 4 bytes per element.  The launch counts are those of one eager call, counted
by the profiler where it is available.
(2) One window of k = 2 of the msgat72 training step at the PEMSD7 shape (B = 32, N = 883, R = 5) through
`engine.Trainer(hip_graph=True, accumulate_steps=2)` -- forward and backward captured, `accumulate` / `step` launched
eagerly -- against two plain captured steps (`accumulate_steps=1`: the step as it was before accumulation existed, update
inside the graph), alternated in one process; `--steps` batches between two device events per figure, all figures per PAIR
of batches.  A second plain trainer ("plain again": the same code over another model instance and other allocations) shows
what two instances differ by before the window is credited with a difference.
Prints one line per round and one JSON line with medians and the spread over the rounds."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_gat_amd  # noqa: E402
from ms_gat_amd import engine, model, parallel  # noqa: E402

CFG = dict(N=883, E=866, R=5, Cin=1, T=12, B=32)     # msgat72 / PEMSD7
N_PARAMS = 1957960
WEIGHT = 32.0


def network():
    adj = ms_gat_amd.synthetic_adjacency(CFG["N"], CFG["E"], seed=0)
    return model.build_msgat("ms-gat72", n_components=CFG["R"], in_channels=CFG["Cin"], in_timesteps=CFG["T"],
                             out_timesteps=CFG["T"], use_te=True, adj=adj)


class Gather:
    """One set of gradients and one flat buffer, and ONE captured accumulation over them."""

    def __init__(self, variant, shapes, dev, seed):
        g = torch.Generator().manual_seed(seed)
        self.grads = [(0.01 * torch.randn(s, generator=g)).to(dev) for s in shapes]
        self.offsets, off = [], 0
        for t in self.grads:
            self.offsets.append(off)
            off += t.numel()
        self.numel = off
        self.flat = torch.zeros(off + 1, device=dev)
        self.views = [self.flat[o:o + t.numel()].view_as(t) for o, t in zip(self.offsets, self.grads)]
        self.cache = {}
        self.call = self.library if variant == "library" else self.foreach
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.call()                              # builds and points the chunk table: nothing is uploaded in the capture
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.call()

    def library(self):
        parallel.gather_scaled(self.flat, self.grads, self.offsets, WEIGHT, self.numel, self.cache, accumulate=True)

    def foreach(self):
        torch._foreach_add_(self.views, self.grads, alpha=WEIGHT)
        self.flat[self.numel:].add_(WEIGHT)


def launches(fn):
    """Device kernels of one eager call, or None where the profiler cannot tell."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:   # noqa: BLE001 -- a figure for the record, not a result
        return None


def timed(fns, iters):
    """us per call over `iters` calls walking through `fns`, after one pass over all of them."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


class Step:
    """The msgat72 training step on one synthetic batch, captured; `window` micro-batches per optimizer step."""

    def __init__(self, dev, window):
        torch.manual_seed(0)
        self.tmp = tempfile.TemporaryDirectory()
        self.trainer = engine.Trainer(network().to(dev), 50.0, self.tmp.name, hip_graph=True, accumulate_steps=window)
        g = torch.Generator().manual_seed(3)
        B = CFG["B"]
        self.batch = [torch.randn(B, CFG["R"], CFG["Cin"], CFG["N"], CFG["T"], generator=g).to(dev),
                      torch.randint(0, 24, (B,), generator=g).to(dev), torch.randint(0, 7, (B,), generator=g).to(dev),
                      (torch.randn(B, CFG["N"], CFG["T"], generator=g) * 30).to(dev)]
        self.dev = dev

    def run(self, batches):
        return self.trainer.run_epoch([self.batch] * batches, gpu_id=self.dev.index, epoch=1, mode="train")

    def ms_per_pair(self, batches):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(batches)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (batches / 2)


def spread(out, key, values, digits):
    out[f"{key}_median"] = round(statistics.median(values), digits)
    out[f"{key}_min_max"] = [round(min(values), digits), round(max(values), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=96)
    ap.add_argument("--sets", type=int, default=24)
    ap.add_argument("--steps", type=int, default=30, help="batches per figure of part (2): an even number")
    ap.add_argument("--skip-step", action="store_true", help="only the gather alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_accumulate_bench.py needs the GPU: there is nothing to time without one")
    if args.steps % 2:
        raise SystemExit("--steps must be even: part (2) counts pairs of batches")
    dev = torch.device("cuda:0")
    shapes = [tuple(p.shape) for p in network().parameters() if p.requires_grad]
    assert sum(torch.Size(s).numel() for s in shapes) == N_PARAMS, "not the msgat72 / PEMSD7 layout"
    variants = ("library", "foreach")
    sets = {v: [Gather(v, shapes, dev, seed) for seed in range(args.sets)] for v in variants}
    out = {"elements": N_PARAMS, "tensors": len(shapes), "sets": args.sets, "replays_per_figure": args.iters,
           "rounds": args.rounds, "bytes_per_element": 12, "cold_bytes_between_reuse": args.sets * N_PARAMS * 8}
    times = {(v, t): [] for v in variants for t in ("cold", "warm")}
    for r in range(args.rounds):
        for t in ("cold", "warm"):
            for v in variants:                       # alternated: library, foreach, library, ...
                fns = [u.graph.replay for u in (sets[v] if t == "cold" else sets[v][:1])]
                times[v, t].append(timed(fns, args.iters))
        print(f"round {r + 1} accumulating gather, graph replay:  "
              + "   ".join(f"{v} {t} {times[v, t][-1]:8.2f} us" for t in ("cold", "warm") for v in variants), flush=True)
    for (v, t), values in times.items():
        spread(out, f"gather_{v}_{t}_us", values, 2)
        out[f"gather_{v}_{t}_GBps"] = round(N_PARAMS * 12 / out[f"gather_{v}_{t}_us_median"] / 1e3, 1)
    probe = {v: sets[v][0] for v in variants}
    del sets
    torch.cuda.empty_cache()
    if not args.skip_step:
        steps = {"plain": Step(dev, 1), "window": Step(dev, 2), "plain_again": Step(dev, 1)}
        for s in steps.values():
            s.run(6)                                 # capture (at first sight) and settle
        ms = {k: [] for k in steps}
        for r in range(args.rounds):
            for k in steps:
                ms[k].append(steps[k].ms_per_pair(args.steps))
            print(f"round {r + 1} msgat72, B = {CFG['B']}, N = {CFG['N']}, R = {CFG['R']}, per pair of batches:  two plain "
                  f"steps {ms['plain'][-1]:8.4f} ms   one window of 2 {ms['window'][-1]:8.4f} ms   plain again "
                  f"{ms['plain_again'][-1]:8.4f} ms", flush=True)
        for k in steps:
            spread(out, f"pair_{k}_ms", ms[k], 4)
        out["pair_window_cost_ms"] = round(out["pair_window_ms_median"] - out["pair_plain_ms_median"], 4)
        out["pair_plain_instances_differ_ms"] = round(out["pair_plain_again_ms_median"] - out["pair_plain_ms_median"], 4)
        out["batches_per_figure"] = args.steps
    for v in variants:                               # last: the profiler is not part of any timed window
        out[f"gather_{v}_launches"] = launches(probe[v].call)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
