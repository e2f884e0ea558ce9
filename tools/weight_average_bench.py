"""Times the averaged weights (`FlatAdam(ema_decay=...)`, `msgat_adam_step_averaged`) on one GPU:

    python tools/weight_average_bench.py [--rounds 5] [--iters 60] [--steps 30] [--skip-step]

(1) The update alone (`FlatAdam.step()`: the copy of the gradients into the flat buffer, 8 more bytes per element in every
variant, and the update) over the msgat72 / PEMSD7 layout (R = 5: 1 957 960 trainable elements), replayed from HIP graphs and
with COLD operands: every variant owns `--sets` complete sets of buffers (parameters, gradient, moments, shadow; 55 - 70 MB a
set) and its replays walk through them, so a set comes back only after more bytes than the 256 MB last-level cache have
passed.  Variants, alternated within every round:
    plain      `msgat_adam_step`                                       28 bytes per element in the update
    averaged   `msgat_adam_step_averaged`, decay 0.999                 36 bytes per element
    foreach    `msgat_adam_step`, then the same average as torch `_foreach` ops (sub, mul_, add_ over the 202 tensors:
               what a user could add from outside the package)
(2) The captured msgat72 training step at the PEMSD7 shape (B = 32, N = 883, R = 5) through `engine.Trainer(hip_graph=True)`,
`ema_decay=0.999` against `None`, alternated in one process: `--steps` replays between two device events per figure.
A second trainer without the average ("off again": the same code over another model instance and other allocations) shows
what two instances differ by before the average is credited with a difference.
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
from ms_gat_amd import engine, model  # noqa: E402

CFG = dict(N=883, E=866, R=5, Cin=1, T=12, B=32)     # msgat72 / PEMSD7
N_PARAMS = 1957960
DECAY = 0.999


def network():
    adj = ms_gat_amd.synthetic_adjacency(CFG["N"], CFG["E"], seed=0)
    return model.build_msgat("ms-gat72", n_components=CFG["R"], in_channels=CFG["Cin"], in_timesteps=CFG["T"],
                             out_timesteps=CFG["T"], use_te=True, adj=adj)


def layout(shapes, dev, seed):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).to(dev)) for s in shapes]
    for p in params:
        p.grad = (0.01 * torch.randn(p.shape, generator=g)).to(dev)
    return params


class Update:
    """One set of buffers and ONE captured update over them."""

    def __init__(self, variant, shapes, dev, seed):
        self.params = layout(shapes, dev, seed)
        self.opt = engine.FlatAdam(self.params, lr=1e-3, weight_decay=5e-4, ema_decay=DECAY if variant == "averaged" else None)
        self.shadow = [p.detach().clone() for p in self.params] if variant == "foreach" else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.step()                              # builds the buffers and the chunk tables
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.step()

    def step(self):
        self.opt.step()
        if self.shadow is not None:                  # e += (1 - d) (w - e) with a host constant for 1 - d
            with torch.no_grad():
                diff = torch._foreach_sub([p.detach() for p in self.params], self.shadow)
                torch._foreach_mul_(diff, 1.0 - DECAY)
                torch._foreach_add_(self.shadow, diff)


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
    """The captured msgat72 training step on one synthetic batch."""

    def __init__(self, dev, ema_decay):
        torch.manual_seed(0)
        self.tmp = tempfile.TemporaryDirectory()
        self.trainer = engine.Trainer(network().to(dev), 50.0, self.tmp.name, hip_graph=True, ema_decay=ema_decay)
        g = torch.Generator().manual_seed(3)
        B = CFG["B"]
        self.batch = [torch.randn(B, CFG["R"], CFG["Cin"], CFG["N"], CFG["T"], generator=g).to(dev),
                      torch.randint(0, 24, (B,), generator=g).to(dev), torch.randint(0, 7, (B,), generator=g).to(dev),
                      (torch.randn(B, CFG["N"], CFG["T"], generator=g) * 30).to(dev)]
        self.dev = dev

    def run(self, steps):
        return self.trainer.run_epoch([self.batch] * steps, gpu_id=self.dev.index, epoch=1, mode="train")

    def ms_per_step(self, steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps


def spread(out, key, values, digits):
    out[f"{key}_median"] = round(statistics.median(values), digits)
    out[f"{key}_min_max"] = [round(min(values), digits), round(max(values), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-step", action="store_true", help="only the update alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weight_average_bench.py needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    shapes = [tuple(p.shape) for p in network().parameters() if p.requires_grad]
    assert sum(torch.Size(s).numel() for s in shapes) == N_PARAMS, "not the msgat72 / PEMSD7 layout"
    variants = ("plain", "averaged", "foreach")
    # the gradient copy (read + write), the update, and for foreach sub, mul_, add_: 2 reads + 1 write, 1 + 1, 2 + 1
    bytes_per_element = {"plain": 8 + 28, "averaged": 8 + 36, "foreach": 8 + 28 + 12 + 8 + 12}
    sets = {v: [Update(v, shapes, dev, seed) for seed in range(args.sets)] for v in variants}
    assert args.sets * N_PARAMS * 28 > 256e6, "the sets of a variant must not fit the last-level cache together"
    out = {"elements": N_PARAMS, "tensors": len(shapes), "sets": args.sets, "replays_per_figure": args.iters,
           "rounds": args.rounds, "decay": DECAY}
    times = {v: [] for v in variants}
    for r in range(args.rounds):
        for v in variants:                           # alternated: plain, averaged, foreach, plain, ...
            times[v].append(timed([u.graph.replay for u in sets[v]], args.iters))
        print(f"round {r + 1} update alone, cold, graph replay:  " + "   ".join(f"{v} {times[v][-1]:8.2f} us" for v in variants),
              flush=True)
    for v in variants:
        spread(out, f"update_{v}_us", times[v], 2)
        out[f"update_{v}_GBps"] = round(N_PARAMS * bytes_per_element[v] / out[f"update_{v}_us_median"] / 1e3, 1)
    out["update_average_cost_us"] = round(out["update_averaged_us_median"] - out["update_plain_us_median"], 2)
    out["update_foreach_cost_us"] = round(out["update_foreach_us_median"] - out["update_plain_us_median"], 2)
    del sets
    torch.cuda.empty_cache()
    if not args.skip_step:
        steps = {"off": Step(dev, None), "on": Step(dev, DECAY), "off_again": Step(dev, None)}
        for s in steps.values():
            s.run(5)                                 # capture (at first sight) and settle
        ms = {k: [] for k in steps}
        for r in range(args.rounds):
            for k in steps:
                ms[k].append(steps[k].ms_per_step(args.steps))
            print(f"round {r + 1} captured msgat72 step, B = {CFG['B']}, N = {CFG['N']}, R = {CFG['R']}:  average off "
                  f"{ms['off'][-1]:8.4f} ms   average on {ms['on'][-1]:8.4f} ms   off again {ms['off_again'][-1]:8.4f} ms", flush=True)
        for k in steps:
            spread(out, f"step_average_{k}_ms", ms[k], 4)
        out["step_average_cost_ms"] = round(out["step_average_on_ms_median"] - out["step_average_off_ms_median"], 4)
        out["steps_per_figure"] = args.steps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
