"""Times the quantile step tail, in one process on one GPU:

    python tools/quantile_bench.py [--pairs 50] [--replays 25] [--steps 20] [--rounds 5] [--out FILE]

1. The metrics + gradient pair at [B * N, Q, T_out] = [32 * 883, 3, 12] (20 % of the truth null): `msgat_quantile_metrics`
   + `msgat_quantile_grad` through the C ABI against the same quantities formed with torch ops (the loss, the
   [T_out + 1, 7 + 2Q] float64 totals, the valid count and the gradient) -- launches per pair, and microseconds per pair
   both launched eagerly (`pairs` back-to-back pairs between two device events, after a warm-up: what an eager step pays,
   host time included) and replayed from a captured HIP graph of `pairs` pairs (median, min and max of `replays` replays).
2. The captured msgat72 training step (N = 883, B = 32, R = 3) with `out_timesteps = 36`: under `QuantileLoss((0.1, 0.5,
   0.9))` on 12-step truths against the same model under the masked `HuberLoss` on 36-step truths -- the two differ only
   in the tail -- as `steps` replays per timing, the two alternating for `rounds` rounds, median per step.
Prints one line per measurement; `--out` also writes them to a file.
"""
import argparse
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_gat_amd  # noqa: E402
from ms_gat_amd import HuberLoss, QuantileLoss, _lib, engine, model, ops  # noqa: E402

LEVELS = (0.1, 0.5, 0.9)
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def event_us(fn, calls_inside):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls_inside


def eager_and_replayed(pair, pairs, replays):
    """-> (us per pair launched eagerly, (median, min, max) us per pair replayed from a graph of `pairs` pairs)."""
    def many():
        for _ in range(pairs):
            pair()
    many()
    torch.cuda.synchronize()
    eager = statistics.median(event_us(many, pairs) for _ in range(5))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        many()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        many()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    got = [event_us(graph.replay, pairs) for _ in range(replays)]
    return eager, (statistics.median(got), min(got), max(got))


def launches_of(pair):
    """Kernels one pair launches, counted by the profiler (None where it gives no device events)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        pair()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            pair()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:      # noqa: BLE001 -- a count is a convenience; the times below do not depend on it
        return None


def tail_pair(dev, pairs, replays):
    rows, t_out, q = 32 * 883, 12, len(LEVELS)
    g = torch.Generator().manual_seed(0)
    truth = 20 + 380 * torch.rand(rows, t_out, generator=g)
    truth[torch.rand(rows, t_out, generator=g) < 0.2] = 0.0
    offset = (torch.tensor(LEVELS) - 0.5).reshape(1, q, 1) * 60.0
    pred = (truth.unsqueeze(1) + offset + 15 * torch.randn(rows, q, t_out, generator=g)).reshape(rows, q * t_out).to(dev)
    truth = truth.to(dev)
    L = _lib.lib()
    part = torch.empty(int(L.msgat_quantile_partial_doubles(rows, t_out, q)), device=dev, dtype=torch.float64)
    loss, valid, dloss = torch.empty((), device=dev), torch.empty(1, device=dev), torch.ones((), device=dev)
    sums = torch.zeros(t_out + 1, 7 + 2 * q, device=dev, dtype=torch.float64)
    dpred = torch.empty_like(pred)
    levels = (_lib.C.c_float * q)(*LEVELS)

    def library():
        stream = _lib.stream_handle(dev)
        st = L.msgat_quantile_metrics(pred.data_ptr(), truth.data_ptr(), rows, t_out, q, levels, 1, 0.0, 0.0, part.data_ptr(),
                                      loss.data_ptr(), valid.data_ptr(), sums.data_ptr(), stream)
        st = st or L.msgat_quantile_grad(pred.data_ptr(), truth.data_ptr(), dloss.data_ptr(), valid.data_ptr(), rows, t_out, q,
                                         levels, 0.0, dpred.data_ptr(), stream)
        assert st == 0, st

    tau = torch.tensor(LEVELS, device=dev).reshape(1, q, 1)
    slopes = ops.quantile_slopes(LEVELS).to(dev).reshape(3, 1, q, 1)
    tsums = torch.zeros_like(sums)
    held = {}

    def torch_ops():
        p, y = pred.reshape(rows, q, t_out), truth
        v = ~torch.isnan(y) & (y != 0.0)
        u = y.unsqueeze(1) - p
        rho = torch.where(v.unsqueeze(1), torch.maximum(tau * u, (tau - 1) * u), torch.zeros_like(u))
        count = v.sum()
        held["loss"] = rho.sum() / (q * count.clamp(min=1))
        e = torch.where(v, p[:, 1] - y, torch.zeros_like(y)).double()
        yd = y.double()
        rel = v & (y > 0.0)
        ape = torch.where(rel, (e / torch.where(rel, yd, torch.ones_like(yd))).abs(), torch.zeros_like(e))
        crossing = v & (p[:, :-1] > p[:, 1:]).any(dim=1)
        width = torch.where(v, p[:, -1] - p[:, 0], torch.zeros_like(y)).double()
        hits = v.unsqueeze(1) & (y.unsqueeze(1) <= p)
        rhod = rho.double()
        cols = torch.cat([torch.stack([v.double().sum(0), e.abs().sum(0), 100.0 * ape.sum(0), (e * e).sum(0),
                                       rhod.sum((0, 1)) / q, crossing.double().sum(0), width.sum(0)], dim=1),
                          hits.double().sum(0).t(), rhod.sum(0).t()], dim=1)
        tsums[:t_out].add_(cols)
        tsums[t_out].add_(cols.sum(0))
        scale = dloss / count.clamp(min=1).float()
        each = torch.where(y.unsqueeze(1) > p, slopes[0], torch.where(y.unsqueeze(1) < p, slopes[1], slopes[2])) * scale
        held["dpred"] = torch.where(v.unsqueeze(1), each, torch.zeros_like(each))

    library()
    torch_ops()
    torch.cuda.synchronize()
    agree = float((tsums - sums).abs().max() / sums.abs().max())
    same_grad = bool(torch.equal(held["dpred"].reshape(rows, -1), dpred))
    say(f"# the two agree: totals within {agree:.1e} of the largest, loss {float(loss):.6f} / {float(held['loss']):.6f}, "
        f"gradient bit-equal: {same_grad}")
    say(f"# metrics + grad pair at [{rows}, {q}, {t_out}] ({rows * t_out} entries, 20 % null); microseconds per pair")
    for name, pair, known in (("library (msgat_quantile_metrics + _grad)", library, 3), ("torch ops", torch_ops, None)):
        n = launches_of(pair) or known
        eager, (med, lo, hi) = eager_and_replayed(pair, pairs, replays)
        say(f"{name:42s} launches {n if n is not None else 'not counted'!s:>12}   eager {eager:9.2f}   "
            f"replayed {med:9.2f}  ({lo:.2f} .. {hi:.2f})")
        held[name] = (eager, med)
    (le, lr), (te, tr) = held["library (msgat_quantile_metrics + _grad)"], held["torch ops"]
    say(f"# torch ops / library: eager {te / le:.1f}x, replayed {tr / lr:.1f}x")


class Step:
    """A captured msgat72 training step (N = 883, B = 32, R = 3, out_timesteps = 36) under one loss."""

    def __init__(self, dev, loss, truth_steps):
        torch.manual_seed(0)
        N, B, R, T = 883, 32, 3, 12
        adj = ms_gat_amd.synthetic_adjacency(N, 866, seed=0)
        net = model.msgat72(n_components=R, in_channels=1, in_timesteps=T, out_timesteps=36, use_te=True, adj=adj).to(dev)
        self._tmp = tempfile.TemporaryDirectory()
        self.trainer = engine.Trainer(net, 50.0, self._tmp.name, hip_graph=True, loss=loss)
        g = torch.Generator().manual_seed(3)
        y = 200 + 30 * torch.randn(B, N, truth_steps, generator=g)
        y[torch.rand(y.shape, generator=g) < 0.2] = 0.0
        self.batch = [torch.randn(B, R, 1, N, T, generator=g).to(dev), torch.randint(0, 24, (B,), generator=g).to(dev),
                      torch.randint(0, 7, (B,), generator=g).to(dev), y.to(dev)]
        self.dev = dev

    def ms_per_step(self, steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.trainer.run_epoch([self.batch] * steps, gpu_id=self.dev.index, epoch=1, mode="train")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps


def whole_step(dev, steps, rounds):
    quantile = Step(dev, QuantileLoss(LEVELS, null_value=0.0), 12)
    huber = Step(dev, HuberLoss(50.0, null_value=0.0), 36)
    for s in (quantile, huber):
        s.ms_per_step(3)          # capture and warm up
    got = {"quantile": [], "huber": []}
    for _ in range(rounds):       # alternating: both see the same machine
        got["quantile"].append(quantile.ms_per_step(steps))
        got["huber"].append(huber.ms_per_step(steps))
    say(f"# captured msgat72 training step, N = 883, B = 32, R = 3, out_timesteps = 36; ms per step over {steps} replays "
        f"(one epoch, its one host read included), median (min .. max) of {rounds} alternating rounds")
    for name, what in (("quantile", "QuantileLoss((0.1, 0.5, 0.9)), 12-step truths"),
                       ("huber", "masked HuberLoss(50), 36-step truths")):
        v = got[name]
        say(f"{what:48s} {statistics.median(v):8.4f}  ({min(v):.4f} .. {max(v):.4f})")
    dq = statistics.median(got["quantile"]) - statistics.median(got["huber"])
    say(f"# quantile - huber = {dq * 1e3:+.1f} us per step ({100 * dq / statistics.median(got['huber']):+.2f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50)
    ap.add_argument("--replays", type=int, default=25)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quantile_bench.py needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tail_pair(dev, args.pairs, args.replays)
    if not args.skip_step:
        say()
        whole_step(dev, args.steps, args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
