"""Online forecasting (`OnlineForecaster`, msgat_ring_push / msgat_ring_windows) on one MI355X at the PEMSD7 serving
shape: one origin per step, R = 5 (hours 1, 2, 3, 24, 168), C = 3, N = 883, tau = 12, msgat72 with `missing_edges="scale"`,
`input_null_value=0.0` and the validity channel (so in_channels = 4); the ring holds 2016 steps.  HIP events after warm-up,
medians over rounds in which the variants alternate; nothing is asserted except what the variants must share (the bits of
X, H, D and of the forecast).

  (a) windows   a reading already on the device goes into the ring and X, H, D come out (push, clock advance, windows):
                its device kernels as torch.profiler lists them, its time launched eagerly, and replayed as ONE captured
                graph with cache-resident operands and cold (512 MiB overwritten before every replay, one replay per event
                pair).  Against it "host": the same X, H, D formed on the host -- the reading normalised there and written
                into a host ring kept twice over (so that every window is a contiguous slice), the windows sliced, imputed
                and masked as `data.PeriodicWindows` does, and X, H, D copied to the device.
  (b) step      `step()` from a HOST reading to a finished forecast (the copy of the reading, then one replay), and the
                same from a reading already on the device; against the host path of (a) followed by the same model's eager
                forward, and against the model's forward ALONE on an X that is already on the device -- eager, and as a
                captured graph, captured twice ("A", "B") so that the spread between two runs of the same work shows.
  (c) memory    `resident_bytes` of the ring.

    python tools/online_bench.py [--rounds 7] [--calls 20] [--out profiles/online] [--name online_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
from ms_gat_amd import _lib, data, model  # noqa: E402

HOURS, C_IN, N, EDGES, TAU, Q, DAYS = [1, 2, 3, 24, 168], 3, 883, 866, 12, 12, 21
NULL = 0.0
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
    return {k: round(statistics.median(v), 2) for k, v in times.items()}


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
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


def synthetic_series():
    """[C, N, total] fp32, seeded: a daily wave plus noise per (channel, node) with 1 % outages and two dead sensors
    written as 0, like data.SyntheticPEMS(missing=0.01, dead_sensors=2)."""
    total = DAYS * 24 * TAU
    g = torch.Generator().manual_seed(1)
    t = torch.arange(total, dtype=torch.float32)
    daily = torch.sin(2 * torch.pi * t / (24 * TAU))
    base = 200 + 80 * torch.rand(C_IN, N, 1, generator=g)
    raw = (base * (1 + 0.4 * daily) + 15 * torch.randn(C_IN, N, total, generator=g)).clamp_min(1.0)
    raw[:, data.SyntheticPEMS.outages(N, total, TAU, 0.01, 2, seed=2)] = NULL
    return raw


class HostPath:
    """X, H, D of the origin after the last reading, formed on the host and copied over.  The normalised history is a
    host ring [C, N, 2L] that holds every reading twice, L apart, so that each window is one contiguous slice (no shift
    of the history, no wrap inside a window); the rest is `data.PeriodicWindows._window`."""

    def __init__(self, stats, start):
        self.stats, self.L, self.t = stats, stats.history, start
        self.hist = torch.full((*stats.mean.shape, 2 * self.L), float("nan"))
        self.nan = torch.full((), float("nan"))

    def push(self, reading):
        s = self.stats
        z = torch.where(data.missing_entries(reading, s.input_null_value), self.nan, (reading - s.mean) / s.std)
        row = self.t % self.L
        self.hist[..., row] = z
        self.hist[..., row + self.L] = z
        self.t += 1

    def windows(self):
        s, t, L = self.stats, self.t, self.L
        xs = []
        for h in s.hours:
            first = t - h * s.tau
            at = first % L
            x = self.hist[..., at: at + s.tau]
            missing = torch.isnan(x)
            slots = torch.arange(first, first + s.tau) % s.period
            x = torch.where(missing, s.climatology[slots].permute(1, 2, 0), x)
            xs.append(torch.cat([x, (~missing.any(0, keepdim=True)).to(x.dtype)]))
        hour = t // s.tau
        return (torch.stack(xs)[None].to(DEV, non_blocking=True), torch.tensor([hour % 24]).to(DEV, non_blocking=True),
                torch.tensor([(hour // 24) % 7]).to(DEV, non_blocking=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "online"))
    ap.add_argument("--name", default="online_bench.txt", help="file name under --out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_bench.py needs the GPU: there is nothing to time without one")
    rounds, calls = a.rounds, a.calls
    say(f"# tools/online_bench.py --rounds {rounds} --calls {calls} on {torch.cuda.get_device_name(0)}: HIP events, medians "
        f"over rounds, variants alternated inside a round, {os.path.basename(_lib.LIB_PATH)}")
    raw = synthetic_series()
    stats = data.series_stats(raw, HOURS, Q, TAU, input_null_value=NULL)
    L, R = stats.history, len(HOURS)
    torch.manual_seed(0)
    net = model.msgat72(n_components=R, in_channels=stats.input_channels, in_timesteps=TAU, out_timesteps=Q, use_te=True,
                        adj=ms_gat_amd.synthetic_adjacency(N, EDGES, seed=1), missing_edges="scale").to(DEV)
    f = ms_gat_amd.OnlineForecaster(net, stats, 0)
    f.push(raw[:, :, :L].permute(2, 0, 1).contiguous().to(DEV))
    host = HostPath(stats, 0)
    for t in range(L):
        host.push(raw[:, :, t])
    say(f"shape: R={R} C={C_IN} (+1 validity) N={N} tau={TAU} T_out={Q}, ring L={L} rows, table period={stats.period}; a reading "
        f"is {C_IN * N * 4} B, X {R * stats.input_channels * N * TAU * 4 / 1e6:.3f} MB")
    say(f"(c) resident_bytes of the ring: {f.resident_bytes} ({f.resident_bytes / 1e6:.2f} MB); the table it is imputed from: "
        f"{f.climatology.numel() * 4 / 1e6:.2f} MB")

    # the two paths must agree before anything is timed: 30 steps, bits of X, H, D and of the forecast
    step_no = [L]

    def next_reading():
        r = raw[:, :, step_no[0] % raw.shape[-1]]
        step_no[0] += 1
        return r

    for _ in range(30):
        r = next_reading()
        y = f.step(r).clone()
        host.push(r)
        X, H, D = host.windows()
        with torch.no_grad():
            want = net(X, H, D)[0]
        assert torch.equal(f._out[0].view(torch.int32), X.view(torch.int32)) and torch.equal(f._out[1], H) \
            and torch.equal(f._out[2], D), "device and host windows differ"
        assert torch.equal(y.view(torch.int32), want.view(torch.int32)), "graphed step and eager forward on host windows differ"
    say("30 steps: X, H, D of the device ring and of the host path have the same bits, and so have the replayed forecast and "
        "the eager forward on the host path's X")

    # ---- (a) ---------------------------------------------------------------------------------------------------------------
    ring, clock, out = f.ring.clone(), f.clock.clone(), f._window_buffers()          # scratch state: the live clock stays
    reading_dev = raw[:, :, 7].contiguous()[None].to(DEV)
    reading_host = raw[:, :, 7].contiguous()

    def device_windows():
        f._push(reading_dev, ring, clock)
        f._windows(ring, clock, out=out)

    def host_windows():
        host.push(reading_host)
        host.windows()

    say("(a) push + windows: device kernels of one eager call (torch.profiler):")
    names = device_kernels(device_windows)
    launches = None if names is None else len(names)
    say(f"  launches: {'not measured' if names is None else launches}")
    for n in names or []:
        say(f"      {n[:150]}")
    a_eager = report("(a) eager, host time included (device: three launches from Python; host: normalise, slice, impute, mask, "
                     "copy X, H, D over), cache-resident operands:",
                     alternate({"device ring": device_windows, "host ring + H2D": host_windows}, rounds, calls))
    g_windows = capture(device_windows)
    a_warm = report("(a) push + windows as ONE captured graph replayed (device time), cache-resident operands:",
                    alternate({"device ring, replayed": g_windows.replay}, rounds, calls))
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    a_cold = report("(a) cold operands (512 MiB overwritten before each call; one call per event pair, so the pair's own "
                    "resolution of a few us is in the figure):",
                    alternate({"device ring, replayed": g_windows.replay, "host ring + H2D": host_windows}, max(rounds, 15), 1,
                              warmup=3, before=lambda: flush.add_(1)))

    # ---- (b) ---------------------------------------------------------------------------------------------------------------
    X, H, D = (t.clone() for t in f._out)

    def forward_alone():
        with torch.no_grad():
            return net(X, H, D)

    def host_step():
        host.push(reading_host)
        with torch.no_grad():
            return net(*host.windows())

    graph_a, graph_b = capture(forward_alone), capture(forward_alone)
    b = report("(b) one forecast, host time included where the host does work:",
               alternate({"step(host reading): copy + ONE replay": lambda: f.step(reading_host),
                          "step(device reading): ONE replay": lambda: f.step(reading_dev),
                          "forward alone, replayed, capture A": graph_a.replay,
                          "forward alone, replayed, capture B": graph_b.replay,
                          "forward alone, eager": forward_alone,
                          "eager forecaster (hip_graph=False path): push, windows, forward": lambda: (
                              f.push(reading_dev), f.forecast()),
                          "host ring + H2D + eager forward": host_step}, rounds, calls))
    b_cold = report("(b) cold operands (512 MiB overwritten before each call; one call per event pair):",
                    alternate({"step(host reading): copy + ONE replay": lambda: f.step(reading_host),
                               "forward alone, replayed, capture A": graph_a.replay,
                               "forward alone, replayed, capture B": graph_b.replay}, max(rounds, 15), 1, warmup=3,
                              before=lambda: flush.add_(1)))
    fa, fb = b["forward alone, replayed, capture A"], b["forward alone, replayed, capture B"]
    extra = b["step(device reading): ONE replay"] - min(fa, fb)
    say(f"step(device reading) - forward alone = {extra:.2f} us; two captures of the forward alone differ by {abs(fa - fb):.2f} "
        f"us; push + windows replayed on its own takes {a_warm['device ring, replayed']:.2f} us")
    result = {"launches_push_windows": launches, "a_eager_us": a_eager, "a_replayed_warm_us": a_warm, "a_cold_us": a_cold,
              "b_us": b, "b_cold_us": b_cold, "resident_bytes": f.resident_bytes}
    say(json.dumps(result))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
