"""Times the device-resident input windows (`ops.window_gather`, `data.DeviceWindows`) on one GPU:

    python tools/device_windows_bench.py [--launches 256] [--steps 200] [--repeats 3] [--only kernel|imputed|epoch]

Shape: the PEMSD7 training shape, B = 32, in_hours = [1, 2, 3, 24, 168], C = 3, N = 883, tau = q = 12, a seeded synthetic
series (28224 steps for the epoch: 299 MB normalised + 100 MB target).

(a) kernel: `msgat_window_gather` on shuffled origins with COLD caches: a series of 4 x 28224 steps (1.6 GB resident), 32
    origin sets in rotation, each into X / Y buffers of its own, so that a rotation reads about 430 MB of series rows and
    writes 694 MB -- past the 256 MiB last-level cache on both sides.  The 32 launches are captured in ONE HIP graph and
    replayed: device time per launch between two events, mean of `--launches` launches after a warm-up.  Next to it
    the floor, timed the same way: `copy_` of set i's X and Y into a second set of buffers (the same bytes written,
    from a contiguous read, equally cold).  For contrast the WARM figures (one origin set, one pair of buffers, over and
    over: everything cache-resident) and the eager call (`ops.window_gather`: three allocations and the launch, host
    time included).
(i) imputed: `msgat_window_gather_imputed` (missing readings filled in, with and without the validity channel) beside the
    plain gather on one series with 1 % missing readings and two dead sensors, cold and warm as in (a), with the bytes
    each variant asks for.
(b) epoch: `Trainer.run_epoch(mode="train")` of msgat72 (R = 5, hip_graph="auto", one model and trainer throughout) over
    `--steps` steps after the step's graph is captured, host clock around the epoch ending in a synchronise, fed by
      host0 / host2 / host4   `make_loaders(...)` DataLoaders with num_workers = 0 / 2 / 4 (pinned, copied per step)
      device                  `make_loaders(..., device=...)`: DeviceWindows
      resident                one synthetic batch already on the device, every step (what bench.py times)
    alternating, `--repeats` times each.  Prints one line per measurement and one JSON line at the end.
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ms_gat_amd  # noqa: E402
from ms_gat_amd import data, engine, model, ops  # noqa: E402

SHAPE = dict(B=32, hours=[1, 2, 3, 24, 168], C=3, N=883, E=866, tau=12, q=12, T_total=28224)


def series(total, seed=0):
    """[C, N, total] fp32, seeded: a daily wave plus noise per (channel, node), like data.SyntheticPEMS."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(total, dtype=torch.float32)
    base = 200 + 80 * torch.rand(SHAPE["C"], SHAPE["N"], 1, generator=g)
    raw = base * (1 + 0.4 * torch.sin(2 * torch.pi * t / (24 * SHAPE["tau"])))
    raw += 15 * torch.randn(SHAPE["C"], SHAPE["N"], total, generator=g)
    return raw.clamp_min_(1.0)


def event_us(fn, calls, launches_per_call, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (calls * launches_per_call)


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def kernel_part(dev, launches, repeats):
    """COLD: a series four times the PEMSD7 length (1.2 GB + 0.4 GB target), `n_sets` = 32 origin sets of 32 shuffled
    origins, every set with X / Y buffers of its own: one rotation reads about 430 MB of series rows (32 * 32 * 60 rows of
    10.6 KB, few shared) and writes 694 MB, so no launch finds its rows, or the lines it writes, in the 256 MiB cache.
    The copy floor rotates the same way: set i's X, Y are copied into a second set of buffers (1.4 GB per rotation).
    WARM, for contrast: one origin set into one pair of buffers, over and over (everything cache-resident)."""
    from ms_gat_amd import _lib
    s = dict(SHAPE, T_total=4 * SHAPE["T_total"])
    raw = series(s["T_total"])
    intervals, train_end = data.split_intervals(s["T_total"], s["hours"], s["q"], s["tau"])
    resident = data.upload_series(data.zscore(raw, split=train_end), raw[0], dev)
    del raw
    n_sets = 32
    lo, hi = intervals[0]
    order = (torch.randperm(hi - lo, generator=torch.Generator().manual_seed(1))[: n_sets * s["B"]] + lo).to(dev)
    sets = [order[i * s["B"]: (i + 1) * s["B"]] for i in range(n_sets)]
    offsets = ops.window_offsets(s["hours"], s["tau"], dev)
    outs = [ops.window_gather(*resident, o, s["hours"], s["tau"], s["q"], offsets=offsets) for o in sets]
    seconds = [(torch.empty_like(x), torch.empty_like(y)) for x, _, _, y in outs]
    L, stream = _lib.lib(), _lib.stream_handle

    def launch(o, out):     # the C entry point into fixed outputs: nothing but the launch
        x, h, d, y = out
        _lib.check(L.msgat_window_gather(resident[0].data_ptr(), resident[1].data_ptr(), o.data_ptr(), offsets.data_ptr(),
                                         x.data_ptr(), h.data_ptr(), d.data_ptr(), y.data_ptr(), s["B"], len(s["hours"]),
                                         s["C"], s["N"], s["T_total"], s["tau"], s["q"], s["tau"] * max(s["hours"]),
                                         stream(dev)), "msgat_window_gather")

    def gather_cold():
        for o, out in zip(sets, outs):
            launch(o, out)

    def gather_warm():
        for _ in range(n_sets):
            launch(sets[0], outs[0])

    def gather_eager():
        for o in sets:
            ops.window_gather(*resident, o, s["hours"], s["tau"], s["q"], offsets=offsets)

    def copy_cold():
        for (x, _, _, y), (x2, y2) in zip(outs, seconds):
            x2.copy_(x)
            y2.copy_(y)

    def copy_warm():
        for _ in range(n_sets):
            seconds[0][0].copy_(outs[0][0])
            seconds[0][1].copy_(outs[0][3])

    calls = max(1, -(-launches // n_sets))
    runs = {"gather_cold": graph_of(gather_cold).replay, "copy_cold": graph_of(copy_cold).replay,
            "gather_warm": graph_of(gather_warm).replay, "copy_warm": graph_of(copy_warm).replay,
            "gather_eager": gather_eager}
    times = {k: [] for k in runs}
    for r in range(repeats):
        for k, fn in runs.items():       # alternated
            times[k].append(event_us(fn, calls, n_sets))
        print(f"kernel round {r + 1}: " + "  ".join(f"{k} {v[-1]:7.2f} us" for k, v in times.items()), flush=True)
    x, _, _, y = outs[0]
    written = 4 * (x.numel() + y.numel()) + 16 * s["B"]
    rows = torch.unique((order[:, None, None] - offsets[None, :, None] + torch.arange(s["tau"], device=dev)).flatten()).numel()
    out = {"T_total": s["T_total"], "bytes_written": written, "launches_per_figure": calls * n_sets, "origin_sets": n_sets,
           "resident_bytes": 4 * s["T_total"] * s["N"] * (s["C"] + 1),
           "series_bytes_read_per_rotation": rows * 4 * s["C"] * s["N"], "bytes_written_per_rotation": written * n_sets}
    for k, v in times.items():
        out[f"{k}_us_median"] = round(statistics.median(v), 2)
        out[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    for k in ("cold", "warm"):
        out[f"gather_{k}_TB_per_s_written"] = round(written / out[f"gather_{k}_us_median"] * 1e-6, 3)
        out[f"copy_{k}_TB_per_s_written"] = round((written - 16 * s["B"]) / out[f"copy_{k}_us_median"] * 1e-6, 3)
        out[f"gather_over_copy_{k}"] = round(out[f"gather_{k}_us_median"] / out[f"copy_{k}_us_median"], 3)
    return out


def imputed_part(dev, launches, repeats):
    """`msgat_window_gather_imputed` beside `msgat_window_gather`, in one process on one series: the 4 x 28224 steps of
    `kernel_part`, z-scored, with 1 % of its (node, step) readings in runs and two dead sensors stored as NaN
    (`SyntheticPEMS.outages`), and a table of one week's slots (2016 x C x N, 21 MB; random values: they do not matter to
    the time).  COLD and WARM as in `kernel_part`; the plain gather copies the same series, NaNs included.  Next to the
    times the bytes each variant asks for per launch: X reads B R tau C N words (once more for the validity channel, whose
    lanes read the C words of their node again), Y reads what it writes, X writes B R C' N tau words."""
    from ms_gat_amd import _lib
    s = dict(SHAPE, T_total=4 * SHAPE["T_total"])
    raw = series(s["T_total"])
    intervals, train_end = data.split_intervals(s["T_total"], s["hours"], s["q"], s["tau"])
    normed = data.zscore(raw, split=train_end)
    down = data.SyntheticPEMS.outages(s["N"], s["T_total"], s["tau"], 0.01, 2, seed=2)
    normed[:, down] = float("nan")
    resident = data.upload_series(normed, raw[0], dev)
    period = 7 * 24 * s["tau"]
    table = torch.randn(period, s["C"], s["N"], generator=torch.Generator().manual_seed(3)).to(dev)
    missing_share = float(down.float().mean())
    del raw, normed, down
    n_sets = 32
    lo, hi = intervals[0]
    order = (torch.randperm(hi - lo, generator=torch.Generator().manual_seed(1))[: n_sets * s["B"]] + lo).to(dev)
    sets = [order[i * s["B"]: (i + 1) * s["B"]] for i in range(n_sets)]
    offsets = ops.window_offsets(s["hours"], s["tau"], dev)
    outs = {"plain": [ops.window_gather(*resident, o, s["hours"], s["tau"], s["q"], offsets=offsets) for o in sets]}
    for name, mask in (("imputed", False), ("imputed_mask", True)):
        outs[name] = [ops.window_gather_imputed(resident[0], table, resident[1], o, s["hours"], s["tau"], s["q"],
                                                mask_channel=mask, offsets=offsets) for o in sets]
    assert not any(bool(torch.isnan(out[0]).any()) for out in outs["imputed_mask"])
    L, stream = _lib.lib(), _lib.stream_handle
    dims = (s["B"], len(s["hours"]), s["C"], s["N"], s["T_total"], s["tau"], s["q"], s["tau"] * max(s["hours"]))

    def launch(name, o, out):     # the C entry points into fixed outputs: nothing but the launch
        x, h, d, y = out
        if name == "plain":
            st = L.msgat_window_gather(resident[0].data_ptr(), resident[1].data_ptr(), o.data_ptr(), offsets.data_ptr(),
                                       x.data_ptr(), h.data_ptr(), d.data_ptr(), y.data_ptr(), *dims, stream(dev))
        else:
            st = L.msgat_window_gather_imputed(resident[0].data_ptr(), table.data_ptr(), resident[1].data_ptr(), o.data_ptr(),
                                               offsets.data_ptr(), x.data_ptr(), h.data_ptr(), d.data_ptr(), y.data_ptr(),
                                               *dims, period, int(name == "imputed_mask"), stream(dev))
        _lib.check(st, name)

    def cold(name):
        def run():
            for o, out in zip(sets, outs[name]):
                launch(name, o, out)
        return run

    def warm(name):
        def run():
            for _ in range(n_sets):
                launch(name, sets[0], outs[name][0])
        return run

    calls = max(1, -(-launches // n_sets))
    runs = {f"{name}_{k}": graph_of(make(name)).replay for k, make in (("cold", cold), ("warm", warm)) for name in outs}
    times = {k: [] for k in runs}
    for r in range(repeats):
        for k, fn in runs.items():       # alternated
            times[k].append(event_us(fn, calls, n_sets))
        print(f"imputed round {r + 1}: " + "  ".join(f"{k} {v[-1]:7.2f} us" for k, v in times.items()), flush=True)
    x_words = s["B"] * len(s["hours"]) * s["C"] * s["N"] * s["tau"]
    y_bytes = 4 * s["B"] * s["N"] * s["q"]
    asked = {"plain": {"read": 4 * x_words + y_bytes, "written": 4 * x_words + y_bytes + 16 * s["B"]}}
    asked["imputed"] = {"read": asked["plain"]["read"] + round(4 * x_words * missing_share), "written": asked["plain"]["written"]}
    asked["imputed_mask"] = {"read": asked["imputed"]["read"] + 4 * x_words,
                             "written": asked["plain"]["written"] + 4 * x_words // s["C"]}
    out = {"T_total": s["T_total"], "period": period, "missing_share": round(missing_share, 5),
           "launches_per_figure": calls * n_sets, "origin_sets": n_sets, "bytes_asked_per_launch": asked}
    for k, v in times.items():
        out[f"{k}_us_median"] = round(statistics.median(v), 2)
        out[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    for k in ("cold", "warm"):
        plain = out[f"plain_{k}_us_median"]
        out[f"plain_{k}_spread"] = round((max(times[f"plain_{k}"]) - min(times[f"plain_{k}"])) / plain, 4)
        for name in ("imputed", "imputed_mask"):
            out[f"{name}_over_plain_{k}"] = round(out[f"{name}_{k}_us_median"] / plain, 3)
    for name in ("imputed", "imputed_mask"):
        out[f"{name}_over_plain_bytes_written"] = round(asked[name]["written"] / asked["plain"]["written"], 3)
        out[f"{name}_over_plain_bytes_moved"] = round(sum(asked[name].values()) / sum(asked["plain"].values()), 3)
    return out


class _First:
    """The first `n` batches of a loader, with what `Engine.run_epoch` looks for on it."""

    def __init__(self, loader, n):
        self.loader, self.n = loader, n
        self.batch_sampler = getattr(loader, "batch_sampler", None)
        self.msgat_sharded = getattr(loader, "msgat_sharded", False)

    def __iter__(self):
        return itertools.islice(iter(self.loader), self.n)


def epoch_part(raw, dev, steps, repeats):
    s = SHAPE
    torch.manual_seed(0)
    adj = ms_gat_amd.synthetic_adjacency(s["N"], s["E"], seed=0)
    net = model.build_msgat("ms-gat72", n_components=len(s["hours"]), in_channels=s["C"], in_timesteps=s["tau"],
                            out_timesteps=s["q"], use_te=True, adj=adj).to(dev)
    tmp = tempfile.TemporaryDirectory()
    trainer = engine.Trainer(net, 50.0, tmp.name)
    assert trainer.hip_graph == "auto"
    args = (raw, s["hours"], s["q"], s["tau"], s["B"])
    sources = {f"host{w}": data.make_loaders(*args, num_workers=w)[0] for w in (0, 2, 4)}
    sources["device"] = data.make_loaders(*args, device=dev)[0]
    first = next(iter(sources["device"]))
    sources["resident"] = [[t.clone() for t in first]] * steps
    assert len(sources["device"]) >= steps, "the training split is shorter than the timed epoch"
    trainer.run_epoch(_First(sources["device"], 8), gpu_id=dev.index, epoch=0, mode="train")     # captures the step
    assert len(trainer._graphs) == 1
    times = {k: [] for k in sources}
    for r in range(repeats):
        for k, src in sources.items():       # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.run_epoch(src if k == "resident" else _First(src, steps), gpu_id=dev.index, epoch=r + 1, mode="train")
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps * 1e3)
        print(f"epoch round {r + 1}: " + "  ".join(f"{k} {v[-1]:7.3f} ms/step" for k, v in times.items()), flush=True)
    assert len(trainer._graphs) == 1, "a source changed the batch's shapes"
    out = {"steps_per_epoch": steps, "repeats": repeats, "resident_bytes": sources["device"].resident_bytes}
    for k, v in times.items():
        med = statistics.median(v)
        out[f"{k}_ms_per_step_median"] = round(med, 3)
        out[f"{k}_ms_per_step_min_max"] = [round(min(v), 3), round(max(v), 3)]
        out[f"{k}_samples_per_s"] = round(s["B"] / med * 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["kernel", "imputed", "epoch"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_windows_bench.py needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    out = {"shape": SHAPE}
    if a.only in (None, "kernel"):
        out["kernel"] = kernel_part(dev, a.launches, max(a.repeats, 3))
        torch.cuda.empty_cache()
    if a.only in (None, "imputed"):
        out["imputed"] = imputed_part(dev, a.launches, max(a.repeats, 3))
        torch.cuda.empty_cache()
    if a.only in (None, "epoch"):
        out["epoch"] = epoch_part(series(SHAPE["T_total"]), dev, a.steps, a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
