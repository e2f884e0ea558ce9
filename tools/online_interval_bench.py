"""Calibrated intervals for online forecasts (`OnlineForecaster(score=True, intervals=...)`, msgat_interval_update /
msgat_interval_apply) on one MI355X at the PEMSD7 serving shape of tools/online_bench.py: one origin per step, R = 5,
C = 3 (+ validity), N = 883, tau = 12, T_out = 12, msgat72 with `missing_edges="scale"`, a point head, score=True, windows
of W = 288 errors, levels (0.8, 0.95).  HIP events after warm-up, medians over rounds in which the variants alternate;
nothing is asserted except what the variants must share.

  (a) update + apply  what the intervals add to a step -- one reading's errors judged and inserted and the radii selected
                      (one launch), lo, hi and the radius book written (one launch) -- replayed as ONE captured graph of
                      those two nodes, with cache-resident operands and cold (512 MiB overwritten before every replay, one
                      replay per event pair).  Against it the same quantities formed by torch ops on the device (a scatter
                      insert, `torch.sort` over [N * T_out, W], compares; rows taken from the device clock, nothing read
                      back), launched eagerly and replayed as a captured graph.
  (b) step            `step()` from a reading already on the device with and without intervals, two forecasters of the
                      same model (both score=True) in the same process, alternating; warm and cold.

    python tools/online_interval_bench.py [--rounds 7] [--calls 20] [--out profiles/online_interval] [--name run1.txt]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ms_gat_amd  # noqa: E402
import online_bench as ob  # noqa: E402
from ms_gat_amd import _lib, data, intervals, model  # noqa: E402

DEV, NULL = ob.DEV, ob.NULL
WINDOW, LEVELS, FILL_STEPS = 288, (0.8, 0.95), 300


def torch_update_apply(reading, pred, book, issued, clock, radius_book, ranks, window, cursor, radius, counts, lo, hi):
    """What intervals.interval_update (K = 1, a point head) and intervals.interval_apply leave, by torch ops with the rows
    taken from the device clock: nothing is read back, so the sequence can be captured too."""
    P, (N, T, W), dev = book.shape[0], window.shape, book.device
    hs = torch.arange(T, device=dev)
    origins = clock[0] - hs
    rows = origins % P
    y = reading[0, 0]
    due = ((issued[rows] == origins) & (origins >= 0))[None] & (~torch.isnan(y) & (y != NULL))[:, None]      # [N, T]
    a = (book[rows, :, hs].t() - y[:, None]).abs()
    r = radius_book[rows, :, :, hs].permute(1, 2, 0)                                                         # [L, N, T]
    judged = due[None] & torch.isfinite(r)
    counts[..., 0] += judged
    counts[..., 1] += judged & (a[None] <= r)
    put = due & torch.isfinite(a)
    c = cursor.long() & 0xFFFFFFFF
    slot = c % W
    old = window.gather(2, slot[..., None])[..., 0]
    window.scatter_(2, slot[..., None], torch.where(put, a, old)[..., None])
    moved = torch.where(put, torch.where(c < W, c + 1, W + (slot + 1) % W), c)
    cursor.copy_(moved.to(torch.int32))
    fill = moved.clamp(max=W)
    inf = torch.full((), float("inf"), device=dev)
    ordered = torch.where(torch.arange(W, device=dev) < fill[..., None], window, inf).sort(dim=-1).values
    rank = ranks.long()[:, fill]                                                                             # [L, N, T]
    picked = ordered[None].expand(rank.shape[0], -1, -1, -1).gather(-1, (rank - 1).clamp(0, W - 1)[..., None])[..., 0]
    radius.copy_(torch.where((rank >= 1) & (rank <= fill), picked, inf))
    p = pred[:, :T]
    lo.copy_(p[None] - radius)
    hi.copy_(p[None] + radius)
    radius_book.index_copy_(0, clock[:1] % P, radius[None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "online_interval"))
    ap.add_argument("--name", default="online_interval_bench.txt", help="file name under --out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_interval_bench.py needs the GPU: there is nothing to time without one")
    rounds, calls, say = a.rounds, a.calls, ob.say
    say(f"# tools/online_interval_bench.py --rounds {rounds} --calls {calls} on {torch.cuda.get_device_name(0)}: HIP "
        f"events, medians over rounds, variants alternated inside a round, {os.path.basename(_lib.LIB_PATH)}")
    raw = ob.synthetic_series()
    stats = data.series_stats(raw, ob.HOURS, ob.Q, ob.TAU, input_null_value=NULL)
    L, R, N, T = stats.history, len(ob.HOURS), ob.N, ob.Q
    torch.manual_seed(0)
    net = model.msgat72(n_components=R, in_channels=stats.input_channels, in_timesteps=ob.TAU, out_timesteps=T, use_te=True,
                        adj=ms_gat_amd.synthetic_adjacency(N, ob.EDGES, seed=1), missing_edges="scale").to(DEV)
    calibrated = ms_gat_amd.OnlineForecaster(net, stats, 0, score=True, intervals=LEVELS, interval_window=WINDOW)
    scored = ms_gat_amd.OnlineForecaster(net, stats, 0, score=True)
    history = raw[:, :, :L].permute(2, 0, 1).contiguous().to(DEV)
    for f in (calibrated, scored):
        f.push(history)
    n_levels = len(LEVELS)
    say(f"shape: R={R} C={ob.C_IN} (+1 validity) N={N} tau={ob.TAU} T_out={T}, a point head, score=True, W={WINDOW}, levels "
        f"{LEVELS}: window [{N}, {T}, {WINDOW}] = {N * T * WINDOW * 4 / 1e6:.1f} MB, radius [{n_levels}, {N}, {T}], radius "
        f"book [{T}, {n_levels}, {N}, {T}] = {T * n_levels * N * T * 4 / 1e6:.2f} MB, counts [{n_levels}, {N}, {T}, 2] int64")

    # both forecasters must give the same forecasts, and the kernels' state that of the torch ops, before anything is timed
    for t in range(L, L + FILL_STEPS):
        r = raw[:, :, t].contiguous()[None].to(DEV)
        prev = calibrated.step(r).clone()
        if t < L + 40:
            assert torch.equal(prev.view(torch.int32), scored.step(r).view(torch.int32)), "the intervals changed the forecast"
        else:
            scored.step(r)
    reading = raw[:, :, L + FILL_STEPS].contiguous()[None].to(DEV)
    pred = prev.clone()
    clock = calibrated.clock.clone()
    book, issued = calibrated._score_state[0].clone(), calibrated._score_state[1].clone()
    ranks = calibrated._interval_ranks

    def fresh():
        return [x.clone() for x in calibrated._interval_state] + [torch.zeros_like(x) for x in calibrated._interval_out]

    def library_on(s):
        window, cursor, radius, radius_book, counts, lo, hi = s
        intervals.interval_update(reading, book, issued, clock, radius_book, ranks, window, cursor, radius, counts,
                                  null_value=NULL)
        intervals.interval_apply(pred, radius, clock, lo, hi, radius_book)

    def torch_on(s):
        window, cursor, radius, radius_book, counts, lo, hi = s
        torch_update_apply(reading, pred, book, issued, clock, radius_book, ranks, window, cursor, radius, counts, lo, hi)

    check, t_check = fresh(), fresh()
    before = int(check[4][..., 0].sum())
    library_on(check)
    torch_on(t_check)
    torch.cuda.synchronize()
    for name, x, y in zip(("window", "cursor", "radius", "radius_book", "counts", "lo", "hi"), check, t_check):
        assert torch.equal(x, y), f"{name}: the kernels and the torch ops disagree"
    fill = (check[1].long() & 0xFFFFFFFF).clamp(max=WINDOW)
    got = calibrated.interval_scores()
    say(f"{FILL_STEPS} steps: step() with and without intervals returns the same bits (40 compared); windows hold "
        f"{int(fill.min())} to {int(fill.max())} errors; one reading judged {int(check[4][..., 0].sum()) - before} issued "
        f"intervals and every state tensor equals the torch ops'; coverage so far {[round(c, 4) for c in got['coverage']]} "
        f"for levels {got['levels']} over {got['judged']} judged, mean width {[round(w, 2) for w in got['width']]}")

    # ---- (a) ---------------------------------------------------------------------------------------------------------------
    state, t_state = fresh(), fresh()
    library = lambda: library_on(state)  # noqa: E731
    torch_ops = lambda: torch_on(t_state)  # noqa: E731
    say("(a) update + apply: device kernels of one eager call (torch.profiler):")
    for label, fn in (("library", library), ("torch ops", torch_ops)):
        names = ob.device_kernels(fn)
        say(f"  {label}: {'not measured' if names is None else len(names)} launches")
        for n in (names or []) if label == "library" else []:
            say(f"      {n[:150]}")
    g_lib, g_torch = ob.capture(library), ob.capture(torch_ops)
    a_warm = ob.report("(a) update + apply, cache-resident operands (device time; eager figures include the host's launches):",
                       ob.alternate({"library, replayed (2 nodes)": g_lib.replay, "torch ops, replayed": g_torch.replay,
                                     "library, eager": library, "torch ops, eager": torch_ops}, rounds, calls))
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device=DEV)
    a_cold = ob.report("(a) cold operands (512 MiB overwritten before each call; one call per event pair, so the pair's own "
                       "resolution of a few us is in the figure):",
                       ob.alternate({"library, replayed (2 nodes)": g_lib.replay, "torch ops, replayed": g_torch.replay},
                                    max(rounds, 15), 1, warmup=3, before=lambda: flush.add_(1)))

    # ---- (b) ---------------------------------------------------------------------------------------------------------------
    variants = {"intervals=None": lambda: scored.step(reading), f"intervals={LEVELS}": lambda: calibrated.step(reading)}
    b = ob.report("(b) step(device reading), ONE replay each, two forecasters of one model alternating:",
                  ob.alternate(variants, rounds, calls))
    b_cold = ob.report("(b) cold operands (512 MiB overwritten before each call; one call per event pair):",
                       ob.alternate(variants, max(rounds, 15), 1, warmup=3, before=lambda: flush.add_(1)))
    with_, without = f"intervals={LEVELS}", "intervals=None"
    extra, alone = b[with_] - b[without], a_warm["library, replayed (2 nodes)"]
    say(f"step(intervals) - step(no intervals) = {extra:.2f} us warm, {b_cold[with_] - b_cold[without]:.2f} us cold; the two "
        f"added nodes replayed on their own take {alone:.2f} us warm, {a_cold['library, replayed (2 nodes)']:.2f} us cold; "
        f"the window is {N * T * WINDOW * 4 / 1e6:.1f} MB read per step")
    result = {"a_warm_us": a_warm, "a_cold_us": a_cold, "b_us": b, "b_cold_us": b_cold,
              "step_extra_us": round(extra, 2), "two_nodes_alone_us": alone}
    say(json.dumps(result))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        fh.write("\n".join(ob.LINES) + "\n")


if __name__ == "__main__":
    main()
