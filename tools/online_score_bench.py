"""Scoring online forecasts (`OnlineForecaster(score=True)`, msgat_forecast_store / msgat_forecast_score) on one MI355X at
the PEMSD7 serving shape of tools/online_bench.py: one origin per step, R = 5, C = 3, N = 883, tau = 12, T_out = 12,
msgat72 with `missing_edges="scale"`, a point head, book of T_out rows.  HIP events after warm-up, medians over rounds in
which the variants alternate; nothing is asserted except what the variants must share.

  (a) score + store   what scoring adds to a step -- settle one reading against the book (two launches), store one
                      forecast (one launch) -- replayed as ONE captured graph of those three nodes, with cache-resident
                      operands and cold (512 MiB overwritten before every replay, one replay per event pair).  Against it
                      the same totals formed by torch ops on the device (rows gathered through index tensors made from
                      the device clock, nothing read back), launched eagerly and replayed as a captured graph.
  (b) step            `step()` from a reading already on the device with score=True against score=False, two forecasters
                      of the same model in the same process, alternating; warm and cold.

    python tools/online_score_bench.py [--rounds 7] [--calls 20] [--out profiles/online_score] [--name run1.txt]
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
from ms_gat_amd import _lib, data, model, ops  # noqa: E402

DEV, NULL, MASK = ob.DEV, ob.NULL, 0.0


def torch_score_store(reading, pred, book, issued, clock, sums, node_sums, t_out):
    """The totals of ops.forecast_score (K = 1, a point head) and the store of ops.forecast_store by torch ops, with the
    rows taken from the device clock: nothing is read back, so the sequence can be captured too."""
    P = book.shape[0]
    hs = torch.arange(t_out, device=book.device)
    origins = clock[0] - hs
    rows = origins % P
    y = reading[0, 0]
    p = book[rows, :, hs]                                                          # [T_out, N]
    valid = ((issued[rows] == origins) & (origins >= 0))[:, None] & ~torch.isnan(y) & (y != NULL)
    e = p - y
    zero = torch.zeros((), dtype=torch.float64, device=book.device)
    e64 = torch.where(valid, e.double(), zero)
    ape = torch.where(valid & (y > MASK), 100.0 * (e / y).abs().double(), zero)
    cols = torch.stack([valid.double().sum(1), e64.abs().sum(1), ape.sum(1), (e64 * e64).sum(1), e64.sum(1)], dim=1)
    sums[:t_out] += cols
    sums[t_out] += cols.sum(0)
    node_sums += torch.stack([valid.double().sum(0), e64.abs().sum(0), e64.sum(0)], dim=1)
    row = clock[:1] % P
    book.index_copy_(0, row, pred[None])
    issued.index_copy_(0, row, clock[:1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "online_score"))
    ap.add_argument("--name", default="online_score_bench.txt", help="file name under --out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_score_bench.py needs the GPU: there is nothing to time without one")
    rounds, calls, say = a.rounds, a.calls, ob.say
    say(f"# tools/online_score_bench.py --rounds {rounds} --calls {calls} on {torch.cuda.get_device_name(0)}: HIP events, "
        f"medians over rounds, variants alternated inside a round, {os.path.basename(_lib.LIB_PATH)}")
    raw = ob.synthetic_series()
    stats = data.series_stats(raw, ob.HOURS, ob.Q, ob.TAU, input_null_value=NULL)
    L, R, N, T = stats.history, len(ob.HOURS), ob.N, ob.Q
    torch.manual_seed(0)
    net = model.msgat72(n_components=R, in_channels=stats.input_channels, in_timesteps=ob.TAU, out_timesteps=T, use_te=True,
                        adj=ms_gat_amd.synthetic_adjacency(N, ob.EDGES, seed=1), missing_edges="scale").to(DEV)
    scored = ms_gat_amd.OnlineForecaster(net, stats, 0, score=True, score_mask_value=MASK)
    plain = ms_gat_amd.OnlineForecaster(net, stats, 0)
    history = raw[:, :, :L].permute(2, 0, 1).contiguous().to(DEV)
    for f in (scored, plain):
        f.push(history)
    say(f"shape: R={R} C={ob.C_IN} (+1 validity) N={N} tau={ob.TAU} T_out={T}, a point head, book [{T}, {N}, {T}] = "
        f"{T * N * T * 4 / 1e3:.0f} kB, totals [{T + 1}, 5] and [{N}, 3] fp64, slots "
        f"{_lib.lib().msgat_forecast_score_partial_doubles(N, T, 0) * 8 / 1e3:.0f} kB")

    # both forecasters must give the same forecasts, and the kernels' totals those of the torch ops, before anything is timed
    for t in range(L, L + 40):
        r = raw[:, :, t].contiguous()[None].to(DEV)
        prev = scored.step(r).clone()
        assert torch.equal(prev.view(torch.int32), plain.step(r).view(torch.int32)), "scoring changed the forecast"
    clock_before = scored.clock.clone()
    book, issued, sums, node_sums = (x.clone() for x in scored._score_state)
    check_sums, check_nodes = torch.zeros_like(sums), torch.zeros_like(node_sums)
    reading = raw[:, :, L + 40].contiguous()[None].to(DEV)
    pred = prev.clone()
    ops.forecast_score(reading, book, issued, clock_before, T, check_sums, check_nodes, null_value=NULL, mask_value=MASK)
    t_sums, t_nodes = torch.zeros_like(sums), torch.zeros_like(node_sums)
    torch_score_store(reading, pred, book.clone(), issued.clone(), clock_before, t_sums, t_nodes, T)
    torch.cuda.synchronize()
    assert float(check_sums[T, 0]) > 0 and torch.equal(check_sums[:, 0], t_sums[:, 0]) and torch.equal(check_nodes[:, 0], t_nodes[:, 0])
    assert torch.allclose(check_sums, t_sums, rtol=1e-9, atol=1e-9) and torch.allclose(check_nodes, t_nodes, rtol=1e-9, atol=1e-9)
    say(f"40 steps: step() with and without scoring returns the same bits; one reading settled against the book gives "
        f"{int(check_sums[T, 0])} valid entries, counts equal and sums within 1e-9 of the torch ops'")

    # ---- (a) ---------------------------------------------------------------------------------------------------------------
    state = [x.clone() for x in scored._score_state]
    clock = clock_before.clone()
    partials = torch.empty_like(scored._score_partials)

    def library():
        ops.forecast_score(reading, state[0], state[1], clock, T, state[2], state[3], null_value=NULL, mask_value=MASK,
                           partials=partials)
        ops.forecast_store(pred, state[0], state[1], clock)

    t_state = [x.clone() for x in scored._score_state]

    def torch_ops():
        torch_score_store(reading, pred, t_state[0], t_state[1], clock, t_state[2], t_state[3], T)

    say("(a) score + store: device kernels of one eager call (torch.profiler):")
    for label, fn in (("library", library), ("torch ops", torch_ops)):
        names = ob.device_kernels(fn)
        say(f"  {label}: {'not measured' if names is None else len(names)} launches")
        for n in (names or []) if label == "library" else []:
            say(f"      {n[:150]}")
    g_lib, g_torch = ob.capture(library), ob.capture(torch_ops)
    a_warm = ob.report("(a) score + store, cache-resident operands (device time; eager figures include the host's launches):",
                       ob.alternate({"library, replayed (3 nodes)": g_lib.replay, "torch ops, replayed": g_torch.replay,
                                     "library, eager": library, "torch ops, eager": torch_ops}, rounds, calls))
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    a_cold = ob.report("(a) cold operands (512 MiB overwritten before each call; one call per event pair, so the pair's own "
                       "resolution of a few us is in the figure):",
                       ob.alternate({"library, replayed (3 nodes)": g_lib.replay, "torch ops, replayed": g_torch.replay},
                                    max(rounds, 15), 1, warmup=3, before=lambda: flush.add_(1)))

    # ---- (b) ---------------------------------------------------------------------------------------------------------------
    b = ob.report("(b) step(device reading), ONE replay each, two forecasters of one model alternating:",
                  ob.alternate({"score=False": lambda: plain.step(reading), "score=True": lambda: scored.step(reading)},
                               rounds, calls))
    b_cold = ob.report("(b) cold operands (512 MiB overwritten before each call; one call per event pair):",
                       ob.alternate({"score=False": lambda: plain.step(reading), "score=True": lambda: scored.step(reading)},
                                    max(rounds, 15), 1, warmup=3, before=lambda: flush.add_(1)))
    extra, alone = b["score=True"] - b["score=False"], a_warm["library, replayed (3 nodes)"]
    say(f"step(score=True) - step(score=False) = {extra:.2f} us warm, {b_cold['score=True'] - b_cold['score=False']:.2f} us "
        f"cold; the three added nodes replayed on their own take {alone:.2f} us warm, "
        f"{a_cold['library, replayed (3 nodes)']:.2f} us cold")
    result = {"a_warm_us": a_warm, "a_cold_us": a_cold, "b_us": b, "b_cold_us": b_cold,
              "step_extra_us": round(extra, 2), "three_nodes_alone_us": alone}
    say(json.dumps(result))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as fh:
        fh.write("\n".join(ob.LINES) + "\n")


if __name__ == "__main__":
    main()
