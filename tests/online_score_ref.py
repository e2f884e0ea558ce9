"""Shared by test_online_score_cpu.py and test_gpu_online_score.py: what scoring online forecasts must give.

`store_ref` / `score_ref` restate `msgat_forecast_store` / `msgat_forecast_score` in numpy in the summation order
include/msgat_hip.h documents -- fp32 per-entry terms, fp64 sums, a lane per node adding k then h, nodes in order inside
tiles of 64, tiles in order, horizons in order for the last row -- so the kernels must agree with them bit for bit.
`brute_force` knows nothing of books, stamps or orders: it takes the forecasts that were issued and the raw series,
enumerates per horizon the (forecast, reading) pairs that are due and sums with `math.fsum`."""
import math

import numpy as np

NEVER = -2 ** 63
TILE = 64
F32, F64 = np.float32, np.float64


def columns(n_levels):
    return 5 if not n_levels else 7 + 2 * n_levels


def entry_terms(p, y, levels, point, mask_value):
    """p [max(Q, 1), n] fp32 forecasts and y [n] fp32 truths -> [W, n] float64 terms, the fp32 arithmetic of the kernel."""
    p, y = np.asarray(p, F32), np.asarray(y, F32)
    with np.errstate(all="ignore"):
        e = p[point] - y
        ape = np.where(y > F32(mask_value), 100.0 * np.abs(e / y).astype(F64), 0.0)
        rows = [np.ones(y.shape, F64), np.abs(e).astype(F64), ape, e.astype(F64) * e.astype(F64), e.astype(F64)]
        if levels:
            tau = np.asarray(levels, F32)
            tau_m1 = (tau.astype(F64) - 1.0).astype(F32)
            u = y[None] - p
            rho = np.maximum(tau[:, None] * u, tau_m1[:, None] * u)
            rows += [(p[:-1] > p[1:]).any(0).astype(F64), (p[-1] - p[0]).astype(F64), *(y[None] <= p).astype(F64),
                     *rho.astype(F64)]
    return np.stack(rows)


def valid_entries(y, null_value):
    ok = ~np.isnan(y)
    return ok if null_value is None else ok & (y != F32(null_value))


def store_ref(pred, book, issued, clock):
    """In place: pred [N,out] into row clock[0] mod P of book [P,N,out], issued[row] = clock[0]."""
    t = int(clock[0])
    row = t % book.shape[0]                                   # Python's % is the floor-mod
    book[row] = pred
    issued[row] = t


def score_ref(raw, book, issued, clock, t_out, levels, point, null_value, mask_value, sums, node_sums):
    """In place on sums [t_out + 1, W] and node_sums [N, 3] (float64): raw [K,C,N] are the steps clock[0] + k."""
    P, N = book.shape[0], book.shape[1]
    n_levels, W = max(len(levels), 1), columns(len(levels))
    s = int(clock[0])
    part = np.zeros((W, t_out, N), F64)                       # a lane's slots, +0.0 at k = 0
    node = np.zeros((N, 3), F64)
    for k in range(raw.shape[0]):
        y = raw[k, 0]
        valid = valid_entries(y, null_value)
        for h in range(t_out):
            o = s + k - h
            row = o % P
            if o < 0 or int(issued[row]) != o:
                continue
            p = book[row].reshape(N, n_levels, t_out)[:, :, h].T
            t = entry_terms(p, y, levels, point, mask_value)
            part[:, h] = np.where(valid, part[:, h] + t, part[:, h])
            for j, c in enumerate((0, 1, 4)):                 # the lane's node totals: k, then h
                node[:, j] = np.where(valid, node[:, j] + t[c], node[:, j])
    node_sums += node
    total = np.zeros((W, t_out), F64)
    for base in range(0, N, TILE):                            # block b of the first launch ...
        tile = np.zeros((W, t_out), F64)
        for n in range(base, min(base + TILE, N)):            # ... its lanes in order
            tile = tile + part[:, :, n]
        total = total + tile                                  # blocks in order
    sums[:t_out] += total.T
    every = np.zeros(W, F64)
    for h in range(t_out):                                    # the last row: horizons in order
        every = every + total[:, h]
    sums[t_out] += every


def brute_force(pairs, raw, stop_step, t_out, levels=(), point=0, null_value=None, mask_value=0.0, first_step=0):
    """pairs: (origin, forecast [N, out]) of every forecast issued, in any order (one origin twice: the same forecast).
    raw [C, N, total] is the raw series on the forecaster's time base; the readings of the steps first_step ..
    stop_step - 1 were pushed while those forecasts were in the book.  A forecast of origin o is due at horizon h when
    step o + h is pushed.  Returns per horizon (row t_out: all) and per node the exact sums, the sums of |term| and the
    numbers of terms, plus what the cases must show they exercise."""
    raw = np.asarray(raw, F32)
    N = raw.shape[1]
    n_levels, W = max(len(levels), 1), columns(len(levels))
    forecasts = {int(o): np.asarray(f, F32).reshape(N, n_levels, t_out) for o, f in pairs}
    terms = [[[] for _ in range(W)] for _ in range(t_out + 1)]
    node_terms = [[[] for _ in range(3)] for _ in range(N)]
    seen = {"null_masked": 0, "mape_left_out": 0}
    for o, f in sorted(forecasts.items()):
        for h in range(t_out):
            step = o + h
            if not first_step <= step < stop_step or step < 0 or step >= raw.shape[2]:
                continue
            y = raw[0, :, step]
            valid = valid_entries(y, null_value)
            if null_value is not None:
                seen["null_masked"] += int((~np.isnan(y) & ~valid).sum())
            seen["mape_left_out"] += int((valid & ~(y > F32(mask_value))).sum())
            t = entry_terms(f[:, :, h].T, y, levels, point, mask_value)
            for n in np.nonzero(valid)[0]:
                for c in range(W):
                    terms[h][c].append(float(t[c, n]))
                    terms[t_out][c].append(float(t[c, n]))
                for j, c in enumerate((0, 1, 4)):
                    node_terms[n][j].append(float(t[c, n]))
    pack = lambda lists: (np.array([[math.fsum(v) for v in row] for row in lists]),  # noqa: E731
                          np.array([[math.fsum(abs(x) for x in v) for v in row] for row in lists]),
                          np.array([[len(v) for v in row] for row in lists]))
    sums, sums_abs, sums_n = pack(terms)
    node, node_abs, node_n = pack(node_terms)
    return {"sums": sums, "abs": sums_abs, "n": sums_n, "node": node, "node_abs": node_abs, "node_n": node_n, **seen}


def assert_within_double_sum_bound(got, want, abs_sum, n, what=""):
    """|got - want| <= (n - 1) 2^-53 sum |term| elementwise: the bound of a double sum of n terms."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    bound = np.maximum(np.asarray(n, F64) - 1.0, 0.0) * 2.0 ** -53 * np.asarray(abs_sum, F64)
    bad = np.abs(got - want) > bound
    assert not bad.any(), (what, got[bad], want[bad], bound[bad])


def assert_equal_brute_force(sums, node_sums, want, n_levels, what=""):
    """Counts, crossings and hits (sums of 0.0 and 1.0) exact, every other sum within the bound of a double sum."""
    sums, node_sums = np.asarray(sums, F64), np.asarray(node_sums, F64)
    exact = [0] + ([5, *range(7, 7 + n_levels)] if n_levels else [])
    assert np.array_equal(sums[:, exact], want["sums"][:, exact]), (what, "counts")
    assert np.array_equal(sums[:, 0], want["n"][:, 0].astype(F64)), (what, "count column")
    assert np.array_equal(node_sums[:, 0], want["node"][:, 0]), (what, "node counts")
    assert_within_double_sum_bound(sums, want["sums"], want["abs"], want["n"], (what, "sums"))
    assert_within_double_sum_bound(node_sums, want["node"], want["node_abs"], want["node_n"], (what, "node_sums"))
