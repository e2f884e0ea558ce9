"""Shared by test_online_interval_cpu.py and test_gpu_online_interval.py: what calibrating online forecasts must give.

`update_ref` / `apply_ref` restate `msgat_interval_update` / `msgat_interval_apply` in numpy as include/msgat_hip.h
documents them -- a series at a time: judged, then inserted at the cursor's slot, the cursor's wrap, the radius as an
element of the sorted filled slots -- so the kernels must agree with them bit for bit in every state tensor.
`BruteForce` knows nothing of rings, cursors, books or stamps: per series it keeps the list of valid finite errors in
arrival order, its radius is the rank-th smallest of the last W of them (the rank from exact rational arithmetic of its
own), and it judges every error against the radius that was current when its forecast was issued.
`StandIn` is the torch stand-in model of the forecaster tests."""
import math
from fractions import Fraction

import numpy as np
from torch import nn

from online_fixtures import HOURS
from online_score_ref import NEVER, store_ref, valid_entries  # noqa: F401  (re-exported for the tests)

F32 = np.float32
INF = F32(np.inf)


def wrap64(x):
    """A Python integer as the two's-complement int64 the kernel's clock arithmetic gives."""
    return (int(x) + 2 ** 63) % 2 ** 64 - 2 ** 63


def fresh_state(L, N, T, W, P):
    """(window, cursor, radius, radius_book, counts) as `intervals.interval_state` makes them."""
    return (np.zeros((N, T, W), F32), np.zeros((N, T), np.int32), np.full((L, N, T), INF, F32),
            np.full((P, L, N, T), INF, F32), np.zeros((L, N, T, 2), np.int64))


def update_ref(raw, book, issued, clock, radius_book, ranks, window, cursor, radius, counts, point=0, null_value=None):
    """In place on window, cursor, radius and counts: raw [K,C,N] are the steps clock[0] + k."""
    P, N, out = book.shape
    L, _, T = radius.shape
    W = window.shape[2]
    s = int(clock[0])
    valid = [valid_entries(raw[k, 0], null_value) for k in range(raw.shape[0])]
    for n in range(N):
        for h in range(T):
            c = int(cursor[n, h]) & 0xFFFFFFFF                         # the word as uint32
            for k in range(raw.shape[0]):
                o = wrap64(wrap64(s + k) - h)
                row = o % P                                            # Python's % is the floor-mod
                if o < 0 or int(issued[row]) != o or not valid[k][n]:
                    continue
                with np.errstate(all="ignore"):
                    a = np.abs(F32(book[row, n, point * T + h]) - F32(raw[k, 0, n]))
                for l in range(L):                                     # judged first
                    r = radius_book[row, l, n, h]
                    if np.isfinite(r):
                        counts[l, n, h, 0] += 1
                        counts[l, n, h, 1] += int(a <= r)
                if not np.isfinite(a):
                    continue
                slot = c % W
                window[n, h, slot] = a
                c = c + 1 if c < W else W + (slot + 1) % W
            cursor[n, h] = np.array(c, np.uint32).view(np.int32)
            fill = min(c, W)
            held = np.sort(window[n, h, :fill].view(np.uint32))        # non-negative finite values order as their bits
            for l in range(L):
                rank = int(ranks[l, fill])
                radius[l, n, h] = held[rank - 1: rank].view(F32)[0] if 1 <= rank <= fill else INF


def apply_ref(pred, radius, clock, lo, hi, radius_book, point=0):
    """In place on lo, hi [L,N,T] and row clock[0] mod P of radius_book [P,L,N,T]."""
    T = radius.shape[2]
    p = np.asarray(pred, F32)[:, point * T: (point + 1) * T]
    with np.errstate(all="ignore"):
        lo[:] = p[None] - radius
        hi[:] = p[None] + radius
    radius_book[int(clock[0]) % radius_book.shape[0]] = radius


def rank_of(level, m, min_count=1):
    """ceil((m + 1) level) in exact arithmetic if it exists among m values and m >= min_count, else 0."""
    rank = math.ceil((m + 1) * Fraction(level).limit_denominator(10 ** 6))
    return rank if rank <= m and m >= min_count else 0


class BruteForce:
    """`issue(origin, forecast [N, out])` when a forecast is made, `push(step)` when the reading of a step arrives (raw
    [C, N, total] is the series on the forecaster's time base), in the order things happen."""

    def __init__(self, raw, t_out, levels, window, min_count=None, point=0, null_value=None):
        self.raw, self.T, self.levels, self.W = np.asarray(raw, F32), t_out, tuple(levels), window
        self.min_count = 1 if min_count is None else min_count
        self.point, self.null = point, null_value
        self.N = self.raw.shape[1]
        self.errors = [[[] for _ in range(t_out)] for _ in range(self.N)]
        self.judged = np.zeros((len(levels), self.N, t_out), np.int64)
        self.covered = np.zeros_like(self.judged)
        self.forecasts, self.issued_radius = {}, {}
        self.null_masked = self.nan_judged = 0

    def radius(self):
        r = np.full((len(self.levels), self.N, self.T), INF, F32)
        for n in range(self.N):
            for h in range(self.T):
                last = sorted(self.errors[n][h][-self.W:])
                for l, level in enumerate(self.levels):
                    rank = rank_of(level, len(last), self.min_count)
                    if rank:
                        r[l, n, h] = last[rank - 1]
        return r

    def issue(self, origin, forecast):
        """-> (lo, hi, r) of this forecast, each [L, N, T]."""
        p = np.asarray(forecast, F32).reshape(self.N, -1, self.T)[:, self.point]
        r = self.radius()
        self.forecasts[origin], self.issued_radius[origin] = p, r
        with np.errstate(all="ignore"):
            return p[None] - r, p[None] + r, r

    def push(self, step):
        y = self.raw[0, :, step]
        valid = valid_entries(y, self.null)
        for h in range(self.T):
            origin = step - h
            if origin not in self.forecasts:
                continue
            self.null_masked += int((~np.isnan(y) & ~valid).sum())
            with np.errstate(all="ignore"):
                a = np.abs(self.forecasts[origin][:, h] - y)
            r = self.issued_radius[origin][:, :, h]
            for n in np.nonzero(valid)[0]:
                for l in range(len(self.levels)):
                    if np.isfinite(r[l, n]):
                        self.judged[l, n, h] += 1
                        self.covered[l, n, h] += int(a[n] <= r[l, n])
                        self.nan_judged += int(np.isnan(a[n]))
                if np.isfinite(a[n]):
                    self.errors[n][h].append(a[n])

    def inserts(self):
        return np.array([[len(v) for v in row] for row in self.errors])

    def cursor(self):
        """What the ring's cursor word is after that many inserts: m below W, then W + (m - W) mod W."""
        m = self.inserts()
        return np.where(m < self.W, m, self.W + (m - self.W) % self.W).astype(np.int32)

    def counts(self):
        return np.stack([self.judged, self.covered], axis=-1)


class StandIn(nn.Module):
    """(X [B,R,C,N,T], H [B], D [B]) -> [B,N,out] near the scale of the readings: every input moves the output."""

    def __init__(self, in_channels, out, tau):
        super().__init__()
        self.in_channels = in_channels
        self.proj = nn.Linear(len(HOURS) * in_channels * tau, out)
        self.h_ebd, self.d_ebd = nn.Embedding(24, out), nn.Embedding(7, out)

    def forward(self, X, H, D):
        B, R, C_, N, T = X.shape
        y = self.proj(X.permute(0, 3, 1, 2, 4).reshape(B, N, R * C_ * T)) + (self.h_ebd(H) + self.d_ebd(D))[:, None]
        return 55.0 + 20.0 * y
