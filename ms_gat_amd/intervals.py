"""Calibrated prediction intervals for online forecasts: rolling split-conformal half-widths from the errors the scorer
settles (`OnlineForecaster(score=True, intervals=...)`).

Per series (sensor n, horizon h) the last W valid absolute errors |p - y| are kept in a ring on the device, and the
half-width of level c is one order statistic of that ring: the `ceil((m + 1) c)`-th smallest of its m values.  Under
exchangeable errors an interval p +- r made that way covers the next reading with probability at least c (the
finite-sample argument of split-conformal prediction); the rolling window follows drift and each sensor's own noise.

Here are the rank policy (`interval_ranks`, the one place it lives), the bindings of the two kernels of
csrc/online_interval.hip (`interval_update`, `interval_apply`) and their torch restatements, which serve CPU tensors and
state what the kernels must give, bit for bit.  The state tensors are described in include/msgat_hip.h; every one of them is
created with `torch.zeros` or `torch.full` (`interval_state`): nothing here needs uninitialised memory.
"""
from __future__ import annotations

from fractions import Fraction
from typing import Optional

import torch

from . import _lib
from ._lib import stream_handle as _stream_handle

MAX_LEVELS = 4
MAX_WINDOW = 1024
STATE_KEYS = ("interval_window", "interval_cursor", "interval_radius", "interval_book", "interval_counts")


def interval_levels(intervals) -> tuple:
    """The nominal coverage levels as floats, or ValueError: 1 to 4 of them (a single number: one), strictly increasing,
    each inside (0, 1)."""
    if isinstance(intervals, (int, float)) and not isinstance(intervals, bool):
        intervals = (intervals,)
    try:
        levels = tuple(float(c) for c in intervals)
    except (TypeError, ValueError):
        raise ValueError(f"intervals must be a number or a sequence of numbers, not {intervals!r}") from None
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"between 1 and {MAX_LEVELS} interval levels, not {len(levels)}")
    seen = 0.0
    for c in levels:
        if not (c > seen and c < 1.0):             # NaN fails both
            raise ValueError(f"interval levels must be strictly increasing inside (0, 1), not {levels!r}")
        seen = c
    return levels


def interval_ranks(levels, window: int, min_count: Optional[int] = None) -> torch.Tensor:
    """int32 [L, W + 1]: `rank[l, m]` is the 1-based order statistic that serves as the half-width of level l when a
    series holds m errors -- `ceil((m + 1) c_l)` if that is at most m and m >= `min_count`, else 0 = no interval yet
    (the radius is +inf).  Exact rational arithmetic on `Fraction(c).limit_denominator(10**6)`: in floating point
    110 * 0.9 is 99.00000000000001, whose ceiling is 100."""
    levels, W = interval_levels(levels), int(window)
    if not 1 <= W <= MAX_WINDOW:
        raise ValueError(f"interval_window = {window} must be between 1 and {MAX_WINDOW}")
    floor = 1 if min_count is None else int(min_count)
    if not 1 <= floor <= W:
        raise ValueError(f"interval_min_count = {min_count} must be between 1 and the window {W}")
    table = torch.zeros((len(levels), W + 1), dtype=torch.int32)
    for l, c in enumerate(levels):
        level = Fraction(c).limit_denominator(10 ** 6)
        for m in range(floor, W + 1):
            rank = -((-(m + 1) * level.numerator) // level.denominator)      # the ceiling, in integers
            if rank <= m:
                table[l, m] = rank
    return table


def interval_state(n_levels: int, n_nodes: int, t_out: int, window: int, rows: int, device) -> tuple:
    """A fresh (window, cursor, radius, radius_book, counts): empty rings, +inf radii, zero counts."""
    inf = float("inf")
    return (torch.zeros((n_nodes, t_out, window), dtype=torch.float32, device=device),
            torch.zeros((n_nodes, t_out), dtype=torch.int32, device=device),
            torch.full((n_levels, n_nodes, t_out), inf, dtype=torch.float32, device=device),
            torch.full((rows, n_levels, n_nodes, t_out), inf, dtype=torch.float32, device=device),
            torch.zeros((n_levels, n_nodes, t_out, 2), dtype=torch.int64, device=device))


def _ptr(t: torch.Tensor):
    return t.data_ptr()


def _check(what: str, book: torch.Tensor, named) -> None:
    """`named` = [(name, tensor, dtype, shape or None)]: dtypes, shapes, one device (the GPU of `book`), contiguous."""
    if not book.is_cuda:
        raise _lib.MsgatError(f"{what}: book is on {book.device}: the kernels run on the GPU only (a CPU model takes the "
                              "torch restatements)")
    for name, t, dtype, shape in named:
        if t.dtype != dtype:
            raise TypeError(f"{what}: {name} must be {dtype}, got {t.dtype}")
        if t.device != book.device:
            raise ValueError(f"{what}: book on {book.device} and {name} on {t.device} must share one device")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name} {tuple(t.shape)} must be {list(shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")


def _head(what: str, P: int, N: int, out: int, radius: torch.Tensor, point: int) -> tuple:
    """The head's sizes (P, N, out, L, T_out) from the book's and `radius` [L, N, T_out], checked against each other."""
    if min(P, N, out) < 1:
        raise ValueError(f"{what}: a book of {P} rows, {N} nodes and {out} outputs per node is empty")
    if radius.dim() != 3 or radius.numel() == 0:
        raise ValueError(f"{what}: radius {tuple(radius.shape)} must be a non-empty [L, N, T_out]")
    L, _, T = radius.shape
    if not 1 <= L <= MAX_LEVELS:
        raise ValueError(f"{what}: between 1 and {MAX_LEVELS} levels, not {L}")
    if out % T or not 0 <= int(point) < out // T or out > 64:
        raise ValueError(f"{what}: a book of out = {out} <= 64 outputs per node does not hold level {point} of a head with "
                         f"T_out = {T} horizons")
    if P < T:
        raise ValueError(f"{what}: the book's P = {P} rows must be at least T_out = {T}")
    return P, N, out, L, T


def interval_update(raw: torch.Tensor, book: torch.Tensor, issued: torch.Tensor, clock: torch.Tensor,
                    radius_book: torch.Tensor, ranks: torch.Tensor, window: torch.Tensor, cursor: torch.Tensor,
                    radius: torch.Tensor, counts: torch.Tensor, point: int = 0,
                    null_value: Optional[float] = None) -> None:
    """The readings `raw` [K,C,N] (float32, RAW, of the steps `clock[0] + k`) settle the forecasts in `book` [P,N,out]
    that they make due, for the intervals: call it where `ops.forecast_score` is called, BEFORE the `ring_push` of the same
    readings.  Per series (n, h) and k in order, the error a = |p_point - y| of the forecast of origin `clock[0] + k - h`
    (if `issued` carries its stamp and y = raw[k, 0, n] is valid) is first judged against the radii issued with that
    forecast (`radius_book` [P,L,N,T_out]; `counts` [L,N,T_out,2] += {judged, covered} where the radius is finite), then
    inserted into the ring `window` [N,T_out,W] at `cursor` [N,T_out]; at the end `radius` [L,N,T_out] is the
    `ranks[l, fill]`-th smallest of each ring, +inf for rank 0 (`msgat_interval_update`: one launch, a wave per series,
    nothing read back).  `ranks`: `interval_ranks(...)` on the device.  Writes window, cursor, radius and counts in place.
    No autograd: data."""
    what = "interval_update"
    if raw.dim() != 3 or raw.shape[0] < 1:
        raise ValueError(f"{what}: raw {tuple(raw.shape)} must be [K >= 1, C, N]")
    if book.dim() != 3:
        raise ValueError(f"{what}: book {tuple(book.shape)} must be [P, N, out]")
    P, N, out, L, T = _head(what, *book.shape, radius, point)
    if window.dim() != 3 or not 1 <= window.shape[2] <= MAX_WINDOW:
        raise ValueError(f"{what}: window {tuple(window.shape)} must be [N, T_out, W] with 1 <= W <= {MAX_WINDOW}")
    W = window.shape[2]
    _check(what, book, [("book", book, torch.float32, None), ("raw", raw, torch.float32, (raw.shape[0], raw.shape[1], N)),
                        ("issued", issued, torch.int64, (P,)), ("clock", clock, torch.int64, (2,)),
                        ("radius_book", radius_book, torch.float32, (P, L, N, T)),
                        ("ranks", ranks, torch.int32, (L, W + 1)), ("window", window, torch.float32, (N, T, W)),
                        ("cursor", cursor, torch.int32, (N, T)), ("radius", radius, torch.float32, (L, N, T)),
                        ("counts", counts, torch.int64, (L, N, T, 2))])
    dev = book.device
    with torch.cuda.device(dev):
        _lib.checked().msgat_interval_update(_ptr(raw), _ptr(book), _ptr(issued), _ptr(clock), _ptr(radius_book),
                                             _ptr(ranks), _ptr(window), _ptr(cursor), _ptr(radius), _ptr(counts),
                                             raw.shape[0], raw.shape[1], N, T, out, int(point), P, L, W,
                                             int(null_value is not None),
                                             0.0 if null_value is None else float(null_value), _stream_handle(dev))


def interval_apply(pred: torch.Tensor, radius: torch.Tensor, clock: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor,
                   radius_book: torch.Tensor, point: int = 0) -> None:
    """The intervals of the forecast `pred` [N,out] of origin `clock[0]`: `lo` = p - r and `hi` = p + r, both [L,N,T_out]
    with p = pred[n, point * T_out + h] and r = `radius` [L,N,T_out], and r goes into row `clock[0] mod P` of `radius_book`
    [P,L,N,T_out] -- call it beside `ops.forecast_store`, which stamps that row (`msgat_interval_apply`: one launch,
    nothing read back; twice for one origin changes nothing).  Writes lo, hi and radius_book in place.  No autograd: data."""
    what = "interval_apply"
    if pred.dim() != 2 or radius_book.dim() != 4:
        raise ValueError(f"{what}: pred {tuple(pred.shape)} must be [N, out] and radius_book {tuple(radius_book.shape)} "
                         f"[P, L, N, T_out]")
    P, N, out, L, T = _head(what, radius_book.shape[0], *pred.shape, radius, point)
    _check(what, pred, [("pred", pred, torch.float32, None), ("radius", radius, torch.float32, (L, N, T)),
                        ("clock", clock, torch.int64, (2,)), ("lo", lo, torch.float32, (L, N, T)),
                        ("hi", hi, torch.float32, (L, N, T)), ("radius_book", radius_book, torch.float32, (P, L, N, T))])
    dev = pred.device
    with torch.cuda.device(dev):
        _lib.checked().msgat_interval_apply(_ptr(pred), _ptr(radius), _ptr(clock), _ptr(lo), _ptr(hi), _ptr(radius_book),
                                            N, T, out, int(point), P, L, _stream_handle(dev))


# ---- the torch restatements: CPU tensors, and what the kernels must give ------------------------------------------------
def _interval_update_torch(raw: torch.Tensor, book: torch.Tensor, issued: torch.Tensor, clock: torch.Tensor,
                           radius_book: torch.Tensor, ranks: torch.Tensor, window: torch.Tensor, cursor: torch.Tensor,
                           radius: torch.Tensor, counts: torch.Tensor, point: int = 0,
                           null_value: Optional[float] = None) -> None:
    """`interval_update` restated with torch ops on host tensors, all nodes of a horizon at once: judged, then inserted,
    the cursor's wrap, and the selection as a sort of each ring with the slots at or beyond its fill put to +inf (the
    element a sort picks is the one the kernel's radix select picks: equal values have equal bits)."""
    P, N, out = book.shape
    L, _, T = radius.shape
    W = window.shape[2]
    start, stamps = int(clock[0]), issued.tolist()
    nodes = torch.arange(N, device=raw.device)
    inf = torch.full((), float("inf"), dtype=torch.float32, device=raw.device)
    for k in range(raw.shape[0]):
        y = raw[k, 0]
        valid = ~torch.isnan(y)
        if null_value is not None:
            valid = valid & (y != null_value)
        for h in range(T):
            origin = start + k - h
            row = origin % P
            if origin < 0 or stamps[row] != origin:
                continue
            a = (book[row, :, point * T + h] - y).abs()
            r = radius_book[row, :, :, h]                                                                 # [L, N]
            judged = valid[None] & torch.isfinite(r)
            counts[:, :, h, 0] += judged
            counts[:, :, h, 1] += judged & (a[None] <= r)
            put = valid & torch.isfinite(a)
            c = cursor[:, h].to(torch.int64) & 0xFFFFFFFF                                                 # as uint32
            slot = c % W
            window[nodes[put], h, slot[put]] = a[put]
            after = torch.where(c < W, c + 1, W + (slot + 1) % W)
            moved = torch.where(put, after, c)
            cursor[:, h] = torch.where(moved >= 2 ** 31, moved - 2 ** 32, moved).to(torch.int32)
    fill = (cursor.to(torch.int64) & 0xFFFFFFFF).clamp(max=W)                                             # [N, T]
    held = torch.where(torch.arange(W, device=raw.device) < fill[..., None], window, inf)
    ordered = held.sort(dim=-1).values
    for l in range(L):
        rank = ranks[l].to(torch.int64)[fill]                                                             # [N, T]
        has = (rank >= 1) & (rank <= fill)
        picked = ordered.gather(-1, (rank - 1).clamp(0, W - 1)[..., None])[..., 0]
        radius[l] = torch.where(has, picked, inf)


def _interval_apply_torch(pred: torch.Tensor, radius: torch.Tensor, clock: torch.Tensor, lo: torch.Tensor,
                          hi: torch.Tensor, radius_book: torch.Tensor, point: int = 0) -> None:
    """`interval_apply` restated with torch indexing."""
    L, N, T = radius.shape
    p = pred[:, point * T: (point + 1) * T]
    lo.copy_(p[None] - radius)
    hi.copy_(p[None] + radius)
    radius_book[clock[0] % radius_book.shape[0]] = radius                     # `%` of tensors is the floor-mod
