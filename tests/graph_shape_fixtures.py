"""Hand-built adjacencies for the core graph attention: skewed, directed and hollow graphs.

`synthetic_adjacency` (uniform random undirected edges + identity, sym-normalised) gives symmetric patterns without an
empty row or column and with a maximum degree within ~3x of the mean.  The graphs here are what a learned dense
adjacency, a thresholded distance matrix or per-sample sparse weights look like instead: directed, with hubs, with
sensors that have no in-edges or no out-edges -- and a few that sit exactly on the thresholds at which the library
changes kernels (`pair_trips` 12 / 13: k_sddmm_sellreg / k_sddmm_sell; 1024 / 1025 edges in a row block: the cached /
uncached tail of the score kernels).

Pure numpy; nothing of the library (or torch) is imported at module import.  Every fixture is fully determined by its
name and a seed.  Stored values are uniform(0.25, 1.5) -- structure is the subject, values are not normalised -- and the
`*_signed` variants multiply them by a random +-1.  A fixture derived from another (`trips13` from `trips12`, `pair13`
from `pair12`, `onerow1025` from `onerow1024`, `lonely65_d5` from `lonely65_d0`) is its base, value for value, plus the
entries of ONE row; `*_T` is the transpose.

tests/test_graph_shapes_cpu.py asserts the structural claims below against the library's own graph builder;
tests/test_gpu_graph_shapes.py runs the kernels on them.
"""
import zlib

import numpy as np

# rows (or columns) per SELL slice and columns per trip (include/msgat_hip.h, msgat_sell_t)
SLICE = 64
TRIP = 4

# the execution modes of ops.gacn at the widths the GPU tests use: name -> (C, Co)
MODES = {"PLAIN": (3, 0), "AGG_FIRST": (3, 24), "PROJ_FIRST": (40, 8)}
# Up to 4 channels under the attention the backward forms the edge gradient inside its row pass (k_bwd_rows<T, DC>, api.hip:
# direct_c) and launches no SDDMM at all -- so at C = 3 only PROJ_FIRST (Co = 8 channels) reaches one.  These widths put
# PLAIN and AGG_FIRST behind the SDDMM on C channels too.
WIDE = {"PLAIN": (6, 0), "AGG_FIRST": (6, 24)}
# the fixtures that run at the WIDE widths as well: both sides of the SDDMM's register form, zero-width slices, a hub
WIDE_NAMES = ("trips12", "trips13", "pair12", "pair13", "hub130", "hollow200")

HUB_ROW, HUB_COL = 17, 90
HUB_EMPTY_ROWS = tuple(range(40, 47))
HUB_ZERO_COLS = (5, 63, 64, 129)
LONELY_ROW = 33
EDGE70 = (3, 41)            # the one stored entry of `edge70`: row, column
CROSS_ROW, CROSS_COL = 9, 30
LARGE_N, LARGE_ROW, LARGE_COL = 2545, 7, 11    # 2545 * 16 * 4 B > 160 KiB - 1 KiB: the first N without a slab at T = 16


def _rng(name, seed, salt=0):
    return np.random.default_rng([int(seed), zlib.crc32(name.encode()), salt])


def _ladder(n, rng, clip):
    """row i stores min(i, clip) columns drawn without replacement"""
    mask = np.zeros((n, n), dtype=bool)
    for i in range(n):
        mask[i, rng.choice(n, size=min(i, clip), replace=False)] = True
    return mask


def _pair(rng):
    """128 rows: 64 of degree 22..28 and 64 of degree 1..20, exactly one of them 20 (the row `touched_row` names)"""
    n = 128
    deg = np.empty(n, dtype=np.int64)
    deg[:64] = 22 + np.arange(64) % 7
    deg[:64][11] = 28
    deg[64:] = 1 + np.arange(64) % 19
    deg[64 + LONELY_ROW] = 20
    order = rng.permutation(n)                  # which node gets which degree: the slices are not index ranges
    mask = np.zeros((n, n), dtype=bool)
    for node, d in zip(order, deg):
        mask[node, rng.choice(n, size=int(d), replace=False)] = True
    return mask, int(order[64 + LONELY_ROW])


def _hub(rng):
    n = 130
    mask = np.zeros((n, n), dtype=bool)
    i = np.arange(n - 1)
    mask[i, i + 1] = True                       # a directed chain i -> i + 1
    loops = np.arange(0, n, 3)
    mask[loops, loops] = True                   # self loops on some nodes only
    mask[HUB_ROW, :] = True                     # one row stored in every column
    mask[:, HUB_COL] = True                     # one column stored by every row
    mask[list(HUB_EMPTY_ROWS), :] = False
    mask[:, list(HUB_ZERO_COLS)] = False        # ... taken out of the hub row too
    return mask


def _hollow(rng, n):
    """rows 0..39 with degrees 1..40; the 820 entries walk a permutation of the columns, so every column is stored"""
    perm = rng.permutation(n)
    mask = np.zeros((n, n), dtype=bool)
    e = 0
    for i in range(40):
        mask[i, perm[(e + np.arange(i + 1)) % n]] = True
        e += i + 1
    return mask


def _lonely(rng):
    """65 rows: 64 of degree 6..20, and LONELY_ROW without an entry (it is the second slice, alone)"""
    n = 65
    mask = np.zeros((n, n), dtype=bool)
    for i in range(n):
        if i != LONELY_ROW:
            mask[i, rng.choice(n, size=6 + i % 15, replace=False)] = True
    return mask


def _onerow(rng):
    n = 1040
    mask = np.zeros((n, n), dtype=bool)
    mask[0, np.sort(rng.permutation(n)[:1024])] = True
    return mask


def _extra(mask, row, count, rng):
    """`count` more entries in `row`, at columns it does not store yet"""
    free = np.flatnonzero(~mask[row])
    out = mask.copy()
    out[row, rng.choice(free, size=count, replace=False)] = True
    return out


def _edge70(rng):
    mask = np.zeros((70, 70), dtype=bool)
    mask[EDGE70] = True
    return mask


def _cross(n):
    def build(rng):
        mask = np.zeros((n, n), dtype=bool)
        mask[CROSS_ROW, :] = True
        mask[:, CROSS_COL] = True
        return mask
    return build


def _large(few):
    """N = LARGE_N, where no [N,16] slab fits the LDS but one 4-timestep column does: a row and a column of more than 8
    entries, a chain through the first 200 nodes, and nothing in the other rows; `few`: five stored entries in all"""
    def build(rng):
        n = LARGE_N
        mask = np.zeros((n, n), dtype=bool)
        if few:
            mask[[3, 3, 100, n - 1, n - 1], [41, 2000, 3, 0, n - 1]] = True
            return mask
        i = np.arange(200)
        mask[i, i + 1] = True
        mask[LARGE_ROW, rng.choice(n, size=20, replace=False)] = True
        mask[rng.choice(n, size=15, replace=False), LARGE_COL] = True
        return mask
    return build


def _values(mask, rng):
    return np.where(mask, rng.uniform(0.25, 1.5, size=mask.shape), 0.0).astype(np.float32)


def _base(name, seed):
    """(mask, values) of a fixture that is not derived from another"""
    rng = _rng(name, seed)
    if name == "ladder64":
        mask = _ladder(64, rng, 63)
    elif name == "trips12":
        mask = _ladder(64, rng, 48)
    elif name == "pair12":
        mask, _ = _pair(rng)
    elif name == "hub130":
        mask = _hub(rng)
    elif name in ("hollow130", "hollow200"):
        mask = _hollow(rng, int(name[6:]))
    elif name == "lonely65_d0":
        mask = _lonely(rng)
    elif name == "onerow1024":
        mask = _onerow(rng)
    elif name == "edge70":
        mask = _edge70(rng)
    elif name in ("cross64", "cross65"):
        mask = _cross(int(name[5:]))(rng)
    elif name in ("wide2545", "few2545"):
        mask = _large(name == "few2545")(rng)
    else:
        raise KeyError(name)
    return mask, _values(mask, _rng(name, seed, 1))


# derived fixture -> (its base, the row that gets more entries, how many); the row of `pair13` comes from the base's rng
_DERIVED = {"trips13": ("trips12", 63, 1), "pair13": ("pair12", None, 1), "onerow1025": ("onerow1024", 0, 1),
            "lonely65_d5": ("lonely65_d0", LONELY_ROW, 5)}


def touched_row(name, seed=0):
    """The one row in which a derived fixture differs from its base."""
    base, row, _ = _DERIVED[name]
    if row is None:
        row = _pair(_rng(base, seed))[1]
    return row


def adjacency(name, seed=0):
    """The dense fp32 [N,N] adjacency of fixture `name`."""
    if name.endswith("_T"):
        return np.ascontiguousarray(adjacency(name[:-2], seed).T)
    if name.endswith("_signed"):
        a = adjacency(name[:-7], seed)
        return a * _rng(name, seed, 2).choice(np.float32([-1.0, 1.0]), size=a.shape)
    if name in _DERIVED:
        base, _, count = _DERIVED[name]
        a = adjacency(base, seed)
        row = touched_row(name, seed)
        mask = _extra(a != 0, row, count, _rng(name, seed))
        new = mask & (a == 0)
        a[new] = _values(new, _rng(name, seed, 1))[new]
        return a
    return _base(name, seed)[1]


# fixtures of the whole-layer tests (both layouts, three modes); the `onerow*` ones have their own (the tail threshold)
LAYER = ("ladder64", "ladder64_signed", "trips12", "trips13", "pair12", "pair13", "hub130", "hub130_signed", "hollow130",
         "hollow200", "hollow200_T", "lonely65_d0", "lonely65_d5")
ONEROW = ("onerow1024", "onerow1025", "onerow1024_T", "onerow1025_T")
SMALL = ("edge70", "cross64", "cross65")
NAMES = LAYER + ONEROW + SMALL
# beyond the LDS slab (their own GPU tests; what they are is asserted there, on the host, before the kernels run)
LARGE = ("wide2545", "few2545")

# What each fixture is built to be.  n, the largest row / column degree, the number of rows / columns without an entry,
# and per side of the SELL layout (rows form, columns form) `pair_trips` and the number of slices of width 0; None where
# the figure follows from random draws and is not the point (the host test then holds the library to `sell_trips`).
_C = ("n", "max_row", "max_col", "empty_rows", "empty_cols", "pair_rows", "pair_cols", "zero_rows", "zero_cols")
CLAIMS = {k: dict(zip(_C, v)) for k, v in {
    "ladder64":        (64, 63, None, 1, 0, 16, None, 0, 0),
    "ladder64_signed": (64, 63, None, 1, 0, 16, None, 0, 0),
    "trips12":         (64, 48, None, 1, 0, 12, None, 0, 0),
    "trips13":         (64, 49, None, 1, 0, 13, None, 0, 0),
    "pair12":          (128, 28, None, 0, 0, 12, None, 0, 0),
    "pair13":          (128, 28, None, 0, 0, 13, None, 0, 0),
    "hub130":          (130, 126, 123, 7, 4, 32, 31, 1, 1),
    "hub130_signed":   (130, 126, 123, 7, 4, 32, 31, 1, 1),
    "hollow130":       (130, 40, None, 90, 0, 10, None, 2, 0),       # an odd slice count in k_sddmm_sellreg: 10 | 0 | 0 trips
    "hollow200":       (200, 40, None, 160, 0, 10, None, 3, 0),
    "hollow200_T":     (200, None, 40, 0, 160, None, 10, 0, 3),
    "lonely65_d0":     (65, 20, None, 1, 0, 5, None, 1, 0),
    "lonely65_d5":     (65, 20, None, 0, 0, 7, None, 0, 0),
    "onerow1024":      (1040, 1024, 1, 1039, 16, 256, 2, 16, 1),
    "onerow1025":      (1040, 1025, 1, 1039, 15, 257, 2, 16, 0),
    "onerow1024_T":    (1040, 1, 1024, 16, 1039, 2, 256, 1, 16),
    "onerow1025_T":    (1040, 1, 1025, 15, 1039, 2, 257, 0, 16),
    "edge70":          (70, 1, 1, 69, 69, 1, 1, 1, 1),
    "cross64":         (64, 64, 64, 0, 0, 16, 16, 0, 0),
    "cross65":         (65, 65, 65, 0, 0, 18, 18, 0, 0),
}.items()}


def degrees(name, seed=0):
    """(entries per row [N], entries per column [N]) of fixture `name`"""
    mask = adjacency(name, seed) != 0
    return mask.sum(1), mask.sum(0)


def sell_trips(deg):
    """(trips per slice, pair_trips) of the degree-sorted sliced layout of rows with degrees `deg`, restated from its
    definition (include/msgat_hip.h): rows by degree, descending; slice s = 64 of them; its width is its first row's
    degree rounded up to a whole trip of 4; k_sddmm_sellreg gives a wave slice i from the wide end and slice
    n_slices - 1 - i from the narrow end, and pair_trips is the most trips any such pair has."""
    d = np.sort(np.asarray(deg))[::-1]
    trips = [int(-(-int(d[s]) // TRIP)) for s in range(0, len(d), SLICE)]
    ns = len(trips)
    pair = max(trips[i] + (trips[ns - 1 - i] if ns - 1 - i > i else 0) for i in range((ns + 1) // 2))
    return trips, pair


def problem(name, C, Co, T=12, Bg=2, R=2, seed=0):
    """x [R Bg,C,N,T], adj [N,N], Wg [R,T,T], alpha [R,C], W [R,Co,C] (None for Co = 0), dz: the distributions of
    `random_problem` in test_gpu_parity.py on fixture `name`.  `seed` draws the signals and parameters only (the
    adjacency is the fixture's, at its default seed), so two fixtures of one size share everything but the graph."""
    adj = adjacency(name)
    N = adj.shape[0]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R * Bg, C, N, T)).astype(np.float32)
    Wg = (rng.standard_normal((R, T, T)) * (1.0 / T) ** 0.5).astype(np.float32)
    alpha = rng.uniform(-C ** -0.5, C ** -0.5, size=(R, C)).astype(np.float32)
    W = None if Co == 0 else (rng.standard_normal((R, Co, C)) * (2.0 / (Co + C)) ** 0.5).astype(np.float32)
    dz = rng.standard_normal((R * Bg, Co if Co else C, N, T)).astype(np.float32)
    return x, adj, Wg, alpha, W, dz


def stored_entry_grad_f64(x, adj, Wg, alpha, W, dz):
    """(rows, cols, the gradient at the stored entries of `adj` in row-major order) in float64: autograd of the dense op
    sequence (oracle/dense_torch.py) with the adjacency as a leaf, summed over the R stacked relations, read where
    adj != 0 -- what a sparse adjacency whose values require grad must receive at its values."""
    import torch
    from oracle import dense_torch
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    a = f(adj).requires_grad_(True)
    R = Wg.shape[0]
    Bg = x.shape[0] // R
    for r in range(R):
        sl = slice(r * Bg, (r + 1) * Bg)
        z = dense_torch.graph_attention_dense(f(x[sl]), a, f(Wg[r]), f(alpha[r])) if W is None else \
            dense_torch.gacn_dense(f(x[sl]), a, f(Wg[r]), f(alpha[r]), f(W[r]))
        z.backward(f(dz[sl]))
    rows, cols = np.nonzero(adj)
    return rows, cols, a.grad.numpy()[rows, cols]
