"""Validity-gated edges restated in numpy, fp32: what msgat_edge_validity{,_backward} must produce bit for bit.

    count[v,n] = #{t : val[v,n,t] > 0.5}          (a NaN compares false and is not counted)
    g[v,n]     = table[count[v,n]]                (table: T + 1 floats, computed in double, rounded once)
    out[v,e]   = exempt[e] ? w : (g[v,col(e)] == 0 ? +0 : w * g[v,col(e)])        one fp32 multiply
    dw[v,e]    = the same expression on dout;  dw[e] = the terms added from +0 in ascending v

and the seeded inputs of the tests: patterns built by hand and validity windows of exact 0.0 / 1.0 with some NaN, 0.49 and
0.51 entries.
"""
import numpy as np

T_SET = (4, 8, 12, 16)


def table(mode, T):
    c = np.arange(T + 1, dtype=np.float64)
    if mode == "scale":
        t = c / T
    elif mode == "drop":
        t = (c == T).astype(np.float64)
    elif isinstance(mode, int) and not isinstance(mode, bool) and 1 <= mode <= T:
        t = (c >= mode).astype(np.float64)
    else:
        raise ValueError(mode)
    return t.astype(np.float32)


def modes(T):
    """every kind of mode at this T: both names, the two extreme thresholds and one inside"""
    return ["scale", "drop", 1, T // 2 + 1, T]


def counts(val):
    with np.errstate(invalid="ignore"):
        return (np.asarray(val, np.float32) > np.float32(0.5)).sum(-1)


def gates(val, col, mode):
    """[V,nnz] fp32: the gate of each edge's source node"""
    T = val.shape[-1]
    return table(mode, T)[counts(val)][:, np.asarray(col)]


def terms(x, g, exempt=None):
    """x [nnz] or [V,nnz] -> [V,nnz]: exempt ? x : (g == 0 ? +0 : x * g)"""
    x = np.broadcast_to(np.asarray(x, np.float32), g.shape)
    with np.errstate(invalid="ignore"):
        out = np.where(g == 0, np.float32(0), (x * g).astype(np.float32))
    if exempt is not None:
        out = np.where(np.asarray(exempt, bool)[None, :], x, out)
    return np.ascontiguousarray(out, np.float32)


def forward(w, val, col, mode, exempt=None):
    return terms(w, gates(val, col, mode), exempt)


def backward_sets(dout, val, col, mode, exempt=None):
    return terms(dout, gates(val, col, mode), exempt)


def backward_shared(dout, val, col, mode, exempt=None):
    t = backward_sets(dout, val, col, mode, exempt)
    acc = np.zeros(t.shape[1], np.float32)
    for v in range(t.shape[0]):                       # from +0, in ascending v, every partial sum rounded to fp32
        acc = (acc + t[v]).astype(np.float32)
    return acc


# ---- the seeded inputs -------------------------------------------------------------------------------------------------

def validity(V, N, T, seed=0):
    """[V,N,T] fp32: mostly exact 1.0, a quarter exact 0.0, a few NaN / 0.49 / 0.51 / exactly 0.5 entries; node 0 of every
    sample is fully valid and node 1 fully missing where they exist, and sample 0 has no missing reading at all when V > 1."""
    rng = np.random.default_rng(1000 + seed)
    val = (rng.random((V, N, T)) >= 0.25).astype(np.float32)
    odd = rng.random((V, N, T))
    val[odd < 0.03] = np.nan
    val[(odd >= 0.03) & (odd < 0.06)] = 0.49
    val[(odd >= 0.06) & (odd < 0.09)] = 0.51
    val[(odd >= 0.09) & (odd < 0.10)] = 0.5
    whole = rng.random((V, N))
    val[whole < 0.15] = 1.0                            # whole windows valid ...
    val[whole > 0.85] = 0.0                            # ... and whole windows missing
    val[:, 0] = 1.0
    if N > 1:
        val[:, 1] = 0.0
    if V > 1:
        val[0] = 1.0
    return val


def pattern(nnz, seed=0):
    """(crow int64 [N+1], col int64 [nnz], N): a CSR pattern with exactly `nnz` stored edges, columns ascending inside a
    row, built by hand: node 3 has the one self-loop, node 2 is a hub whose column is stored by 70 rows (nnz >= 71: column
    degree 70), and the last two nodes have no edge at all, neither in their row nor as anyone's column."""
    rng = np.random.default_rng(2000 + seed)
    n_live = max(4, min(90, nnz)) if nnz >= 4 else 4
    N = n_live + 2                                     # the last two nodes stay without an edge
    rows = [set() for _ in range(N)]
    left = nnz
    if left > 0:
        rows[3].add(3)                                 # the self-loop
        left -= 1
    hub_rows = [r for r in range(n_live) if r != 2][: min(70, left)]
    for r in hub_rows:                                 # the hub: column 2 stored by up to 70 rows
        rows[r].add(2)
    left -= len(hub_rows)
    while left > 0:
        r, c = int(rng.integers(0, n_live)), int(rng.integers(0, n_live))
        if r != c and c != 2 and c not in rows[r]:
            rows[r].add(c)
            left -= 1
    crow = np.zeros(N + 1, np.int64)
    col = []
    for r in range(N):
        col += sorted(rows[r])
        crow[r + 1] = len(col)
    assert len(col) == nnz
    return crow, np.asarray(col, np.int64), N


def self_loops(crow, col):
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    return rows == col
