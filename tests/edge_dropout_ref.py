"""A numpy restatement of the edge-dropout draw (include/msgat_hip.h, msgat_edge_dropout) and of its forward and both
backward forms, for the tests: Philox4x32-10 with the Random123 constants through uint64 products, the masks of a
[V,nnz] draw, and float32 loops.  Nothing here touches the library.
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key increments
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) broadcast together, key: two -> four uint32 arrays, the generator's words."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]        # < 2^64: the whole product
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def constants(p):
    """(thr, scale): thr = floor(p * 2^32) as an integer, scale = 1 / (1 - p) in double rounded once to float32."""
    return int(math.floor(float(p) * 4294967296.0)), np.float32(1.0 / (1.0 - float(p)))


def words(seed, step, V, nnz, sample_offset=0):
    """[V,nnz] uint32: the word edge e of global sample sample_offset + v reads at `step` under `seed`."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    quads = (nnz + 3) // 4
    q = np.arange(quads, dtype=np.uint64)[None, :]
    s = (np.arange(V, dtype=np.uint64) + np.uint64(sample_offset))[:, None]
    r = philox4x32_10((q, s, step & MASK32, step >> 32), (seed & MASK32, seed >> 32))     # four [V,quads]
    return np.stack(r, axis=-1).reshape(V, 4 * quads)[:, :nnz]


def dropped(seed, step, V, nnz, p, sample_offset=0, exempt=None):
    """[V,nnz] bool: the edges the draw drops (an exempt edge never is)."""
    thr, _ = constants(p)
    d = words(seed, step, V, nnz, sample_offset).astype(np.uint64) < np.uint64(thr)
    if exempt is not None:
        d &= ~np.asarray(exempt, dtype=bool)[None, :]
    return d


def multipliers(seed, step, V, nnz, p, sample_offset=0, exempt=None):
    """[V,nnz] float32: +0 dropped, scale kept, 1 exempt."""
    _, scale = constants(p)
    m = np.where(dropped(seed, step, V, nnz, p, sample_offset, exempt), np.float32(0), scale).astype(np.float32)
    if exempt is not None:
        m[:, np.asarray(exempt, dtype=bool)] = np.float32(1)
    return m


def forward(w, seed, step, V, p, sample_offset=0, exempt=None):
    """out [V,nnz] float32, entry by entry: exempt -> w, dropped -> +0, else w * scale (one float32 multiply)."""
    w = np.asarray(w, dtype=np.float32)
    nnz = w.shape[-1]
    _, scale = constants(p)
    drop = dropped(seed, step, V, nnz, p, sample_offset, exempt)
    ex = np.zeros(nnz, bool) if exempt is None else np.asarray(exempt, dtype=bool)
    out = np.empty((V, nnz), np.float32)
    for v in range(V):                   # a float32 row at a time: numpy rounds every product once, to float32
        row = w if w.ndim == 1 else w[v]
        kept = (row * scale).astype(np.float32)
        out[v] = np.where(ex, row, np.where(drop[v], np.float32(0), kept))
    return out


def backward_sets(dout, m):
    """dw [V,nnz] = dout * m, one float32 multiply per entry."""
    dout = np.asarray(dout, dtype=np.float32)
    dw = np.empty_like(dout)
    for v in range(dout.shape[0]):
        dw[v] = dout[v] * m[v]
    return dw


def backward_shared(dout, m):
    """dw [nnz] = sum_v dout[v] * m[v]: float32, rounded products added from +0 in ascending sample order."""
    dout = np.asarray(dout, dtype=np.float32)
    dw = np.zeros(dout.shape[1], np.float32)
    for v in range(dout.shape[0]):
        dw = dw + (dout[v] * m[v]).astype(np.float32)
    return dw
