"""numpy restatements of the averaged weights (`msgat_adam_step_averaged`, csrc/tail.hip; `Trainer(ema_decay=...)`):

    t   = the tensor's step count, already advanced (1 at its first update)
    d   = min(decay, (1 + t) / (10 + t))
    omd = 1 - d
    e   = e + omd * (w_new - e)

`average_f32` takes every operation in float32, each rounded on its own: it must give the BITS of the kernel and of the
torch restatement.  `average_f64` takes the same lines in float64 from the float32 inputs: what the float32 one is
measured against."""
import numpy as np

F = np.float32


def rate_f32(decay, t):
    """1 - d in float32: (1 + t), (10 + t), their quotient, the minimum with (float)decay, 1 - d."""
    t = F(t)
    d = np.minimum(F(decay), (F(1.0) + t) / (F(10.0) + t))
    return F(1.0) - d


def average_f32(e, w_new, decay, t):
    """One update of the shadow `e` (float32 array) towards `w_new` at step count `t`: a new float32 array."""
    e, w_new = np.asarray(e, dtype=F), np.asarray(w_new, dtype=F)
    diff = w_new - e
    step = rate_f32(decay, t) * diff
    out = e + step
    assert out.dtype == F and diff.dtype == F and step.dtype == F
    return out


def average_f64(e, w_new, decay, t):
    e, w_new = np.asarray(e, dtype=np.float64), np.asarray(w_new, dtype=np.float64)
    d = min(float(decay), (1.0 + float(t)) / (10.0 + float(t)))
    return e + (1.0 - d) * (w_new - e)


def run(average, start, observed, decay, first_t=1):
    """The shadow after following `observed` (the parameter after each of its updates), starting at `start`."""
    e = start
    for k, w in enumerate(observed):
        e = average(e, w, decay, first_t + k)
    return e


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
