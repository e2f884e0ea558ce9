"""numpy float32 restatement of a gradient-accumulation window (`msgat_gather_scaled{,_dev}` for the first micro-batch,
`msgat_gather_accumulate{,_dev}` for the later ones, csrc/tail.hip; `FlatAdam.accumulate` / `Trainer(accumulate_steps=k)`).

Every operation is one float32 numpy ufunc, so it is rounded on its own: the product `w * g` first, then the sum with what
the buffer holds, then the weight sum -- no fused multiply-add anywhere, which is what the kernels promise."""
import numpy as np


def f32(x):
    return np.asarray(x, dtype=np.float32)


def gather(flat, grads, offsets, weight, weight_index):
    """The first micro-batch of a window: flat[o : o + n] = w * g for every (gradient, offset), flat[weight_index] = w.
    In place on the float32 array `flat`; elements no gradient covers keep their bits."""
    w = np.float32(weight)
    for g, o in zip(grads, offsets):
        g = f32(g).reshape(-1)
        flat[o:o + g.size] = w * g
    if weight_index >= 0:
        flat[weight_index] = w
    return flat


def accumulate(flat, grads, offsets, weight, weight_index):
    """A later micro-batch: flat[o : o + n] = flat[o : o + n] + (w * g), the product rounded to float32 before the sum is
    formed and rounded; flat[weight_index] = flat[weight_index] + w.  In place."""
    w = np.float32(weight)
    for g, o in zip(grads, offsets):
        g = f32(g).reshape(-1)
        term = w * g                                   # rounded
        flat[o:o + g.size] = flat[o:o + g.size] + term   # rounded again
    if weight_index >= 0:
        flat[weight_index] = flat[weight_index] + w
    return flat


def window(flat, micro_batches, offsets, weight_index):
    """`micro_batches`: [(weight, [gradient per offset]), ...] in call order.  Returns `flat` (modified in place): sum(w g)
    in the covered elements and sum(w), in call order, at `weight_index`."""
    for k, (w, grads) in enumerate(micro_batches):
        (gather if k == 0 else accumulate)(flat, grads, offsets, w, weight_index)
    return flat


def window_mean(micro_batches):
    """sum(w g) / max(sum w, 1) per gradient, in the float32 arithmetic above: what the update consumes."""
    sizes = [np.asarray(g).size for g in micro_batches[0][1]]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = np.zeros(int(offsets[-1]) + 1, dtype=np.float32)
    window(flat, micro_batches, offsets[:-1], int(offsets[-1]))
    div = np.maximum(flat[-1], np.float32(1.0))
    return [(flat[o:o + n] / div).reshape(np.asarray(g).shape) for o, n, g in zip(offsets[:-1], sizes, micro_batches[0][1])]
