"""Host side of gradient accumulation: the two new C-ABI entry points and their status codes, the numpy restatement of a
window, and `Trainer(accumulate_steps=k)` on CPU parameters -- the torch restatement of what `FlatAdam` does on the GPU --
against ONE step of the same trainer on the union of the window's micro-batches.  Nothing in the model has batch
statistics, so a window is mathematically that step; what differs is rounding (three sums instead of one), and the
tolerance is the relative 1e-6 `test_guarded_step_cpu.py` holds its figures to.  No device compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_accumulate_ref as ref
from conftest import ROOT, rel_err
from test_guarded_step_cpu import DELTA, _TinyMSGAT

RTOL = 1e-6       # test_guarded_step_cpu.py's pytest.approx(rel=1e-6), per element of every parameter


@pytest.fixture(scope="module")
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


NEW = {"msgat_gather_accumulate": 8, "msgat_gather_accumulate_dev": 8}


def test_accumulate_entry_points_are_declared_exported_and_bound_under_abi_10(built_library):
    from ms_gat_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW.items():
        assert hasattr(h, name), name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.exported_symbols() and len(_lib._PROTOTYPES[name][1]) == n_args, name
        sibling = name.replace("accumulate", "scaled")       # the argument lists of the overwriting gathers
        assert _lib._PROTOTYPES[name] == _lib._PROTOTYPES[sibling], name
    assert "const float* scale" in re.search(r"msgat_gather_accumulate_dev\s*\(([^)]*)\)", code).group(1)
    assert re.search(r"#define\s+MSGAT_ABI_VERSION\s+10\b", code)
    assert _lib.ABI_VERSION == 10 and _lib.lib().msgat_abi_version() == 10
    assert "msgat_gather_accumulate and msgat_gather_accumulate_dev" in header.split("#define MSGAT_ABI_VERSION")[0]


def test_accumulate_entry_points_report_bad_arguments_before_any_launch(built_library):
    from ms_gat_amd import _lib
    L = _lib.lib()
    x = C.cast(C.create_string_buffer(64), C.c_void_p)       # a non-NULL pointer; nothing is launched on these paths
    for n in (0, -1):
        assert L.msgat_gather_accumulate(x, x, x, n, 1.0, x, 0, None) == -2
        assert L.msgat_gather_accumulate_dev(x, x, x, n, x, x, 0, None) == -2
    for hole in (0, 1, 2, 5):
        args = [x, x, x, 1, 1.0, x, 0, None]
        args[hole] = None
        assert L.msgat_gather_accumulate(*args) == -1, hole
    for hole in (0, 1, 2, 4, 5):
        args = [x, x, x, 1, x, x, 0, None]
        args[hole] = None
        assert L.msgat_gather_accumulate_dev(*args) == -1, hole


def test_restatement_rounds_the_product_then_the_sum_then_the_weight():
    rng = np.random.default_rng(5)
    g0, g1, g2 = (rng.standard_normal(4099).astype(np.float32) for _ in range(3))
    w = (3.0, 7.0, 5.0)
    flat = np.full(4099 + 3, 9.0, dtype=np.float32)            # one foreign element on each side, the weight last
    ref.window(flat, [(w[0], [g0]), (w[1], [g1]), (w[2], [g2])], [1], 4101)
    assert flat[0] == 9.0 and flat[4100] == 9.0 and flat[4101] == np.float32(15.0)
    # the same through float64, where a product of two float32 is exact: round it, add, round
    t = [(np.float64(np.float32(wi)) * g.astype(np.float64)).astype(np.float32) for wi, g in zip(w, (g0, g1, g2))]
    two = (t[0].astype(np.float64) + t[1].astype(np.float64)).astype(np.float32)
    want = (two.astype(np.float64) + t[2].astype(np.float64)).astype(np.float32)
    assert np.array_equal(flat[1:4100], want)
    # and a fused multiply-add (one rounding of acc + w g) is NOT the same number everywhere: the distinction is observable
    fused = (t[0].astype(np.float64) + np.float64(7.0) * g1.astype(np.float64)).astype(np.float32)
    assert np.count_nonzero(fused != two) > 0
    mean = ref.window_mean([(w[0], [g0]), (w[1], [g1]), (w[2], [g2])])[0]
    assert np.array_equal(mean, want / np.float32(15.0))


# ---- Trainer on CPU parameters ---------------------------------------------------------------------------------------------
def _batch(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 2, 2, 5, 12, generator=g) * scale
    y = X.reshape(n, 4, 5, 12).mean(1) + 0.5 * torch.randn(n, 5, 12, generator=g) + 2.0
    return [X, torch.zeros(n, dtype=torch.long), torch.zeros(n, dtype=torch.long), y]


def _union(batches):
    return [torch.cat([b[i] for b in batches]) for i in range(4)]


def _trained(tmp_path, name, batches, **kw):
    from ms_gat_amd import engine
    model = _TinyMSGAT()
    tr = engine.Trainer(model, DELTA, str(tmp_path / name), **kw)
    assert isinstance(tr.optimizer, torch.optim.Adam)
    tr.run_epoch(batches, epoch=1, mode="train")
    return model, tr


def _assert_same_step(got, want):
    """Parameters per element, and the gradient the last step consumed (left in p.grad) per tensor on its own scale: Adam's
    first step from fresh moments is lr * sign(g) whatever the size of g, so the parameters alone would not notice a wrongly
    weighted window -- the gradient does."""
    for (name, p), q in zip(got.named_parameters(), want.parameters()):
        worst_g = rel_err(p.grad, q.grad)
        p, q = p.detach(), q.detach()
        assert torch.isfinite(p).all()
        worst = float(((p - q).abs() / q.abs()).max())
        print(f"{name}: worst relative difference {worst:.3e}, of the gradient {worst_g:.3e} (bar {RTOL:g})")
        assert torch.allclose(p, q, rtol=RTOL, atol=0.0), (name, worst)
        assert worst_g < RTOL, (name, worst_g)


@pytest.mark.parametrize("sizes", [(3, 3), (3, 3, 2)])     # an even window; a ragged one with k = 3
def test_a_window_is_one_step_on_the_union_of_its_micro_batches(tmp_path, sizes):
    micro = [_batch(n, 20 + i) for i, n in enumerate(sizes)]
    got, tr = _trained(tmp_path, "window", micro, accumulate_steps=len(sizes))
    want, _ = _trained(tmp_path, "union", [_union(micro)])
    start = _TinyMSGAT()
    assert not any(torch.equal(p.detach(), s.detach()) for p, s in zip(want.parameters(), start.parameters()))
    _assert_same_step(got, want)
    assert tr.last_stats["optimizer_steps"] == 1
    assert all(float(tr.optimizer.state[p]["step"]) == 1.0 for p in got.parameters())
    assert all(p.grad is not None for p in got.parameters()) and tr._cpu_window is None


def test_masked_micro_batches_are_weighted_by_their_valid_counts(tmp_path):
    """null_value = 0: a truth of exactly 0 is a missing reading.  The first micro-batch of each window loses most of its
    entries, the second none, so sum(v g) / sum(v) is far from the plain mean of the two gradients -- which must NOT
    pass.  Two windows: the second step's size depends on the gradients' sizes, so the parameters notice as well."""
    from ms_gat_amd import engine
    micro = [_batch(3, 31 + i) for i in range(4)]
    for i in (0, 2):
        keep = torch.rand(micro[i][3].shape, generator=torch.Generator().manual_seed(7 + i)) < 0.2
        micro[i][3] = torch.where(keep, micro[i][3], torch.zeros(()))
    counts = [int((b[3] != 0).sum()) for b in micro]
    assert counts[1] == counts[3] == 3 * 5 * 12 and 0 < counts[0] < counts[1] // 3 and 0 < counts[2] < counts[1] // 3
    got, tr = _trained(tmp_path, "window", micro, accumulate_steps=2, null_value=0.0)
    want, _ = _trained(tmp_path, "union", [_union(micro[:2]), _union(micro[2:])], null_value=0.0)
    assert tr.last_stats["optimizer_steps"] == 2
    _assert_same_step(got, want)
    # the plain mean of the two masked gradients of each window, stepped by hand
    plain = _TinyMSGAT()
    opt = torch.optim.Adam(plain.parameters(), lr=1e-3, weight_decay=5e-4)
    for pair in (micro[:2], micro[2:]):
        grads = []
        for X, H, D, y in pair:
            opt.zero_grad(set_to_none=True)
            engine.masked_huber_loss(plain(X, H, D), y, DELTA, 0.0).backward()
            grads.append([p.grad.clone() for p in plain.parameters()])
        for p, a, b in zip(plain.parameters(), *grads):
            p.grad = (a + b) / 2
        opt.step()
    assert not all(torch.allclose(p.detach(), q.detach(), rtol=RTOL, atol=0.0)
                   for p, q in zip(plain.parameters(), want.parameters()))
    assert max(rel_err(p.grad, q.grad) for p, q in zip(plain.parameters(), want.parameters())) > 1e3 * RTOL


def test_five_batches_with_a_window_of_two_are_three_steps(tmp_path):
    micro = [_batch(3, 40 + i) for i in range(5)]
    got, tr = _trained(tmp_path, "window", micro, accumulate_steps=2)
    assert tr.last_stats["optimizer_steps"] == 3
    assert all(float(tr.optimizer.state[p]["step"]) == 3.0 for p in got.parameters())
    assert tr._cpu_window is None                                 # the last, shorter window closed with the epoch
    line = open(tr.log_file).read().splitlines()[0]
    assert "[Train   ] - epoch=1,loss=" in line and line.endswith("optimizer_steps=3")
    tr.run_epoch(micro[:1], epoch=1, mode="validate")             # validation takes no step and reports none
    assert "optimizer_steps" not in tr.last_stats


def test_one_nan_in_the_second_micro_batch_leaves_the_window_out(tmp_path):
    micro = [_batch(3, 50), _batch(3, 51)]
    micro[1][0][1, 0, 1, 2, 7] = float("nan")
    got, tr = _trained(tmp_path, "window", micro, accumulate_steps=2, skip_nonfinite=True)
    for p, s in zip(got.parameters(), _TinyMSGAT().parameters()):
        assert torch.equal(p.detach(), s.detach())
    assert tr.last_stats["skipped_steps"] == 1 and tr.last_stats["optimizer_steps"] == 1
    assert not tr.optimizer.state                                 # no step count, no moment


def test_a_changed_set_of_gradients_inside_a_window_is_refused(tmp_path):
    from ms_gat_amd import engine
    model = _TinyMSGAT()
    tr = engine.Trainer(model, DELTA, str(tmp_path / "run"), accumulate_steps=2)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    tr._window_step(3, 1, close=False)
    model.mix.bias.grad = None
    with pytest.raises(RuntimeError, match="mix.bias"):
        tr._window_step(3, 1, close=True)


@pytest.mark.parametrize("bad", [0, -2, 1.5, True, "2", None])
def test_bad_accumulate_steps_are_refused(tmp_path, bad):
    from ms_gat_amd import engine
    with pytest.raises(ValueError, match="accumulate_steps"):
        engine.Trainer(_TinyMSGAT(), DELTA, str(tmp_path / "bad"), accumulate_steps=bad)


def test_a_window_of_one_is_the_trainer_as_it_was(tmp_path):
    micro = [_batch(3, 60 + i) for i in range(3)]
    got, tr = _trained(tmp_path, "k1", micro, accumulate_steps=1)
    want, plain = _trained(tmp_path, "plain", micro)
    assert tr.accumulate_steps == plain.accumulate_steps == 1
    assert sorted(tr.last_stats) == sorted(plain.last_stats) == ["MAE", "MAPE", "RMSE", "loss"]
    for p, q in zip(got.parameters(), want.parameters()):
        assert torch.equal(p.detach(), q.detach())
    for t in (tr, plain):
        lines = open(t.log_file).read().splitlines()
        assert len(lines) == 1 and "optimizer_steps" not in lines[0]
