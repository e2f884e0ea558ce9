"""Host side of the guarded optimizer step (global-norm clipping, non-finite steps left out): the new C-ABI entry points
and their error codes, and `Trainer(max_grad_norm, skip_nonfinite)` on CPU parameters -- the torch restatement of what
the library does on the GPU -- against a hand-written `clip_grad_norm_` + skip + `optim.Adam` loop.  No device compute."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT

DELTA = 50.0
INF = float("inf")


@pytest.fixture(scope="module")
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


_NEW = {"msgat_grad_guard_partial_doubles": 1, "msgat_grad_guard": 9, "msgat_adam_step_guarded": 19}


def test_guard_entry_points_are_declared_exported_and_bound_under_abi_10(built_library):
    from ms_gat_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in _NEW.items():
        assert hasattr(h, name), name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.exported_symbols() and len(_lib._PROTOTYPES[name][1]) == n_args, name
    assert re.search(r"#define\s+MSGAT_ABI_VERSION\s+10\b", code)
    assert _lib.ABI_VERSION == 10 and _lib.lib().msgat_abi_version() == 10
    assert re.search(r"#define\s+MSGAT_GUARD_FLOATS\s+%d\b" % _lib.GUARD_FLOATS, code)
    # the unguarded update keeps its signature
    assert len(_lib._PROTOTYPES["msgat_adam_step"][1]) == 18
    assert len(re.search(r"\bmsgat_adam_step\s*\(([^)]*)\)", code).group(1).split(",")) == 18


def test_guard_entry_points_report_bad_arguments_before_any_launch(built_library):
    from ms_gat_amd import _lib
    L = _lib.lib()
    x = C.cast(C.create_string_buffer(64), C.c_void_p)       # a non-NULL pointer; nothing is launched on these paths
    assert L.msgat_grad_guard(x, x, 1, x, None, 0.0, x, x, None) == -2             # max_norm <= 0
    assert L.msgat_grad_guard(x, x, 1, x, None, -1.0, x, x, None) == -2
    assert L.msgat_grad_guard(x, x, 1, x, None, float("nan"), x, x, None) == -2    # a NaN max_norm
    assert L.msgat_grad_guard(x, x, 1, x, None, 1.0, x, None, None) == -1          # a null guard
    assert L.msgat_grad_guard(x, x, 1, x, None, INF, x, None, None) == -1
    assert L.msgat_grad_guard(x, x, 1, x, None, 1.0, None, x, None) == -1          # chunks without partials
    assert L.msgat_grad_guard(x, x, 1, None, None, 1.0, x, x, None) == -1
    assert L.msgat_grad_guard(x, x, -1, x, None, 1.0, x, x, None) == -2
    adam = [x, x, x, x, 1, x, 1, x, x, x, x, x, 0.9, 0.999, 1e-8, 5e-4, None]
    assert L.msgat_adam_step_guarded(*adam, None, None) == -1                        # a null guard
    assert L.msgat_adam_step_guarded(*adam[:12], 1.0, 0.999, 1e-8, 5e-4, None, x, None) == -2
    assert L.msgat_adam_step_guarded(*adam[:4], -1, *adam[5:], x, None) == -2
    # the workspace query: one double per chunk; the library allocates nothing
    assert L.msgat_grad_guard_partial_doubles(0) == 0 and L.msgat_grad_guard_partial_doubles(-3) == 0
    assert L.msgat_grad_guard_partial_doubles(957) == 957


def test_bad_max_grad_norm_is_refused_on_the_host(tmp_path):
    from ms_gat_amd import engine
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            engine.Trainer(_TinyMSGAT(), DELTA, str(tmp_path / "bad"), max_grad_norm=bad)
        with pytest.raises(ValueError):
            engine.FlatAdam([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=bad)


# ---- Trainer on CPU parameters: the same semantics in torch ops ---------------------------------------------------------
class _TinyMSGAT(torch.nn.Module):
    """CPU stand-in with the MSGAT call signature model(X, H, D) -> [B,N,T]."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.mix = torch.nn.Conv2d(4, 1, 1)

    def forward(self, X, H, D):
        B, R, C_, N, T = X.shape
        return self.mix(X.reshape(B, R * C_, N, T)).squeeze(1)


POISONED = 2     # the batch with a NaN in X: a sensor that was down, which `null_value` (a mask of the truth) does not catch


def _batches():
    g = torch.Generator().manual_seed(11)
    out = []
    for i in range(5):
        # the input scale sweeps, so the gradient norm does: some steps clip, some do not
        X = torch.randn(8, 2, 2, 5, 12, generator=g) * (0.02, 40.0, 40.0, 0.02, 10.0)[i]
        y = X.reshape(8, 4, 5, 12).mean(1) + 0.05 * torch.randn(8, 5, 12, generator=g)
        out.append((X, torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long), y))
    out[POISONED][0][3, 1, 0, 2, 7] = float("nan")
    return out


def _by_hand(max_norm):
    """clip_grad_norm_, skip on a non-finite norm, optim.Adam: what a user of the reference's loop would write."""
    from ms_gat_amd import engine
    model = _TinyMSGAT()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    skipped, norms = 0, []
    for X, H, D, y in _batches():
        opt.zero_grad(set_to_none=True)
        engine.huber_loss(model(X, H, D), y, DELTA).backward()
        norm = float(torch.nn.utils.clip_grad_norm_(list(model.parameters()), INF if max_norm is None else max_norm))
        norms.append(norm)
        if not math.isfinite(norm):
            skipped += 1
            continue
        opt.step()
    return model, opt, skipped, norms


@pytest.mark.parametrize("max_norm", [0.5, None])
def test_cpu_trainer_with_the_guard_equals_clip_skip_and_adam_written_by_hand(tmp_path, max_norm):
    from ms_gat_amd import engine
    want, want_opt, skipped, norms = _by_hand(max_norm)
    finite = [n for n in norms if math.isfinite(n)]
    assert skipped == 1 and not math.isfinite(norms[POISONED])
    if max_norm is not None:     # the sweep does what it is there for
        assert min(finite) < max_norm < max(finite)
    model = _TinyMSGAT()
    tr = engine.Trainer(model, DELTA, str(tmp_path / "run"), max_grad_norm=max_norm, skip_nonfinite=True)
    assert isinstance(tr.optimizer, torch.optim.Adam)
    tr.run_epoch(_batches(), epoch=1, mode="train")
    for p, q in zip(model.parameters(), want.parameters()):
        assert torch.isfinite(p).all() and torch.equal(p.detach(), q.detach())
    for p, q in zip(model.parameters(), want.parameters()):     # the skipped step advanced no step count
        assert float(tr.optimizer.state[p]["step"]) == float(want_opt.state[q]["step"]) == 4.0
    assert tr.last_stats["skipped_steps"] == 1
    assert tr.last_stats["grad_norm_max"] == pytest.approx(max(finite), rel=1e-6)
    stats = tr.guard_stats()
    assert stats["skipped_steps"] == 1 and stats["grad_norm"] == pytest.approx(norms[-1], rel=1e-6)
    assert stats["clip_coef"] == pytest.approx(1.0 if max_norm is None else min(1.0, max_norm / (norms[-1] + 1e-6)), rel=1e-6)
    # a second epoch reports ITS skipped steps and restarts the maximum
    tr.run_epoch(_batches()[:2], epoch=2, mode="train")
    assert tr.last_stats["skipped_steps"] == 0 and tr.guard_stats()["skipped_steps"] == 1
    lines = open(tr.log_file).read().splitlines()
    assert len(lines) == 4 and ["guard" in ln for ln in lines] == [False, True, False, True]
    assert "[Train   ] - guard - epoch=1,skipped_steps=1,grad_norm_max=" in lines[1]
    # validation takes no step: no guard line, no guard keys
    tr.run_epoch(_batches()[:1], epoch=2, mode="validate")
    assert "skipped_steps" not in tr.last_stats and len(open(tr.log_file).read().splitlines()) == 5


def test_clipping_alone_still_leaves_a_non_finite_step_out(tmp_path):
    from ms_gat_amd import engine
    want, _, _, _ = _by_hand(0.5)
    model = _TinyMSGAT()
    tr = engine.Trainer(model, DELTA, str(tmp_path / "run"), max_grad_norm=0.5)
    tr.run_epoch(_batches(), epoch=1, mode="train")
    assert tr.last_stats["skipped_steps"] == 1
    for p, q in zip(model.parameters(), want.parameters()):
        assert torch.equal(p.detach(), q.detach())


def test_default_trainer_reports_and_logs_what_it_did_before(tmp_path):
    from ms_gat_amd import engine
    tr = engine.Trainer(_TinyMSGAT(), DELTA, str(tmp_path / "plain"))
    assert tr.max_grad_norm is None and tr.skip_nonfinite is False
    clean = [b for i, b in enumerate(_batches()) if i != POISONED]
    tr.run_epoch(clean, epoch=1, mode="train")
    assert sorted(tr.last_stats) == ["MAE", "MAPE", "RMSE", "loss"]
    lines = open(tr.log_file).read().splitlines()
    assert len(lines) == 1 and "guard" not in lines[0] and "[Train   ] - epoch=1,loss=" in lines[0]
    # and the unguarded step is torch.optim.Adam's, NaN and all: the guard is what keeps a poisoned batch out
    tr.run_epoch(_batches(), epoch=2, mode="train")
    assert not all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
