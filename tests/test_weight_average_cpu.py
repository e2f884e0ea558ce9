"""Host side of the averaged weights (an exponential moving average of the parameters kept by the fused Adam step): the two
C-ABI entry points and their status codes, the numpy restatements against each other, and `Trainer(ema_decay=...)` on CPU
parameters -- the torch restatement of what the library does on the GPU -- through training, validation, checkpoints and
`Evaluator(weights=...)`.  No device compute."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import weight_average_ref as ref

DELTA = 50.0
NEW = {"msgat_adam_step_averaged": 21, "msgat_param_swap": 6}


@pytest.fixture(scope="module")
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


# ---- declarations and status codes -----------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound_under_abi_10(built_library):
    from ms_gat_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW.items():
        assert hasattr(h, name), name
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name
        assert name in _lib.exported_symbols() and len(_lib._PROTOTYPES[name][1]) == n_args, name
    assert "msgat_adam_step_averaged and msgat_param_swap" in header.split("#define MSGAT_ABI_VERSION")[0]
    assert re.search(r"#define\s+MSGAT_ABI_VERSION\s+10\b", code)
    assert _lib.ABI_VERSION == 10 and _lib.lib().msgat_abi_version() == 10
    # the two updates that existed keep their signatures
    assert len(_lib._PROTOTYPES["msgat_adam_step"][1]) == 18 and len(_lib._PROTOTYPES["msgat_adam_step_guarded"][1]) == 19


def test_entry_points_report_bad_arguments_before_any_launch(built_library):
    from ms_gat_amd import _lib
    L = _lib.lib()
    x = C.cast(C.create_string_buffer(64), C.c_void_p)       # a non-NULL pointer; nothing is launched on these paths
    adam = [x, x, x, x, 1, x, 1, x, x, x, x, x, 0.9, 0.999, 1e-8, 5e-4, None]
    for guard in (None, x):                                  # a NULL guard is the unguarded update, not an error
        assert L.msgat_adam_step_averaged(*adam, guard, None, 0.999, None) == -1     # a null shadow
        for decay in (-0.1, 1.0, float("nan")):
            assert L.msgat_adam_step_averaged(*adam, guard, x, decay, None) == -2
    assert L.msgat_adam_step_averaged(*adam[:4], -1, *adam[5:], None, x, 0.5, None) == -2
    assert L.msgat_adam_step_averaged(*adam[:12], 1.0, 0.999, 1e-8, 5e-4, None, None, x, 0.5, None) == -2   # beta1 = 1
    assert L.msgat_adam_step_averaged(*adam[:10], None, x, *adam[12:], None, x, 0.5, None) == -1            # no step counts
    # nothing to update: both launches are left out, and so is the swap's
    assert L.msgat_adam_step_averaged(None, None, None, None, 0, None, 0, None, None, None, x, x, 0.9, 0.999, 1e-8, 5e-4,
                                      None, None, x, 0.0, None) == 0
    assert L.msgat_param_swap(None, None, None, 0, None, None) == 0
    assert L.msgat_param_swap(x, x, x, 0, x, None) == 0
    assert L.msgat_param_swap(x, x, x, -1, x, None) == -2
    assert L.msgat_param_swap(x, x, x, 1, None, None) == -1
    assert L.msgat_param_swap(None, x, x, 1, x, None) == -1


# ---- the restatements -------------------------------------------------------------------------------------------------
K = 12


@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_float32_restatement_follows_the_float64_one(decay):
    """Random walks of K = 12 steps.  Bound 5 K 2^-24 max|w|: a step rounds three times (w - e, omd times that, e plus that),
    each on a magnitude of at most 2 max|w| and so by at most 2^-24 * 2 max|w| / 2 ... in all under 5 * 2^-24 max|w| with the
    rounding of omd itself; the map e -> d e + (1 - d) w is a contraction (d <= 1), so the steps' errors add, never grow."""
    rng = np.random.default_rng(7)
    w = rng.standard_normal(4096).astype(np.float32) * np.float32(3.0)
    start = w.copy()
    walk = []
    for _ in range(K):
        w = (w + np.float32(0.05) * rng.standard_normal(w.size).astype(np.float32)).astype(np.float32)
        walk.append(w)
    top = max(float(np.abs(x).max()) for x in [start, *walk])
    e32 = ref.run(ref.average_f32, start, walk, decay)
    e64 = ref.run(ref.average_f64, start, walk, decay)
    worst = float(np.abs(e32.astype(np.float64) - e64).max())
    bound = 5 * K * 2.0 ** -24 * top
    print(f"decay {decay}: float32 vs float64 restatement, worst {worst:.3e}, bound {bound:.3e}")
    assert e32.dtype == np.float32 and worst <= bound
    assert worst > 0.0 or decay == 0.0           # the two are different computations, not one taken twice


def test_decay_regimes_warm_up_then_cap():
    """decay = 0.5 meets the warm-up at t = 8, (1 + 8) / (10 + 8) = 0.5, and caps from there on; 0.999 is never reached
    within the test.  Rates are compared as bits: every quotient here is the float32 nearest to the exact one."""
    warm = [np.float32(1.0) - np.float32(1.0 + t) / np.float32(10.0 + t) for t in range(1, K + 1)]
    half = [ref.rate_f32(0.5, t) for t in range(1, K + 1)]
    slow = [ref.rate_f32(0.999, t) for t in range(1, K + 1)]
    assert all(h == w and h > 0.5 for h, w in zip(half[:7], warm[:7]))          # t = 1 .. 7: the warm-up, d < 0.5
    assert (1.0 + 8) / (10.0 + 8) == 0.5 and half[7] == np.float32(0.5)          # they meet at t = 8
    assert all(h == np.float32(0.5) for h in half[7:]) and warm[8] < 0.5         # the cap from there on
    assert slow == warm and all(s > np.float32(1.0) - np.float32(0.999) for s in slow)
    assert half[0] == np.float32(1.0) - np.float32(2.0) / np.float32(11.0)       # t = 1: d = 2 / 11
    # t = 0 would be d = 0.1; the first update a tensor sees has t = 1 (the count is advanced before it is read)
    assert float(ref.rate_f32(0.999, 10 ** 6)) == pytest.approx(1e-3, rel=1e-4)  # far out: the cap, 1 - decay


def test_torch_rate_has_the_bits_of_the_restatement():
    from ms_gat_amd import engine
    for decay in (0.0, 0.5, 0.9, 0.999):
        for t in (1, 2, 7, 8, 9, 100, 12345):
            got = engine.average_rate(decay, torch.tensor(float(t)))
            assert got.dtype == torch.float32 and ref.same_bits(got.numpy(), ref.rate_f32(decay, t)), (decay, t)


# ---- Trainer on CPU parameters: the same semantics in torch ops ---------------------------------------------------------
class _Tiny(torch.nn.Module):
    """CPU stand-in with the MSGAT call signature model(X, H, D) -> [B,N,T]; `spare` never receives a gradient and
    `frozen` does not require one."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.mix = torch.nn.Conv2d(4, 1, 1)
        self.spare = torch.nn.Parameter(torch.randn(5))
        self.frozen = torch.nn.Parameter(torch.randn(3), requires_grad=False)

    def forward(self, X, H, D):
        B, R, C_, N, T = X.shape
        return self.mix(X.reshape(B, R * C_, N, T)).squeeze(1)


POISONED = 2


def _batches(n=5, poison=False, seed=11):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        X = torch.randn(8, 2, 2, 5, 12, generator=g) * (0.5, 4.0, 2.0, 0.1, 1.0)[i % 5]
        y = X.reshape(8, 4, 5, 12).mean(1) + 0.05 * torch.randn(8, 5, 12, generator=g)
        out.append((X, torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long), y))
    if poison:
        out[POISONED][0][3, 1, 0, 2, 7] = float("nan")
    return out


def _trained(model):
    return [p for p in model.parameters() if p.requires_grad]


def _at(model, p):
    """The place of parameter `p` among the trainable ones (the order of the shadows)."""
    return [i for i, q in enumerate(_trained(model)) if q is p][0]


def _bits_equal(a, b):
    return ref.same_bits(a.detach().numpy(), b.detach().numpy())


@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_cpu_trainer_shadow_has_the_bits_of_the_restatement(tmp_path, decay):
    from ms_gat_amd import engine
    model = _Tiny()
    tr = engine.Trainer(model, DELTA, str(tmp_path / "run"), ema_decay=decay)
    assert isinstance(tr.optimizer, torch.optim.Adam) and tr.ema_decay == decay
    params = _trained(model)
    assert len(tr._cpu_shadow) == len(params) == 3           # not the frozen one
    want = [p.detach().numpy().copy() for p in params]
    start = copy.deepcopy(want)
    for k, batch in enumerate(_batches(12, seed=5)):         # one batch per epoch call: the parameters after every step
        tr.run_epoch([batch], epoch=1, mode="train")
        for i, p in enumerate(params):
            if p.grad is not None:
                assert float(tr.optimizer.state[p]["step"]) == k + 1
                want[i] = ref.average_f32(want[i], p.detach().numpy(), decay, k + 1)
    for i, (p, e) in enumerate(zip(params, tr._cpu_shadow)):
        assert ref.same_bits(e.numpy(), want[i]), i
    # the parameter without a gradient: Adam skipped it, and its shadow is what it started as
    spare, mixed = _at(model, model.spare), _at(model, model.mix.weight)
    assert model.spare.grad is None and ref.same_bits(tr._cpu_shadow[spare].numpy(), start[spare])
    assert not ref.same_bits(tr._cpu_shadow[mixed].numpy(), start[mixed])
    assert not _bits_equal(tr._cpu_shadow[mixed], params[mixed])     # the average lags the weights


def test_a_step_the_guard_leaves_out_leaves_the_shadow_bits_alone(tmp_path):
    from ms_gat_amd import engine
    model = _Tiny()
    tr = engine.Trainer(model, DELTA, str(tmp_path / "run"), ema_decay=0.5, skip_nonfinite=True)
    batches = _batches(5, poison=True)
    tr.run_epoch(batches[:POISONED], epoch=1, mode="train")
    before = [e.clone() for e in tr._cpu_shadow]
    weights = [p.detach().clone() for p in _trained(model)]
    tr.run_epoch([batches[POISONED]], epoch=1, mode="train")
    assert tr.last_stats["skipped_steps"] == 1
    assert all(_bits_equal(a, b) for a, b in zip(before, tr._cpu_shadow))
    assert all(_bits_equal(a, b) for a, b in zip(weights, _trained(model)))
    # the next finite step uses t as if the skipped one had not happened: t = 3, not 4
    tr.run_epoch([batches[POISONED + 1]], epoch=1, mode="train")
    p, at = model.mix.weight, _at(model, model.mix.weight)
    assert float(tr.optimizer.state[p]["step"]) == 3.0
    assert not _bits_equal(tr._cpu_shadow[at], before[at])
    assert ref.same_bits(tr._cpu_shadow[at].numpy(), ref.average_f32(before[at].numpy(), p.detach().numpy(), 0.5, 3))


def _loaders():
    return _batches(3, seed=21), _batches(2, seed=22)


def test_fit_validates_on_the_averaged_weights_and_gives_the_raw_ones_back(tmp_path):
    from ms_gat_amd import engine
    model = _Tiny()
    tr = engine.Trainer(model, DELTA, str(tmp_path / "run"), ema_decay=0.9)
    tr.max_epochs = 1
    train, val = _loaders()
    # the same epoch by hand on a copy, to know the raw weights and the shadow that fit must end with
    twin = _Tiny()
    by_hand = engine.Trainer(twin, DELTA, str(tmp_path / "twin"), ema_decay=0.9)
    by_hand.run_epoch(train, epoch=1, mode="train")
    averaged = _Tiny()
    averaged.load_state_dict({**twin.state_dict(), **by_hand.averaged_state()["shadow"]})
    want_loss = engine.Engine(averaged, DELTA, str(tmp_path / "avg")).run_epoch(val, mode="validate")
    raw_loss = engine.Engine(twin, DELTA, str(tmp_path / "raw")).run_epoch(val, mode="validate")
    tr.fit((train, val))
    assert tr.last_stats["loss"] == want_loss and want_loss != raw_loss
    for p, q in zip(model.parameters(), twin.parameters()):          # the raw weights are back, bit for bit
        assert _bits_equal(p, q)
    for e, f in zip(tr._cpu_shadow, by_hand._cpu_shadow):
        assert _bits_equal(e, f)
    lines = open(tr.log_file).read().splitlines()
    assert len(lines) == 3 and "[Validate] - average - epoch=1,decay=0.9" in lines[2]
    assert f"loss={want_loss}" in lines[1]


def test_averaged_parameters_restores_when_the_block_raises_and_refuses_a_step(tmp_path):
    from ms_gat_amd import engine
    model = _Tiny()
    tr = engine.Trainer(model, DELTA, str(tmp_path / "run"), ema_decay=0.5)
    tr.run_epoch(_batches(3), epoch=1, mode="train")
    raw = [p.detach().clone() for p in _trained(model)]
    shadow = [e.clone() for e in tr._cpu_shadow]
    with pytest.raises(ZeroDivisionError):
        with tr.averaged_parameters():
            assert all(_bits_equal(p, e) for p, e in zip(_trained(model), shadow))
            assert all(_bits_equal(e, p) for e, p in zip(tr._cpu_shadow, raw))
            1 / 0
    assert all(_bits_equal(p, q) for p, q in zip(_trained(model), raw))
    assert all(_bits_equal(e, f) for e, f in zip(tr._cpu_shadow, shadow))
    with tr.averaged_parameters():
        with pytest.raises(RuntimeError, match="swapped in"):
            tr.run_epoch(_batches(1), epoch=1, mode="train")
        with pytest.raises(RuntimeError, match="swapped in"):
            tr.averaged_state()
    plain = engine.Trainer(_Tiny(), DELTA, str(tmp_path / "plain"))
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.averaged_parameters():
            pass


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, float("nan"), "0.9", True])
def test_bad_decay_is_refused_on_the_host(tmp_path, bad):
    from ms_gat_amd import engine
    with pytest.raises(ValueError, match="ema_decay"):
        engine.Trainer(_Tiny(), DELTA, str(tmp_path / "bad"), ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        engine.FlatAdam([torch.nn.Parameter(torch.zeros(3))], ema_decay=bad)


def test_flat_adam_takes_a_decay_without_touching_the_device():
    from ms_gat_amd import engine
    opt = engine.FlatAdam([torch.nn.Parameter(torch.zeros(3))], ema_decay=0.0)
    assert opt.ema_decay == 0.0 and opt.shadow is None and opt.swapped is False and opt.buffer_token() == ()
    assert engine.FlatAdam([torch.nn.Parameter(torch.zeros(3))]).ema_decay is None


# ---- checkpoints ---------------------------------------------------------------------------------------------------------
FIVE = ["best", "epoch", "grad_scaler", "model", "optimizer", "scheduler"]


def test_checkpoint_gains_the_ema_key_only_with_the_average_on(tmp_path):
    from ms_gat_amd import engine
    plain = engine.Trainer(_Tiny(), DELTA, str(tmp_path / "plain"))
    plain.run_epoch(_batches(2), epoch=1, mode="train")
    plain.save(tmp_path / "plain.pkl")
    assert sorted(torch.load(tmp_path / "plain.pkl", weights_only=False)) == FIVE
    model = _Tiny()
    tr = engine.Trainer(model, DELTA, str(tmp_path / "run"), ema_decay=0.75)
    tr.run_epoch(_batches(2), epoch=1, mode="train")
    tr.save(tmp_path / "ema.pkl")
    states = torch.load(tmp_path / "ema.pkl", weights_only=False)
    assert sorted(states) == sorted(FIVE + ["ema"])
    assert sorted(states["ema"]) == ["decay", "shadow"] and states["ema"]["decay"] == 0.75
    assert sorted(states["ema"]["shadow"]) == ["mix.bias", "mix.weight", "spare"]       # the trainable ones, by name
    names = [name for name, p in model.named_parameters() if p.requires_grad]
    for name, e in states["ema"]["shadow"].items():
        assert _bits_equal(e, dict(zip(names, tr._cpu_shadow))[name])
    assert not _bits_equal(states["ema"]["shadow"]["mix.weight"], states["model"]["mix.weight"])
    for name, p in model.state_dict().items():              # `model` stays the raw weights
        assert _bits_equal(states["model"][name], p)


def test_save_load_continue_gives_the_bits_of_an_uninterrupted_run(tmp_path):
    from ms_gat_amd import engine
    batches = _batches(6, seed=9)
    whole = engine.Trainer(_Tiny(), DELTA, str(tmp_path / "whole"), ema_decay=0.5)
    whole.run_epoch(batches, epoch=1, mode="train")
    first = engine.Trainer(_Tiny(), DELTA, str(tmp_path / "first"), ema_decay=0.5)
    first.run_epoch(batches[:3], epoch=1, mode="train")
    first.save(tmp_path / "half.pkl")
    model = _Tiny()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)                                      # whatever it held is replaced
    second = engine.Trainer(model, DELTA, str(tmp_path / "second"), ema_decay=0.5)
    held = [e.data_ptr() for e in second._cpu_shadow]
    second.load(tmp_path / "half.pkl")
    assert held == [e.data_ptr() for e in second._cpu_shadow]            # restored in place
    assert all(_bits_equal(e, f) for e, f in zip(second._cpu_shadow, first._cpu_shadow))
    second.run_epoch(batches[3:], epoch=1, mode="train")
    for p, q in zip(model.parameters(), whole.model.parameters()):
        assert _bits_equal(p, q)
    for e, f in zip(second._cpu_shadow, whole._cpu_shadow):
        assert _bits_equal(e, f)


def test_a_checkpoint_without_ema_starts_the_shadow_at_the_loaded_parameters(tmp_path):
    from ms_gat_amd import engine
    plain = engine.Trainer(_Tiny(), DELTA, str(tmp_path / "plain"))
    plain.run_epoch(_batches(3), epoch=1, mode="train")
    plain.save(tmp_path / "plain.pkl")
    tr = engine.Trainer(_Tiny(), DELTA, str(tmp_path / "run"), ema_decay=0.9)
    tr.run_epoch(_batches(2, seed=4), epoch=1, mode="train")             # a shadow of its own, to be replaced
    tr.load(tmp_path / "plain.pkl")
    for p, q, e in zip(_trained(tr.model), _trained(plain.model), tr._cpu_shadow):
        assert _bits_equal(p, q) and _bits_equal(e, q)
    # and the other way round: a run without the average reads a checkpoint with the key
    tr.save(tmp_path / "ema.pkl")
    plain.load(tmp_path / "ema.pkl")
    assert plain._cpu_shadow is None


def test_evaluator_picks_the_weights(tmp_path):
    from ms_gat_amd import engine
    tr = engine.Trainer(_Tiny(), DELTA, str(tmp_path / "run"), ema_decay=0.9)
    tr.run_epoch(_batches(4), epoch=1, mode="train")
    tr.save(tmp_path / "ema.pkl")
    plain = engine.Trainer(_Tiny(), DELTA, str(tmp_path / "plain"))
    plain.run_epoch(_batches(4), epoch=1, mode="train")
    plain.save(tmp_path / "plain.pkl")
    raw = {k: v.clone() for k, v in tr.model.state_dict().items()}
    averaged = {**raw, **tr.averaged_state()["shadow"]}
    assert not _bits_equal(raw["mix.weight"], averaged["mix.weight"])

    def loaded(ckpt, **kw):
        model = _Tiny()
        ev = engine.Evaluator(model, DELTA, str(tmp_path / "eval"), ckpt, **kw)
        return ev, model.state_dict()

    for kw, want, which in (({}, averaged, "averaged"), ({"weights": "auto"}, averaged, "averaged"),
                            ({"weights": "averaged"}, averaged, "averaged"), ({"weights": "raw"}, raw, "raw")):
        ev, got = loaded(tmp_path / "ema.pkl", **kw)
        assert ev.weights == which and all(_bits_equal(got[k], want[k]) for k in want), kw
    for kw in ({}, {"weights": "raw"}):                      # no key: the raw weights either way
        ev, got = loaded(tmp_path / "plain.pkl", **kw)
        assert ev.weights == "raw" and all(_bits_equal(got[k], v) for k, v in plain.model.state_dict().items())
    with pytest.raises(KeyError, match="'ema'"):
        loaded(tmp_path / "plain.pkl", weights="averaged")
    with pytest.raises(ValueError, match="weights"):
        loaded(tmp_path / "ema.pkl", weights="best")
    # the losses differ, so the choice is visible where it matters
    val = _batches(2, seed=22)
    a = loaded(tmp_path / "ema.pkl")[0].eval(val)
    r = loaded(tmp_path / "ema.pkl", weights="raw")[0].eval(val)
    assert a != r
