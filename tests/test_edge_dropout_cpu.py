"""CPU: edge dropout (`msgat_edge_dropout{,_backward}`, `ops.edge_dropout`, `model.EdgeDropout`, `MSGAT(edge_dropout=p)`,
the Trainer's sixth checkpoint key).  The numpy restatement of the draw against the Random123 known answers and its drop
rate; the two entry points in the header, the ctypes table and the built library; their argument checks, which launch
nothing; the refusals of the op; the options, buffers and state-dict keys of the models.  No device compute is called here.
"""
import copy
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import edge_dropout_ref as ref

NAMES = {"msgat_edge_dropout": 13, "msgat_edge_dropout_backward": 12}


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from ms_gat_amd import build
    return build.build(verbose=False)


# ---- the restatement -------------------------------------------------------------------------------------------------

KNOWN_ANSWERS = [      # Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_restatement_reproduces_the_random123_known_answers(counter, key, want):
    got = tuple(int(x) for x in ref.philox4x32_10(counter, key))
    assert got == want, [hex(x) for x in got]


def test_restatement_reads_word_e_and_3_of_the_quads_call():
    seed, step, V, nnz, off = (1 << 32) + 5, (1 << 32) + 3, 3, 11, 7
    w = ref.words(seed, step, V, nnz, off)
    assert w.shape == (V, nnz) and w.dtype == np.uint32
    for v in range(V):
        for e in range(nnz):
            r = ref.philox4x32_10((e >> 2, off + v, step & 0xffffffff, step >> 32), (seed & 0xffffffff, seed >> 32))
            assert int(w[v, e]) == int(r[e & 3]), (v, e)


def test_constants_are_computed_in_double():
    assert ref.constants(0.0) == (0, np.float32(1.0))
    assert ref.constants(0.5) == (1 << 31, np.float32(2.0))
    thr, scale = ref.constants(0.1)
    assert thr == int(math.floor(0.1 * 2.0 ** 32)) == 429496729 and scale == np.float32(1.0 / 0.9)
    assert ref.constants(1.0 - 2.0 ** -53)[0] == (1 << 32) - 1
    from ms_gat_amd import ops
    for p in (0.0, 0.1, 0.25, 0.5, 0.9):
        thr, scale = ops.edge_dropout_constants(p)
        assert (thr, np.float32(scale)) == ref.constants(p)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5, 0.9])
def test_drop_rate_of_the_restatement(p):
    """|drops - p V nnz| <= 4 sqrt(V nnz p (1 - p)) at every step: a binomial count within four standard deviations."""
    V, nnz, seed = 6, 301, 1234
    masks = [ref.dropped(seed, step, V, nnz, p) for step in range(8)]
    for step, d in enumerate(masks):
        z = abs(int(d.sum()) - p * V * nnz) / math.sqrt(V * nnz * p * (1 - p))
        print(f"p = {p} step {step}: {int(d.sum())} drops, {z:.2f} standard deviations")
        assert z <= 4.0, (p, step, z)
    for a, b in zip(masks, masks[1:]):
        assert not np.array_equal(a, b)                       # consecutive steps
    for d in masks:
        for v in range(V - 1):
            assert not np.array_equal(d[v], d[v + 1])         # different samples


def test_restatement_of_the_forward_and_backward_forms():
    V, nnz, p = 4, 9, 0.5
    rng = np.random.default_rng(0)
    w = rng.standard_normal((V, nnz)).astype(np.float32)
    exempt = np.zeros(nnz, bool)
    exempt[[0, 4]] = True
    m = ref.multipliers(3, 2, V, nnz, p, exempt=exempt)
    assert set(np.unique(m)) <= {np.float32(0), np.float32(1), np.float32(2)} and (m[:, exempt] == 1).all()
    out = ref.forward(w, 3, 2, V, p, exempt=exempt)
    assert np.array_equal(out, w * m)                         # p = 0.5: the scale is exact
    assert not np.signbit(out[m == 0]).any()                  # a dropped edge is +0 whatever the sign of w
    shared = ref.forward(w[0], 3, 2, V, p, exempt=exempt)
    assert np.array_equal(shared, w[0][None] * m)
    dout = rng.standard_normal((V, nnz)).astype(np.float32)
    assert np.array_equal(ref.backward_sets(dout, m), dout * m)
    want = np.zeros(nnz, np.float32)
    for v in range(V):
        for e in range(nnz):
            want[e] = np.float32(want[e] + np.float32(dout[v, e] * m[v, e]))
    assert np.array_equal(ref.backward_shared(dout, m).view(np.int32), want.view(np.int32))
    # the sharded draw: rows [lo, hi) are the draw at sample_offset = lo
    assert np.array_equal(ref.words(3, 2, 7, nnz)[2:5], ref.words(3, 2, 3, nnz, sample_offset=2))


# ---- the library -----------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_prototyped_and_exported_and_the_abi_version_is_still_10():
    from ms_gat_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, f"{name} is not declared in include/msgat_hip.h"
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == n_args and args[-1] == "void* stream", args
        assert [a.rsplit(" ", 1)[0] for a in args[5:11]] == ["int32_t", "int64_t", "int32_t", "int64_t", "uint32_t", "float"]
        assert name in _lib.exported_symbols() and len(_lib._PROTOTYPES[name][1]) == n_args
        assert _lib._PROTOTYPES[name][1][5:11] == [C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_uint32, C.c_float]
        assert hasattr(h, name), f"{name} is not exported by the library"
    assert "edge_dropout.hip" in build.SOURCES
    assert "#define MSGAT_ABI_VERSION 10\n" in header and _lib.ABI_VERSION == 10
    assert _lib.lib().msgat_abi_version() == 10


def test_argument_checks_launch_nothing():
    from ms_gat_amd import _lib
    L = _lib.lib()
    p = 1      # never dereferenced: every call below returns before a launch
    fwd, bwd = L.msgat_edge_dropout, L.msgat_edge_dropout_backward
    thr, scale = 1 << 31, 2.0
    # empty sizes: OK, nothing launched
    assert fwd(p, p, p, p, p, 0, 9, 0, 0, thr, scale, 1, None) == 0 and fwd(p, p, p, p, p, 4, 0, 1, 0, thr, scale, 1, None) == 0
    assert bwd(p, p, p, p, p, 0, 9, 0, 0, thr, scale, None) == 0 and bwd(p, p, p, p, p, 4, 0, 1, 0, thr, scale, None) == 0
    assert bwd(p, p, p, p, None, 4, 9, 1, 0, thr, scale, None) == 0                # no output asked for
    for V, nnz, off in ((-1, 9, 0), (4, -1, 0), (4, 9, -1)):
        assert fwd(p, p, p, p, p, V, nnz, 0, off, thr, scale, 1, None) == -2, (V, nnz, off)
        assert bwd(p, p, p, p, p, V, nnz, 0, off, thr, scale, None) == -2, (V, nnz, off)
    for V, nnz, off in ((4, 1 << 34, 0), (4, 9, (1 << 32) - 3), (1, 9, 1 << 32)):   # the counter's words are 32 bits
        assert fwd(p, p, p, p, p, V, nnz, 0, off, thr, scale, 1, None) == -3, (V, nnz, off)
        assert bwd(p, p, p, p, p, V, nnz, 0, off, thr, scale, None) == -3, (V, nnz, off)
    for missing in (0, 2, 3, 4):             # w, state, used, out; exempt (1) is optional
        args = [p] * 5
        args[missing] = None
        assert fwd(*args, 4, 9, 0, 0, thr, scale, 1, None) == -1, missing
    for missing in (0, 2, 3):                # dout, state, used
        args = [p] * 5
        args[missing] = None
        assert bwd(*args, 4, 9, 0, 0, thr, scale, None) == -1, missing


def test_status_codes_are_the_headers():
    header = open(os.path.join(ROOT, "include", "msgat_hip.h")).read()
    for name, value in (("MSGAT_ERR_NULL", -1), ("MSGAT_ERR_SHAPE", -2), ("MSGAT_ERR_UNSUPPORTED", -3)):
        assert re.search(r"%s\s*=?\s*\(?%d\)?" % (name, value), header), name


def test_op_refuses_cpu_tensors_and_bad_operands():
    from ms_gat_amd import ops
    w = torch.ones(5)
    state = ops.edge_dropout_state(3, "cpu")
    assert state.dtype == torch.int64 and state.tolist() == [3, 0]
    assert ops.edge_dropout_state((1 << 63) + 1, "cpu").tolist() == [-(1 << 63) + 1, 0]      # the same 64 bits
    with pytest.raises(ValueError, match="edge_dropout"):
        ops.edge_dropout(w, 0.5, state, samples=2)                                            # a CPU tensor
    for bad in (1.0, -0.1, 1.5, float("nan"), "0.1", None, True):
        with pytest.raises(ValueError, match="edge_dropout"):
            ops.edge_dropout_constants(bad)


def test_op_checks_run_before_any_launch(monkeypatch):
    """The op's own checks on operands that claim to be on the device: `is_cuda` is the first thing it reads, so CPU tensors
    wrapped to answer True reach every later check; the launch is replaced by a function that fails the test."""
    from ms_gat_amd import ops

    class OnDevice(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    def wrap(t):
        return t.as_subclass(OnDevice)

    monkeypatch.setattr(ops._EdgeDropoutFunction, "apply", lambda *a: pytest.fail("launched"))
    w, state = wrap(torch.ones(5)), ops.edge_dropout_state(0, "cpu")
    with pytest.raises(TypeError, match="edge_dropout"):
        ops.edge_dropout(wrap(torch.ones(5, dtype=torch.float64)), 0.5, state, samples=2)
    for p in (1.0, -0.5, "x"):
        with pytest.raises(ValueError, match="edge_dropout"):
            ops.edge_dropout(w, p, state, samples=2)
    with pytest.raises(ValueError, match="edge_dropout.*samples"):
        ops.edge_dropout(w, 0.5, state)                                   # [nnz] without the number of samples
    with pytest.raises(ValueError, match="edge_dropout"):
        ops.edge_dropout(wrap(torch.ones(2, 5)), 0.5, state, samples=3)   # [V,nnz] with another V
    with pytest.raises(ValueError, match="edge_dropout"):
        ops.edge_dropout(wrap(torch.ones(2, 2, 5)), 0.5, state)
    for bad_state in (torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), [0, 0],
                      torch.zeros(2, dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError, match="edge_dropout.*state"):
            ops.edge_dropout(w, 0.5, bad_state, samples=2)
    for bad_exempt in (torch.zeros(4, dtype=torch.uint8), torch.zeros(5), torch.zeros(5, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match="edge_dropout.*exempt"):
            ops.edge_dropout(w, 0.5, state, samples=2, exempt=bad_exempt)
    for bad_offset in (-1, 1 << 32, 1.5):
        with pytest.raises(ValueError, match="edge_dropout.*sample_offset"):
            ops.edge_dropout(w, 0.5, state, samples=2, sample_offset=bad_offset)


# ---- the models ------------------------------------------------------------------------------------------------------

LEARN = [False, True, "time", "signal"]


def _models(n=32, edges=40):
    import ms_gat_amd
    from ms_gat_amd import model
    adj = ms_gat_amd.synthetic_adjacency(n, edges, seed=5)
    make = lambda learn, **kw: model.msgat48(n_components=3, in_channels=1, in_timesteps=12, out_timesteps=12,  # noqa: E731
                                             use_te=True, adj=adj, learn_edge_weights=learn, **kw)
    return adj, make


def test_bad_edge_dropout_values_raise():
    _, make = _models()
    for bad in (1.0, -0.1, 2, "0.1", None, True, float("nan")):
        with pytest.raises(ValueError, match="edge_dropout"):
            make(False, edge_dropout=bad)
    from ms_gat_amd import model
    with pytest.raises(ValueError, match="edge_dropout"):
        model.EdgeDropout(1.0)


@pytest.mark.parametrize("learn", LEARN)
def test_state_dict_keys_do_not_change_and_the_default_model_has_no_dropout_buffer(learn):
    adj, make = _models()
    plain, dropping = make(learn), make(learn, edge_dropout=0.2, edge_dropout_seed=11)
    assert set(dropping.state_dict()) == set(plain.state_dict())
    assert not any("drop" in name for name, _ in plain.named_buffers()) and plain.edge_dropout == 0.0
    assert plain.edge_dropout_state() is None and plain.edge_dropout_sample_offset == 0
    with pytest.raises(ValueError, match="edge_dropout"):
        plain.set_edge_dropout_state({"seed": 1, "step": 2})
    if learn is False:
        assert plain.adjacency() is plain.adj
        assert dropping.eval().adjacency() is dropping.adj            # eval mode: `adj` itself, as without dropout
        dropping.train()
        with torch.no_grad():
            assert dropping.adjacency() is dropping.adj               # and under no_grad
    names = {name for name, _ in dropping.named_buffers() if "drop" in name}
    want = {"edge_drop_state", "edge_drop_exempt"} | ({"edge_drop_crow", "edge_drop_col", "edge_drop_index"} if not learn else set())
    assert names == want
    assert dropping.edge_dropout_state() == {"seed": 11, "step": 0}
    # the stored diagonal is exempt; keep_self=False exempts nothing
    csr = adj.to_sparse_csr()
    rows = torch.repeat_interleave(torch.arange(len(adj)), csr.crow_indices()[1:] - csr.crow_indices()[:-1])
    assert torch.equal(dropping.edge_drop_exempt.bool(), rows == csr.col_indices()) and int(dropping.edge_drop_exempt.sum()) > 0
    assert make(learn, edge_dropout=0.2, edge_dropout_keep_self=False).edge_drop_exempt is None
    if not learn:
        assert torch.equal(adj.reshape(-1)[dropping.edge_drop_index], csr.values())
    with pytest.raises(ValueError, match="edge_dropout"):
        dropping.adjacency()                                          # training mode: the masks are per sample


def test_stream_position_is_set_restored_and_carried_by_deepcopy():
    _, make = _models()
    net = make(True, edge_dropout=0.3, edge_dropout_seed=(1 << 40) + 9)
    buf = net.edge_drop_state
    net.set_edge_dropout_state({"seed": 5, "step": (1 << 33) + 4})
    assert net.edge_drop_state is buf and buf.tolist() == [5, (1 << 33) + 4]            # in place
    twin = copy.deepcopy(net)
    assert twin.edge_dropout_state() == {"seed": 5, "step": (1 << 33) + 4} and twin.edge_drop_state is not buf
    assert twin.edge_dropout == 0.3
    loaded = make(True, edge_dropout=0.3)
    loaded.load_state_dict(net.state_dict())                          # strict: no missing or unexpected key
    assert loaded.edge_dropout_state() == {"seed": 0, "step": 0}      # the stream is not a state_dict entry


def test_edge_dropout_module():
    from ms_gat_amd import model
    m = model.EdgeDropout(0.25, seed=7, exempt=torch.tensor([True, False, False]))
    assert m.state_dict() == {} and m.state() == {"seed": 7, "step": 0}
    assert m.edge_drop_exempt.dtype == torch.uint8 and m.edge_drop_exempt.tolist() == [1, 0, 0]
    m.set_state({"seed": 7, "step": 12})
    assert copy.deepcopy(m).state() == {"seed": 7, "step": 12}
    w = torch.ones(3)
    assert m.eval()(w, samples=4) is w                                # eval mode: the weights themselves
    with pytest.raises(ValueError, match="edge_dropout"):
        m.train()(w, samples=4)                                       # training mode draws, and the op has no CPU path
    assert model.EdgeDropout(0.0).state_dict() == {}


def test_trainer_checkpoint_has_a_sixth_key_only_when_the_model_drops_edges(tmp_path):
    from ms_gat_amd import engine
    _, make = _models()
    five = {"best", "epoch", "model", "optimizer", "scheduler", "grad_scaler"}
    plain = engine.Trainer(make(True), 50.0, str(tmp_path / "plain"), hip_graph=False)
    plain.save(tmp_path / "plain.pkl")
    assert set(torch.load(tmp_path / "plain.pkl", weights_only=False)) == five
    net = make(True, edge_dropout=0.1, edge_dropout_seed=21)
    tr = engine.Trainer(net, 50.0, str(tmp_path / "drop"), hip_graph=False)
    net.set_edge_dropout_state({"seed": 21, "step": 17})
    tr.save(tmp_path / "drop.pkl")
    states = torch.load(tmp_path / "drop.pkl", weights_only=False)
    assert set(states) == five | {"edge_dropout"} and states["edge_dropout"] == {"seed": 21, "step": 17}
    assert set(states["model"]) == set(make(True).state_dict())
    fresh = make(True, edge_dropout=0.1)
    other = engine.Trainer(fresh, 50.0, str(tmp_path / "fresh"), hip_graph=False)
    other.load(tmp_path / "drop.pkl")
    assert fresh.edge_dropout_state() == {"seed": 21, "step": 17}
    other.load(tmp_path / "plain.pkl")                                # a checkpoint without the key leaves the stream alone
    assert fresh.edge_dropout_state() == {"seed": 21, "step": 17}
