"""K26 without a GPU: the C ABI entries of oly_iq_q_*, the float64 restatement of tests/iq_restate.py against the three
reference-run fixtures of tests/golden/gen_iq_q_update.py (and the two wrong readings, which must miss them), the sweep's
table held to its purpose, the argument checks of olympic_hip.iq and DeviceReplayMemory's ring on CPU tensors."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import iq_restate as R
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = R.TOL
K26_ENTRIES = ("oly_iq_q_ws", "oly_iq_q_ws_values", "oly_iq_q_update")
FIXTURES = ("iq_target", "iq_notarget", "sqil")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_declares_the_k26_entry_points():
    raw = _header()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in K26_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    k26 = raw[raw.index("K26 :"):]
    for cite in ("iq_sac.py:373-420, 467-595, 621-647, 674-676", "sqil_sac.py:64-136", "v0", "gradient_penalty_lambda"):
        assert cite in k26, cite
    define = lambda n: int(re.search(rf"#define {n} (\d+)", txt).group(1))
    assert {k: define("OLY_IQ_ALGO_" + k.upper()) for k in _abi.IQ_ALGO} == _abi.IQ_ALGO
    assert {k: define("OLY_IQ_" + k.upper()) for k in _abi.IQ_PLCY_LOSS_MODES} == _abi.IQ_PLCY_LOSS_MODES
    assert {k: define("OLY_SQIL_" + k.upper()) for k in _abi.SQIL_PLCY_LOSS_MODES} == _abi.SQIL_PLCY_LOSS_MODES
    assert {k: define("OLY_IQ_REG_" + k.upper()) for k in _abi.IQ_REGULARIZER_MODES} == _abi.IQ_REGULARIZER_MODES
    assert len(_abi.IQ_Q_TAGS) == 16 and set(R.IQ_MODES) | {"v0"} == set(_abi.IQ_PLCY_LOSS_MODES)
    assert set(R.SQIL_MODES) == set(_abi.SQIL_PLCY_LOSS_MODES) and set(R.REG_MODES) == set(_abi.IQ_REGULARIZER_MODES)


def test_struct_layout_matches_the_header(tmp_path):
    cls = _abi.IQQ
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             'printf("size %zu\\n", sizeof(oly_iq_q));']
    lines += [f'printf("{f} %zu\\n", offsetof(oly_iq_q, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    assert len(out) == len(cls._fields_) + 1
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_workspace_sizes_and_refusals():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    sizes = [int(L.oly_iq_q_ws(b, 32, 11)) for b in (2, 16, 17, 64, 512, 4096)]
    assert sizes[0] == sizes[1] > 0 and all(a < b for a, b in zip(sizes[1:], sizes[2:]))
    assert int(L.oly_iq_q_ws(64, 1, 1)) == int(L.oly_iq_q_ws(64, 48, 16)) == sizes[3]
    # per row and gradient pass: 64 + 512 + 256 activations, 512 + 256 + 1 deltas; three passes; the transposed W2
    assert sizes[1] >= 3 * 16 * 1601 + 256 * 512 and sizes[5] >= 3 * 4096 * 1601 + 256 * 512
    for b in (2, 18, 4096):
        off = int(L.oly_iq_q_ws_values(b, 12, 5))
        assert 0 < off and off + 3 * ((b + 15) // 16 * 16) <= int(L.oly_iq_q_ws(b, 12, 5))
    for bad in ((1, 12, 5), (0, 12, 5), (-1, 12, 5), (4097, 12, 5), (18, 0, 5), (18, 12, 0), (18, 12, 17), (18, 60, 5),
                (18, 64, 1)):
        assert int(L.oly_iq_q_ws(*bad)) == -1, bad
        assert int(L.oly_iq_q_ws_values(*bad)) == -1, bad
    # a NULL context is refused before anything is read
    assert L.oly_iq_q_update(None, None, None) == _abi.OLY_EINVAL
    assert L.oly_iq_q_update(None, ctypes.byref(_abi.IQQ()), None) == _abi.OLY_EINVAL


# ------------------------------------------------------------------------------ the restatement against the reference runs
def fixture_run(g, name, wrong=None, dtype=torch.float64):
    import gen_iq_q_update as gen
    spec = gen.FIXTURES[name]
    cfg = R.Cfg(algo=spec["algo"], mode=spec["mode"], reg=spec["reg"], treat=False, use_target=spec["use_target"],
                standardizer=True, gamma=float(g["gamma"]), alpha=float(g["alpha"]), reg_mult=float(g["reg_mult"]), R_min=0.0,
                R_max=1.0, lr=float(g["lr"]), tau=float(g["tau"]))
    init = [gen.w2_init(12) if n == "w2" else g[f"critic_init_{n}"] for n in R.NAMES]
    steps = [{k: g[k][i] for k in ("obs", "act", "next_obs", "absorbing", "a_next", "logp_next", "a_pi", "logp_pi")}
             for i in range(gen.N_ITER)]
    return R.run(init, cfg, steps, int(g["n_policy"]), dtype=dtype, wrong=wrong), gen


def fixture_miss(g, state, gen, prefix="critic", key="params"):
    """The largest distance of a restated state's parameters from the stored ones (layer 2: its stored rows)."""
    worst = 0.0
    for n, a in zip(R.NAMES, state[key]):
        r = g[f"{prefix}_w2_head"] if n == "w2" else g[f"{prefix}_{n}"]
        worst = max(worst, float(np.abs((a[:gen.W2_HEAD] if n == "w2" else a) - r).max()))
    return worst


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_reference_run(golden, name):
    g = golden(f"iq_q_update/{name}.npz")
    (state, out), gen = fixture_run(g, name)
    tol_p, tol_t = max(TOL, 4 * float(g["spread_params"])), max(TOL, 4 * float(g["spread_target"]))
    err_p, err_t = fixture_miss(g, state, gen), fixture_miss(g, state, gen, "target", "target")
    print(f"{name}: parameters {err_p:.3e} (tolerance {tol_p:.3e}), target {err_t:.3e} ({tol_t:.3e})")
    assert err_p <= tol_p and err_t <= tol_t
    scal = g["scalars"]
    logged = ~np.isnan(scal)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * float(g["spread_scalars"]))
    assert np.all(np.abs(out - scal)[logged] <= tol[logged])
    # what each algorithm logs: IQ every slot, SQIL neither Loss2, Chi2, V nor the absorbing states' Q
    assert logged.all() if name != "sqil" else (logged.sum(axis=1) == 11).all()
    for got, want in ((state["colstats"], g["colstats"]), (state["tcolstats"], g["target_colstats"])):
        assert np.array_equal(got[0], want[0])
        assert np.all(np.abs(got - want) <= np.maximum(TOL * np.maximum(1.0, np.abs(want)), 4 * float(g["spread_stats"])))
    # the live Standardizer leaves an update two batches later with a target, three without; the target's has its own
    n = gen.N_ITER * gen.B
    assert g["colstats"][0, 0] == (2 if g["use_target"] else 3) * n
    assert g["target_colstats"][0, 0] == (n if g["use_target"] else 0)
    # about a fifth of the rows are absorbing, in both halves
    ab = g["absorbing"]
    assert ab[:, :gen.N_POLICY].sum() >= 8 and ab[:, gen.N_POLICY:].sum() >= 8 and 0.15 < ab.mean() < 0.35


@pytest.mark.parametrize("name", FIXTURES)
def test_the_wrong_readings_miss_the_reference_run(golden, name):
    g = golden(f"iq_q_update/{name}.npz")
    tol = max(TOL, 4 * float(g["spread_params"]))
    for wrong in ("one_stats", "shared_target"):
        (state, _), gen = fixture_run(g, name, wrong=wrong)
        miss, stored = fixture_miss(g, state, gen), float(g[f"miss_{wrong}"])
        print(f"{name} {wrong}: misses the stored parameters by {miss / tol:.1f} tolerances (stored {stored / tol:.1f})")
        if wrong == "shared_target" and not g["use_target"]:
            assert stored == 0.0 and miss <= tol        # the target network is never run
        else:
            assert stored > 10 * tol and miss > 10 * tol


def test_float32_restatement_of_a_fixture_lies_within_its_spread(golden):
    g = golden("iq_q_update/iq_target.npz")
    (state, _), gen = fixture_run(g, "iq_target", dtype=torch.float32)
    assert fixture_miss(g, state, gen) <= max(TOL, 4 * float(g["spread_params"]))


def test_update_target_is_two_float32_products_and_an_add():
    w = torch.tensor([1.0, 3.0, -7.0, 1e-3], dtype=torch.float32)
    t = torch.tensor([2.0, -5.0, 11.0, 1.0], dtype=torch.float32)
    got = R.update_target(0.005, w, t).numpy()
    want = (np.float32(0.005) * w.numpy()).astype(np.float32) + (np.float32(0.995) * t.numpy()).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(R.update_target(1.0, w, t).numpy(), w.numpy())
    assert np.array_equal(R.update_target(0.0, w, t).numpy(), t.numpy())


# ------------------------------------------------------------------------------ the sweep's table
def test_the_sweep_covers_every_mode_once():
    seen = [j for k in range(len(R.SHAPES)) for j, _ in R.sweep(k)]
    assert sorted(seen) == list(range(len(R.CONFIGS))) and len(R.CONFIGS) == 4 * 4 * 2 * 2 + 3 * 2
    iq = {(c.mode, c.reg, c.treat, c.use_target) for c in R.CONFIGS if c.algo == "iq"}
    assert len(iq) == 64
    assert {(c.mode, c.use_target) for c in R.CONFIGS if c.algo == "sqil"} == {(m, t) for m in R.SQIL_MODES for t in (True, False)}
    assert R.SHAPES == ((1, 1, 2, 1), (12, 5, 18, 9), (16, 16, 16, 8), (32, 11, 48, 24), (48, 16, 33, 1)) and R.UPDATES == 3
    for k in range(len(R.SHAPES)):
        assert {c.standardizer for _, c in R.sweep(k)} == {True, False}
        assert {c.use_target for _, c in R.sweep(k)} == {True, False}
        assert any(c.wd > 0 for _, c in R.sweep(k))
    # an empty absorbing subset (NaN in both) at B = 2, filled ones elsewhere
    assert np.isnan(R.yardstick(0, R.sweep(0)[0][0])[1][:, 13]).all()
    assert not np.isnan(R.yardstick(1, R.sweep(1)[0][0])[1][:, 13:15]).all()


@pytest.mark.parametrize("k", range(len(R.SHAPES)), ids=["-".join(map(str, s)) for s in R.SHAPES])
def test_every_case_of_the_sweep_is_one_float32_can_hold(k):
    """torch's own float32 run lies within TOL / 4 of float64 on the parameters and the target, and every tensor moves by
    10 TOL: a case that fails the first cannot tell a kernel from a rounding, one that fails the second tests nothing.
    The output bias is left out of the second: its gradient is the sum of the rows' coefficients, in which IQ's
    loss_term1 (-1 over the expert rows) and loss_term2 (+1) cancel, so only the regulariser and the weight decay move
    it, and with the regulariser off it stands still in the reference too."""
    steps, params = R.sweep_inputs(k)
    for j, cfg in R.sweep(k):
        ref, ref_out, f32, _ = R.yardstick(k, j)
        for key in ("params", "target"):
            spread = float(np.abs(R.cat(f32[key]) - R.cat(ref[key])).max())
            assert spread <= TOL / 4, (j, R.cfg_id(cfg), key, spread)
        for name, p0, p1 in zip(R.NAMES[:5], params, ref["params"]):
            assert float(np.abs(p1 - p0.astype(np.float64)).max()) >= 10 * TOL, (j, name)
        assert np.isfinite(ref_out[:, :13]).all() and np.isfinite(ref_out[:, 15]).all()


# ------------------------------------------------------------------------------ the module's argument checks
def _fake_engine():
    return types.SimpleNamespace(device=torch.device("cpu"))


def _policy(in_dim=12, act_dim=5):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy as P
    pol = object.__new__(P)
    pol.in_dim, pol.act_dim, pol.stand = in_dim, act_dim, None
    return pol


def _critic(D=17):
    from olympic_hip.iq import DeviceSoftQCritic as Q
    c = object.__new__(Q)
    c.D = D
    return c


def _demo(n=6, in_dim=12, A=5):
    return dict(states=np.zeros((n, in_dim)), actions=np.zeros((n, A)), next_states=np.zeros((n, in_dim)),
                absorbing=np.zeros(n))


def test_critic_argument_checks():
    from olympic_hip._ffi import OlyError
    from olympic_hip.iq import DeviceSoftQCritic as Q
    eng = _fake_engine()
    lins = lambda d=17, h1=512, h2=256, out=1: [torch.nn.Linear(d, h1), torch.nn.Linear(h1, h2), torch.nn.Linear(h2, out)]
    with pytest.raises(OlyError, match="three Linear"):
        Q(eng, lins()[:2])
    for bad in (lins(h1=256), lins(out=2), lins(d=65), lins(d=1)):
        with pytest.raises(OlyError, match="512 -> 256 -> 1"):
            Q(eng, bad)
    with pytest.raises(OlyError, match="whole row"):
        Q(eng, lins(), standardizer=types.SimpleNamespace(dim=12))
    with pytest.raises(OlyError, match="tau"):
        Q(eng, lins(), tau=1.5)


def test_trainer_argument_checks():
    from olympic_hip._ffi import OlyError
    from olympic_hip.iq import FOLLOW_UP, DeviceIQLearn as IQ, DeviceSQIL as SQIL
    eng, pol, cr = _fake_engine(), _policy(), _critic()
    mk = lambda cls=IQ, policy=pol, critic=cr, demo=None, **kw: cls(eng, policy, critic, _demo() if demo is None else demo,
                                                                    0.99, 8, True, **kw)
    with pytest.raises(OlyError, match="must be a DeviceSquashedGaussianPolicy"):
        mk(policy=object())
    with pytest.raises(OlyError, match="must be a DeviceSoftQCritic"):
        mk(critic=object())
    for kw, what in ((dict(learnable_alpha=True), "learnable_alpha"), (dict(gradient_penalty_lambda=0.1), "gradient_penalty"),
                     (dict(plcy_loss_mode="v0"), "v0")):
        with pytest.raises(OlyError, match=what) as e:
            mk(**kw)
        assert FOLLOW_UP in str(e.value)
    with pytest.raises(OlyError, match="plcy_loss_mode"):
        mk(plcy_loss_mode="plcy")                      # SQIL's mode, not IQ's
    with pytest.raises(OlyError, match="plcy_loss_mode"):
        mk(cls=SQIL, plcy_loss_mode="value_expert")    # IQ's mode, not SQIL's
    with pytest.raises(OlyError, match="regularizer_mode"):
        mk(regularizer_mode="both")
    with pytest.raises(OlyError, match="> 64"):
        mk(policy=_policy(60, 5), critic=_critic(65))
    with pytest.raises(OlyError, match="the critic takes"):
        mk(critic=_critic(16))
    for k in ("states", "actions", "next_states", "absorbing"):
        d = _demo()
        del d[k]
        with pytest.raises(OlyError, match=f"no '{k}'"):
            mk(demo=d)
    with pytest.raises(OlyError, match="states"):
        mk(demo=dict(_demo(), states=np.zeros((6, 11))))
    with pytest.raises(OlyError, match="actions"):
        mk(demo=dict(_demo(), actions=np.zeros((6, 4))))
    with pytest.raises(OlyError, match="rows"):
        mk(demo=dict(_demo(), absorbing=np.zeros(5)))
    with pytest.raises(OlyError, match="batch_size"):
        IQ(eng, pol, cr, _demo(), 0.99, 0, True)
    with pytest.raises(OlyError, match="batch_size"):
        IQ(eng, pol, cr, _demo(), 0.99, 2049, True)
    # a state_mask picks the demonstrations' columns; the defaults are the reference's
    a = mk(demo=dict(_demo(), states=np.zeros((6, 20)), next_states=np.zeros((6, 20))), state_mask=list(range(12)))
    assert tuple(a.demo["states"].shape) == (6, 12) and a._iter == 1 and a.plcy_loss_mode == "value"
    assert abs(a.alpha - 1e-3) < 1e-9 and a.reg_mult == 0.5 and a.regularizer_mode == "exp_and_plcy"
    s = mk(cls=SQIL, R_min=-1.0, R_max=2.0)
    assert (s.plcy_loss_mode, s.R_min, s.R_max, s._has_v(), a._has_v()) == ("plcy", -1.0, 2.0, False, True)
    import olympic_hip
    assert olympic_hip.DeviceIQLearn is IQ and olympic_hip.DeviceSQIL is SQIL


# ------------------------------------------------------------------------------ the replay memory's ring
class NumpyReplay:
    """mushroom-rl's ReplayMemory.add / size / initialized restated sample by sample, for the rows' order alone."""

    def __init__(self, initial, max_size):
        self.initial, self.max, self.idx, self.full, self.rows = initial, max_size, 0, False, [None] * max_size

    def add(self, rows):
        for r in rows:
            self.rows[self.idx] = r
            self.idx += 1
            if self.idx == self.max:
                self.full, self.idx = True, 0

    @property
    def size(self):
        return self.max if self.full else self.idx


def test_replay_memory_ring_against_numpy():
    from olympic_hip._ffi import OlyError
    from olympic_hip.iq import DeviceReplayMemory
    mem, ref = DeviceReplayMemory(_fake_engine(), 5, 10, 3, 2), NumpyReplay(5, 10)
    rng = np.random.default_rng(0)
    with pytest.raises(OlyError, match="empty"):
        mem.get(2)
    tag = 0
    for n in (3, 2, 1, 4, 7, 10, 23, 0, 1):
        ids = np.arange(tag, tag + n, dtype=np.float32)
        tag += n
        mem.add(dict(states=np.repeat(ids[:, None], 3, 1), actions=np.repeat(ids[:, None], 2, 1) + 0.5,
                     next_states=np.repeat(ids[:, None], 3, 1) + 0.25, absorbing=ids % 2, rewards=-ids, last=ids % 3 == 0))
        ref.add(ids.tolist())
        assert mem.size == ref.size and mem.initialized == (ref.size > 5) and mem._idx == ref.idx
        want = np.array([np.nan if r is None else r for r in ref.rows])
        have = mem.blocks["states"][:, 0].numpy()
        filled = ~np.isnan(want)
        assert np.array_equal(have[filled], want[filled])
        assert np.array_equal(mem.blocks["actions"][filled, 1].numpy(), want[filled] + 0.5)
        assert np.array_equal(mem.blocks["rewards"][filled].numpy(), -want[filled])
    g = torch.Generator().manual_seed(3)
    s, a, r, ns, ab, last = mem.get(64, g)
    assert tuple(s.shape) == (64, 3) and tuple(a.shape) == (64, 2) and tuple(ab.shape) == (64,)
    assert torch.equal(a[:, 0], s[:, 0] + 0.5) and torch.equal(ns, s + 0.25) and torch.equal(r, -s[:, 0])
    assert set(s[:, 0].tolist()) <= set(ref.rows) and len(set(s[:, 0].tolist())) > 5       # the stored rows, with replacement
    st = mem.state_dict()
    other = DeviceReplayMemory(_fake_engine(), 5, 10, 3, 2)
    other.load_state_dict(st)
    assert other.size == mem.size and torch.equal(other.blocks["states"], mem.blocks["states"])
