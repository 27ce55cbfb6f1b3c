"""LSIQ (K26's third algorithm) without a GPU: the C ABI of the block oly_lsiq and of the grown oly_iq_q, the float64
restatement of tests/lsiq_restate.py against the four reference-run fixtures of tests/golden/gen_lsiq_q_update.py (and the
wrong readings, which must miss them), the sweep's table held to its purpose, and the argument checks of DeviceLSIQ."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import iq_restate as R
import lsiq_restate as L
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = L.TOL
FIXTURES = ("iq_fix", "iq_bootstrap", "sqil_value_plcy", "sqil_fix_value")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_and_abi_tables_agree():
    raw = _header()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    define = lambda n: int(re.search(rf"#define {n} (\d+)", txt).group(1))
    assert _abi.IQ_ALGO["lsiq"] == define("OLY_IQ_ALGO_LSIQ") == 2
    assert {k: define("OLY_LSIQ_" + k.upper()) for k in _abi.LSIQ_PLCY_LOSS_MODES} == _abi.LSIQ_PLCY_LOSS_MODES
    assert {k: define("OLY_LSIQ_SQ_" + k.upper()) for k in _abi.LSIQ_SQIL_LIKE_MODES} == _abi.LSIQ_SQIL_LIKE_MODES
    assert {k: define("OLY_LSIQ_" + k.upper()) for k in _abi.LSIQ_LOSSQ_TYPES} == _abi.LSIQ_LOSSQ_TYPES
    assert {k: define("OLY_LSIQ_EXP_" + k.upper()) for k in _abi.LSIQ_LOSS_MODES_EXP} == _abi.LSIQ_LOSS_MODES_EXP
    assert {k: define("OLY_LSIQ_LOSS_" + ("NONE" if k is None else k.upper())) for k in _abi.LSIQ_Q_EXP_LOSSES} == \
        _abi.LSIQ_Q_EXP_LOSSES
    # iq_like extends IQ's modes by number; the restatement's names are the tables'
    assert all(_abi.LSIQ_PLCY_LOSS_MODES[k] == v for k, v in _abi.IQ_PLCY_LOSS_MODES.items())
    assert set(L.IQ_LIKE_MODES) | {"v0"} == set(_abi.LSIQ_PLCY_LOSS_MODES)
    assert set(L.SQIL_LIKE_MODES) == set(_abi.LSIQ_SQIL_LIKE_MODES)
    k26 = raw[raw.index("K26 :"):]
    assert "lsiq.py:9-195" in k26
    assert "lsiq.py:9-195" in open(os.path.join(ROOT, "olympics-mujoco_amd", "csrc", "k26_iq_critic.hip")).read()
    # no entry point of its own: LSIQ goes through oly_iq_q_update
    assert not re.search(r"\boly_lsiq\w*\s*\(", txt)
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION


@pytest.mark.parametrize("struct,cls", (("oly_lsiq", "LSIQ"), ("oly_iq_q", "IQQ")))
def test_struct_layout_matches_the_header(tmp_path, struct, cls):
    cls = getattr(_abi, cls)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             f'printf("size %zu\\n", sizeof({struct}));']
    lines += [f'printf("{f} %zu\\n", offsetof({struct}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    assert len(out) == len(cls._fields_) + 1
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f
    if struct == "oly_iq_q":        # the struct grew at its end alone, by the pointer to the block
        assert cls._fields_[-1][0] == "lsiq" and cls._fields_[-2][0] == "out"
        assert cls.lsiq.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(cls)


def test_a_null_context_is_refused_before_the_block_is_read():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    f = _abi.IQQ(algo=_abi.IQ_ALGO["lsiq"])
    assert _ffi.lib().oly_iq_q_update(None, ctypes.byref(f), None) == _abi.OLY_EINVAL


# ------------------------------------------------------------------------------ the restatement against the reference runs
def fixture_run(g, name, wrong=None, dtype=torch.float64, check=False):
    import gen_lsiq_q_update as gen
    cfg = gen.twin_cfg(gen.FIXTURES[name], float(g["alpha"]), lr=float(g["lr"]), tau=float(g["tau"]), gamma=float(g["gamma"]))
    assert cfg.reg_mult == float(g["reg_mult"]) and cfg.q_min == float(g["Q_min"]) and cfg.q_max == float(g["Q_max"])
    init = [gen.w2_init(12) if n == "w2" else g[f"critic_init_{n}"] for n in R.NAMES]
    steps = [{k: g[k][i] for k in ("obs", "act", "next_obs", "absorbing", "a_next", "logp_next", "a_pi", "logp_pi")}
             for i in range(gen.N_ITER)]
    return L.run(init, cfg, steps, int(g["n_policy"]), dtype=dtype, wrong=wrong, check=check), gen


def fixture_miss(g, state, gen, prefix="critic", key="params"):
    """The largest distance of a restated state's parameters from the stored ones (layer 2: its stored rows)."""
    worst = 0.0
    for n, a in zip(R.NAMES, state[key]):
        r = g[f"{prefix}_w2_head"] if n == "w2" else g[f"{prefix}_{n}"]
        worst = max(worst, float(np.abs((a[:gen.W2_HEAD] if n == "w2" else a) - r).max()))
    return worst


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_reference_run(golden, name):
    g = golden(f"lsiq_q_update/{name}.npz")
    (state, out, margins), gen = fixture_run(g, name, check=True)
    spec = gen.FIXTURES[name]
    L.assert_margins(margins, name)
    tol_p, tol_t = max(TOL, 4 * float(g["spread_params"])), max(TOL, 4 * float(g["spread_target"]))
    err_p, err_t = fixture_miss(g, state, gen), fixture_miss(g, state, gen, "target", "target")
    print(f"{name}: parameters {err_p:.3e} (tolerance {tol_p:.3e}), target {err_t:.3e} ({tol_t:.3e})")
    assert err_p <= tol_p and err_t <= tol_t
    scal = g["scalars"]
    logged = ~np.isnan(scal)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * float(g["spread_scalars"]))
    assert np.all(np.abs(out - scal)[logged] <= tol[logged])
    # what each loss type logs: iq_like every slot, sqil_like all but V (its Chi2 slot is the constant 0.0)
    assert logged.all() if spec["type"] == "iq_like" else (logged.sum(axis=1) == 15).all() and not logged[:, 3].any()
    for got, want in ((state["colstats"], g["colstats"]), (state["tcolstats"], g["target_colstats"])):
        assert np.array_equal(got[0], want[0])
        assert np.all(np.abs(got - want) <= np.maximum(TOL * np.maximum(1.0, np.abs(want)), 4 * float(g["spread_stats"])))
    # the live Standardizer's rows per update: X0, X1 without a target, and the value pass's (n_policy for value_plcy)
    n_v = gen.N_POLICY if spec["mode"] == "value_plcy" else gen.B
    per = gen.B + (0 if spec["use_target"] else gen.B) + n_v
    assert g["colstats"][0, 0] == gen.N_ITER * per
    assert g["target_colstats"][0, 0] == (gen.N_ITER * gen.B if spec["use_target"] else 0)
    assert g["a_pi"].shape == (gen.N_ITER, n_v, gen.ACT_DIM) and g["logp_pi"].shape == (gen.N_ITER, n_v)
    # the policy's Standardizer: next_obs, the value pass and logging_loss's draw on the expert rows
    assert g["policy_colstats"][0, 0] == gen.N_ITER * (gen.B + n_v + gen.B - gen.N_POLICY)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_wrong_readings_miss_the_reference_run(golden, name):
    g = golden(f"lsiq_q_update/{name}.npz")
    tol = max(TOL, 4 * float(g["spread_params"]))
    import gen_lsiq_q_update as gen
    assert gen.FIXTURES[name]["wrong"]
    for wrong in gen.FIXTURES[name]["wrong"]:
        (state, _), _ = fixture_run(g, name, wrong=wrong)
        miss = fixture_miss(g, state, gen)
        print(f"{name}: {wrong} misses by {miss:.3e} = {miss / tol:.1f} tolerances (stored {float(g['miss_' + wrong]):.3e})")
        assert miss > tol, (wrong, miss, tol)
        assert float(g["miss_" + wrong]) > tol


def test_the_fixtures_hold_data_only(golden):
    for name in FIXTURES:
        g = golden(f"lsiq_q_update/{name}.npz")
        for k in g.files:
            assert g[k].dtype.kind in "fiu", (name, k, g[k].dtype)
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lsiq_q_update", name + ".npz")) < 1 << 20


def test_float32_follows_float64_on_the_fixtures(golden):
    """The reference runs in float32: the restatement in float32 stays within the stored spread's reach of float64."""
    g = golden("lsiq_q_update/sqil_value_plcy.npz")
    (s64, _), gen = fixture_run(g, "sqil_value_plcy")
    (s32, _), _ = fixture_run(g, "sqil_value_plcy", dtype=torch.float32)
    assert float(np.abs(L.cat(s32["params"]) - L.cat(s64["params"])).max()) <= TOL


# ------------------------------------------------------------------------------ the restatement against IQ's
def test_lsiq_without_its_additions_is_iq():
    """iq_like, bootstrap, no clipping: the restatement gives iq_restate's numbers exactly (the same torch lines)."""
    k = 1
    steps, params = L.sweep_inputs(k)
    n_policy = L.SHAPES[k][3]
    for mode, reg, tgt in (("value", "exp_and_plcy", True), ("q_old_policy", "exp", False), ("value_policy", "off", False)):
        cfg = L.LCfg(exp_mode="bootstrap", exp_loss=None, clip=False, mode=mode, reg=reg, use_target=tgt)
        a, a_out = L.run(params, cfg, steps, n_policy)
        b, b_out = R.run(params, L.as_iq(cfg), steps, n_policy)
        assert np.array_equal(L.cat(a["params"]), L.cat(b["params"])) and np.array_equal(a_out, b_out)
    assert L.as_iq(L.LCfg()) is None and L.as_iq(L.LCfg(exp_mode="bootstrap", clip=False, mode="off")) is None


def test_the_clip_passes_the_gradient_on_its_bounds_and_not_for_nan():
    """What the kernel's mask restates: torch.clip's backward is 1 where Q_min <= x <= Q_max, bounds included, 0 for NaN."""
    x = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0, float("nan")], dtype=torch.float32, requires_grad=True)
    y = torch.clip(x, -1.0, 1.0)
    y.sum().backward()
    assert x.grad.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert np.isnan(float(y.detach()[5]))
    # Huber's backward at the kink: the residual itself at |d| = 1, the sign beyond
    d = torch.tensor([-3.0, -1.0, 0.5, 1.0, 3.0], requires_grad=True)
    torch.nn.functional.huber_loss(d, torch.zeros(5), reduction="sum").backward()
    assert d.grad.tolist() == [-1.0, -1.0, 0.5, 1.0, 1.0]


# ------------------------------------------------------------------------------ the sweep's table
def test_the_sweep_covers_what_it_claims():
    cs = L.CONFIGS
    experts = {(c.type, c.exp_mode, c.exp_loss, c.clip, c.use_target) for c in cs}
    assert len(experts) == len(cs) == 28
    assert {c.mode for c in cs if c.type == "iq_like"} == set(L.IQ_LIKE_MODES)
    assert {c.reg for c in cs if c.type == "iq_like"} == set(R.REG_MODES)
    assert {c.mode for c in cs if c.type == "sqil_like"} == set(L.SQIL_LIKE_MODES)
    for typ in ("iq_like", "sqil_like"):
        assert {(c.standardizer, c.treat) for c in cs if c.type == typ} == {(a, b) for a in (0, 1) for b in (0, 1)}
    for j, c in enumerate(cs):                      # sqil_like / value only where the halves are equal
        if c.type == "sqil_like" and c.mode == "value":
            _, _, B, n_policy = L.SHAPES[L.shape_of(j)]
            assert 2 * n_policy == B
    assert sorted(j for k in range(len(L.SHAPES)) for j, _ in L.sweep(k)) == list(range(len(cs)))
    assert all(L.sweep(k) for k in range(len(L.SHAPES)))


@pytest.mark.parametrize("k", (1, 4))
def test_the_sweeps_margins_hold(k):
    """Two of the five shapes here (the GPU test asserts all of them through lsiq_restate.yardstick): every update of every
    config keeps next_v and Huber's residuals away from their kinks and has rows of every kind."""
    steps, params = L.sweep_inputs(k)
    n_policy = L.SHAPES[k][3]
    for j, c in L.sweep(k):
        _, _, margins = L.run(params, c, L.case_steps(c, steps, n_policy), n_policy, check=True)
        L.assert_margins(margins, (k, L.cfg_id(c)))
        assert len(margins) == L.UPDATES


# ------------------------------------------------------------------------------ the host classes
class _Eng:
    device = torch.device("cpu")


def _parts():
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.iq import DeviceSoftQCritic
    policy = DeviceSquashedGaussianPolicy.__new__(DeviceSquashedGaussianPolicy)
    policy.in_dim, policy.act_dim, policy.stand = 12, 5, None
    critic = DeviceSoftQCritic.__new__(DeviceSoftQCritic)
    critic.D = 17
    demo = dict(states=np.zeros((4, 12), np.float32), actions=np.zeros((4, 5), np.float32),
                next_states=np.zeros((4, 12), np.float32), absorbing=np.zeros(4, np.float32))
    return policy, critic, demo


def test_device_lsiq_is_a_device_iq_learn_with_the_references_defaults():
    import olympic_hip
    from olympic_hip.iq import DeviceIQLearn, DeviceIQSAC, DeviceLSIQ, DeviceLSIQSAC, _PolicySide
    assert olympic_hip.DeviceLSIQ is DeviceLSIQ and olympic_hip.DeviceLSIQSAC is DeviceLSIQSAC
    assert "DeviceLSIQ" in olympic_hip.__all__ and "DeviceLSIQSAC" in olympic_hip.__all__
    assert issubclass(DeviceLSIQ, DeviceIQLearn) and issubclass(DeviceLSIQSAC, DeviceLSIQ)
    assert issubclass(DeviceLSIQSAC, _PolicySide) and DeviceLSIQSAC.update_policy is DeviceIQSAC.update_policy
    assert (DeviceLSIQ.ALGO, DeviceLSIQ.KIND, DeviceLSIQSAC.KIND) == ("lsiq", "lsiq_critic", "lsiq_sac")
    policy, critic, demo = _parts()
    a = DeviceLSIQ(_Eng(), policy, critic, demo, 0.99, 9, True, Q_exp_loss="MSE")
    assert (a.Q_max, a.Q_min, a.loss_mode_exp, a.treat_absorbing_states, a.target_clipping, a.lossQ_type) == \
        (1.0, -1.0, "fix", False, True, "iq_like")
    assert a._algo_block()["lsiq"] == dict(lossQ_type="iq_like", loss_mode_exp="fix", Q_exp_loss="MSE", target_clipping=True,
                                           Q_min=-1.0, Q_max=1.0)
    assert a._has_v() and a._logs_before_value() and a._unlogged_slots() == ()
    for mode in ("q_old_policy", "off", "value_q_old_policy"):      # getV(obs) runs in every iq_like mode
        assert DeviceLSIQ(_Eng(), policy, critic, demo, 0.99, 9, True, Q_exp_loss="Huber", plcy_loss_mode=mode)._has_v()
    s = DeviceLSIQ(_Eng(), policy, critic, demo, 0.99, 9, True, Q_exp_loss="Huber", lossQ_type="sqil_like",
                   plcy_loss_mode="value_plcy")
    obs = torch.zeros(18, 12)
    assert s._value_rows(obs, 9).shape == (9, 12) and a._value_rows(obs, 9).shape == (18, 12)
    assert not s._logs_before_value() and s._unlogged_slots() == (3,)
    q = DeviceLSIQ(_Eng(), policy, critic, demo, 0.99, 9, True, Q_exp_loss="MSE", lossQ_type="sqil_like",
                   plcy_loss_mode="q_old_policy")
    assert not q._has_v()


def test_device_lsiq_refuses_what_the_reference_raises_on():
    from olympic_hip._ffi import OlyError
    from olympic_hip.iq import DeviceLSIQ
    policy, critic, demo = _parts()
    make = lambda **kw: DeviceLSIQ(_Eng(), policy, critic, demo, 0.99, 9, True, **kw)
    make(loss_mode_exp="bootstrap")                                  # the one place Q_exp_loss=None is valid
    for kw in (dict(), dict(Q_exp_loss=None, loss_mode_exp="fix"), dict(lossQ_type="sqil_like", loss_mode_exp="bootstrap"),
               dict(Q_exp_loss="L1"), dict(Q_exp_loss="MSE", lossQ_type="other"), dict(Q_exp_loss="MSE", loss_mode_exp="both"),
               dict(Q_exp_loss="MSE", Q_min=1.0, Q_max=1.0), dict(Q_exp_loss="MSE", Q_min=float("nan")),
               dict(Q_exp_loss="MSE", plcy_loss_mode="v0"), dict(Q_exp_loss="MSE", plcy_loss_mode="value_plcy"),
               dict(Q_exp_loss="MSE", lossQ_type="sqil_like", plcy_loss_mode="value_expert"),
               dict(Q_exp_loss="MSE", lossQ_type="sqil_like", plcy_loss_mode="off"),
               dict(Q_exp_loss="MSE", gradient_penalty_lambda=1.0), dict(Q_exp_loss="MSE", learnable_alpha=True)):
        with pytest.raises(OlyError):
            make(**kw)


def test_the_examples_take_the_lsiq_options():
    for name in ("iq_fit.py", "iq_q_fit.py"):
        src = open(os.path.join(ROOT, "examples", name)).read()
        for opt in ("lsiq", "--lossq-type", "--loss-mode-exp", "--q-exp-loss", "--q-min", "--q-max", "--no-target-clipping"):
            assert opt in src, (name, opt)

