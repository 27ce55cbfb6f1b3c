"""The H update of LSIQ_H / LSIQ_HC (K26's fourth algorithm) without a GPU: the C ABI of the grown block oly_lsiq, the
closed form the kernel computes against the [B, B] broadcast of tests/lsiq_h_restate.py (which restates the reference's
lines), the sweep's table held to its purpose, and the wrong readings, which must miss the right one on the sweep's own
cases.

Which of these fail without the feature: the tests of the ABI, the exports, the schedule and the fixtures (which need
the grown structs, the new classes and the committed reference runs).  The tests that exercise tests/lsiq_h_restate.py
alone (the closed form, the sweep's table, the margins, the wrong readings among the restatement's variants) check the
yardstick itself and would pass on any commit that holds that file; they are here so that the GPU tests' reference is
itself held to something."""
import ctypes
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lsiq_h_restate as H
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
TOL = H.TOL
OLD_MEMBERS = ("lossQ_type", "loss_mode_exp", "Q_exp_loss", "target_clipping", "Q_min", "Q_max")
NEW_MEMBERS = ("h_loss", "h_cost", "h_clip_expert", "h_pad", "h_tau_up", "h_tau_down", "h_max_state", "h_q_t", "h_v_t")


# ------------------------------------------------------------------------------ C ABI
def test_header_and_abi_tables_agree():
    raw = open(os.path.join(ROOT, "include", "olympic_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    define = lambda n: int(re.search(rf"#define {n} (\d+)", txt).group(1))
    assert _abi.IQ_ALGO["lsiq_h"] == define("OLY_IQ_ALGO_LSIQ_H") == 3
    assert {k: define("OLY_LSIQ_LOSS_" + k.upper()) for k in _abi.LSIQ_H_LOSSES} == _abi.LSIQ_H_LOSSES
    assert len(_abi.LSIQ_H_TAGS) == 9 and len(set(_abi.LSIQ_H_TAGS)) == 9
    assert _abi.LSIQ_H_TAGS[:7] == ("H function/Loss", "H function/H", "H function/H plcy", "H function/H expert",
                                    "H function/H_step", "H function/H_step plcy", "H function/H_step expert")
    k26 = raw[raw.index("K26 :"):raw.index("K27 :")]
    for text in ("lsiq_h.py:57-102", "lsiq_hc.py:23-88", "OLY_IQ_ALGO_LSIQ_H"):
        assert text in k26, text
    src = open(os.path.join(ROOT, "olympics-mujoco_amd", "csrc", "k26_iq_critic.hip")).read()
    assert "lsiq_h.py:57-102" in src and "lsiq_hc.py:23-88" in src
    # no entry point of its own: the H update goes through oly_iq_q_update
    assert not re.search(r"\boly_lsiq\w*\s*\(", txt)
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8, "additive: no bump"


def test_the_block_grew_at_its_end_and_matches_the_header(tmp_path):
    cls = _abi.LSIQ
    names = tuple(f for f, _ in cls._fields_)
    assert names == OLD_MEMBERS + NEW_MEMBERS
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             'printf("size %zu\\n", sizeof(oly_lsiq));']
    lines += [f'printf("{f} %zu\\n", offsetof(oly_lsiq, {f}));' for f in names]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for f in names:
        assert int(out[f]) == getattr(cls, f).offset, f
    # the old members keep the offsets of the 24-byte block they were; every new one lies behind them
    assert [getattr(cls, f).offset for f in OLD_MEMBERS] == [0, 4, 8, 12, 16, 20]
    assert min(getattr(cls, f).offset for f in NEW_MEMBERS) == 24
    # a zero-filled tail names no loss: OLY_LSIQ_LOSS_MSE and _HUBER are not 0
    assert 0 not in _abi.LSIQ_H_LOSSES.values()


def test_a_null_context_is_refused_before_the_block_is_read():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    f = _abi.IQQ(algo=_abi.IQ_ALGO["lsiq_h"])
    assert _ffi.lib().oly_iq_q_update(None, ctypes.byref(f), None) == _abi.OLY_EINVAL


# ------------------------------------------------------------------------------ the closed form against the broadcast
def broadcast_loss(cfg, H_, next_H, absorbing, q_t, v_t):
    """The reference's lines from next_H on, in float64 with autograd: H [B, 1] against a [B, B] target.  Returns
    (loss, dL/dH [B])."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    B = len(H_)
    Hc = t(H_).reshape(B, 1).requires_grad_(True)
    next_H, absorbing, gamma = t(next_H).reshape(B, 1), t(absorbing), t(cfg.gamma)
    if cfg.cost:
        Q_plcy, V_plcy = t(q_t).reshape(B, 1), t(v_t).reshape(B, 1)
        y = (1 - absorbing) * gamma * torch.clip(V_plcy, cfg.q_min, cfg.q_max)
        reward_non_abs = torch.square(torch.clip(Q_plcy - y, -1 / cfg.reg_mult, 1 / cfg.reg_mult))
        reward_abs = torch.square(torch.clip(Q_plcy - y, cfg.q_min, cfg.q_max))
        squared = (1 - absorbing) * cfg.reg_mult * reward_non_abs + absorbing * (1.0 - gamma) * cfg.reg_mult * reward_abs
        target = squared + (1 - absorbing) * gamma * next_H
        target = torch.clip(target, -1000, float((1.0 / cfg.reg_mult) ** 2 / (1 - gamma) + 100))
    else:
        target = torch.clip((1 - absorbing) * gamma * next_H, -10000, 1000)
    assert tuple(target.shape) == (B, B)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = F.huber_loss(Hc, target) if cfg.loss == "Huber" else F.mse_loss(Hc, target)
    loss.backward()
    return float(loss.detach()), Hc.grad.reshape(-1).numpy()


def kernel_targets(cfg, next_H, q_t, v_t):
    """The row's two targets as include/olympic_hip.h states them: t0 against the non-absorbing columns, t1 against the
    absorbing ones."""
    g, nH = cfg.gamma, np.asarray(next_H, np.float64)
    if not cfg.cost:
        return np.clip(g * nH, -10000, 1000), np.clip(0.0 * nH, -10000, 1000)
    r, q = 1.0 / cfg.reg_mult, np.asarray(q_t, np.float64)
    vt = np.clip(np.asarray(v_t, np.float64), cfg.q_min, cfg.q_max)
    hi = r * r / (1 - g) + 100
    t0 = cfg.reg_mult * np.square(np.clip(q - g * vt, -r, r)) + g * nH
    t1 = ((1 - g) * cfg.reg_mult) * np.square(np.clip(q, cfg.q_min, cfg.q_max)) + 0.0 * nH
    return np.clip(t0, -1000, hi), np.clip(t1, -1000, hi)


@pytest.mark.parametrize("cost", (False, True), ids=("h", "hc"))
@pytest.mark.parametrize("loss", ("MSE", "Huber"))
@pytest.mark.parametrize("n1", ("0", "1", "2", "B-1"))
def test_closed_form_equals_the_broadcast(cost, loss, n1):
    """Loss and gradient of the closed form against torch's own [B, B] broadcast, at B = 6 and 18, with residuals on both
    Huber branches and LSIQ_HC's values on both sides of its three clips."""
    for B in (6, 18):
        rng = np.random.default_rng(B)
        k = B - 1 if n1 == "B-1" else int(n1)
        absorbing = np.zeros(B)
        absorbing[rng.permutation(B)[:k]] = 1.0
        cfg = H.HCfg(cost=cost, loss=loss, reg_mult=2.0, q_min=H.Q_MIN, q_max=H.Q_MAX)
        H_, next_H = rng.standard_normal(B) * 1.5, rng.standard_normal(B) * 1.5
        q_t, v_t = rng.standard_normal(B) * H.QT_DEV, rng.standard_normal(B) * H.QT_DEV
        want, want_g = broadcast_loss(cfg, H_, next_H, absorbing, q_t, v_t)
        t0, t1 = kernel_targets(cfg, next_H, q_t, v_t)
        if loss == "Huber":
            res = np.abs(np.concatenate([H_ - t0, H_ - t1]))
            assert (res < 1).sum() >= 2 and (res > 1).sum() >= 2
        got, got_g = H.closed_form(H_, t0, t1, k, loss)
        assert abs(got - want) <= 1e-14 * max(1.0, abs(want)), (B, got, want)
        assert np.abs(got_g - want_g).max() <= 1e-15, (B, np.abs(got_g - want_g).max())


def test_the_row_wise_reading_gives_another_loss_when_a_row_is_absorbing():
    """The quirk is not a matter of rounding: at B = 6 with two absorbing rows the plain row-wise TD loss differs from the
    broadcast's in its first digits, and with no absorbing row the two are the same loss."""
    B = 6
    rng = np.random.default_rng(1)
    H_, next_H = rng.standard_normal(B) * 1.5, rng.standard_normal(B) * 1.5
    cfg = H.HCfg()
    for absorbing, same in ((np.array([0, 1, 0, 0, 1, 0.0]), False), (np.zeros(B), True)):
        want, _ = broadcast_loss(cfg, H_, next_H, absorbing, None, None)
        row = float(np.mean(np.square(H_ - np.clip((1 - absorbing) * cfg.gamma * next_H, -10000, 1000))))
        assert (abs(row - want) <= 1e-14) == same, (row, want)
        if not same:
            assert abs(row - want) > 0.05 * want


# ------------------------------------------------------------------------------ the sweep's table
def test_sweep_table_runs_both_classes_and_every_option():
    assert len(H.CONFIGS) == 16
    assert {(c.cost, c.loss, c.clip_expert, c.standardizer) for c in H.CONFIGS} == \
        {(a, b, c, d) for a in (False, True) for b in ("MSE", "Huber") for c in (True, False) for d in (True, False)}
    assert H.SHAPES == ((1, 1, 2, 1), (12, 5, 18, 9), (16, 16, 16, 8), (32, 11, 48, 24), (48, 16, 33, 1))
    assert [c.cost for c in H.CLIPPED] == [False, True] and all(c.alpha > 1 for c in H.CLIPPED)


def test_no_case_of_the_sweep_is_beyond_float32():
    """The yardstick of shape 1 (whose float64 margins lsiq_h_restate.yardstick asserts): torch's own float32 run of every
    case stays within TOL / 4 of float64 on the parameters, so a case tells a kernel from a rounding."""
    for j, cfg in enumerate(H.CONFIGS):
        ref, _, f32, _ = H.yardstick(1, j)
        spread = float(np.abs(H.cat(f32["params"]) - H.cat(ref["params"])).max())
        assert spread <= TOL / 4, (H.cfg_id(cfg), spread)
        if cfg.clip_expert:
            assert abs(f32["max"] - ref["max"]) <= TOL * abs(ref["max"])


def test_with_no_absorbing_row_the_update_is_the_plain_td_update():
    k = 1
    in_dim, A, B, n_policy = H.SHAPES[k]
    steps, params = H.sweep_inputs(k)
    steps = [dict(s, absorbing=np.zeros(B, np.float32)) for s in steps]
    for cfg in (H.CONFIGS[0], H.CONFIGS[12]):
        st = H.case_steps(cfg, steps)
        a, ao = H.run(params, cfg, st, n_policy)
        b, bo = H.run(params, cfg, st, n_policy, wrong="row_wise")
        assert np.abs(H.cat(a["params"]) - H.cat(b["params"])).max() <= 1e-12
        assert np.abs(ao - bo).max() <= 1e-12


@pytest.mark.parametrize("wrong", ("row_wise", "clip_old_max", "h_step_clipped"))
def test_wrong_readings_miss_on_the_sweeps_cases(wrong):
    """Each wrong reading, run in float64 on the cases the GPU test runs at shape 1, leaves the right reading's result by
    several tolerances (the tolerance of tests/test_gpu_lsiq_h.py: max(TOL, 4 x the float32 spread), relative for the
    scalars and moments): a kernel that implemented it would fail there."""
    k = 1
    n_policy = H.SHAPES[k][3]
    steps, params = H.sweep_inputs(k)
    for j, cfg in enumerate(H.CONFIGS):
        if wrong != "row_wise" and not cfg.clip_expert:
            continue
        ref, ref_out, f32, f32_out = H.yardstick(k, j)
        got, got_out = H.run(params, cfg, H.case_steps(cfg, steps), n_policy, wrong=wrong)
        worst = 0.0
        if wrong != "h_step_clipped":                 # the logged scalars alone differ there
            for rk in ("exp_avg", "exp_avg_sq"):
                r = H.cat(ref[rk])
                scale = float(np.abs(r).max())
                tol = max(TOL, 4 * float(np.abs(H.cat(f32[rk]) - r).max()) / scale)
                worst = max(worst, float(np.abs(H.cat(got[rk]) - r).max()) / scale / tol)
        tol = np.maximum(TOL * np.maximum(1.0, np.abs(ref_out)), 4 * np.abs(f32_out - ref_out))
        worst = max(worst, float((np.abs(got_out - ref_out) / tol).max()))
        assert worst >= 5.0, (wrong, H.cfg_id(cfg), worst)


def test_clipped_cases_reach_the_targets_upper_bound():
    """lsiq_h_restate.yardstick asserts, for the two cases with a large alpha, at least two rows' targets above the upper
    clip bound and two inside at every update."""
    for j in range(len(H.CLIPPED)):
        H.yardstick("clipped", j)


# ------------------------------------------------------------------------------ the agents' critic side
def test_the_classes_are_exported_and_derive_from_lsiq():
    import olympic_hip
    from olympic_hip.iq import DeviceLSIQ, DeviceLSIQH, DeviceLSIQHC
    assert olympic_hip.DeviceLSIQH is DeviceLSIQH and olympic_hip.DeviceLSIQHC is DeviceLSIQHC
    assert "DeviceLSIQH" in olympic_hip.__all__ and "DeviceLSIQHC" in olympic_hip.__all__
    assert issubclass(DeviceLSIQH, DeviceLSIQ) and issubclass(DeviceLSIQHC, DeviceLSIQH)
    assert (DeviceLSIQH.KIND, DeviceLSIQHC.KIND) == ("lsiq_h_critic", "lsiq_hc_critic")
    assert (DeviceLSIQH.H_COST, DeviceLSIQHC.H_COST) == (False, True)
    # the Q critic's values carry no entropy, and LSIQ_HC alone defers the Q critic's target update
    assert DeviceLSIQH._q_alpha(None) == 0.0
    assert DeviceLSIQ._q_update_target(None) and DeviceLSIQH._q_update_target(None) and not DeviceLSIQHC._q_update_target(None)


@pytest.mark.parametrize("cost", (False, True), ids=("lsiq_h", "lsiq_hc"))
def test_the_agents_case_holds_its_margins_and_float32_holds_it(cost):
    case = H.agent_case(cost)
    ref, _, _, margins = H.run_agent(case, check=True)
    H.assert_margins(margins, ("agent", cost), counts=False)
    f32 = H.run_agent(case, torch.float32)[0]
    for net in ("q", "h"):
        assert np.abs(H.cat(f32[net]["params"]) - H.cat(ref[net]["params"])).max() <= TOL / 4, net


def test_reading_the_target_after_its_update_misses():
    """LSIQ_HC with the Q critic's target updated before the H update reads it: H's first moments leave the right
    reading's by many tolerances of tests/test_gpu_lsiq_h.py, so the deferred update is pinned by the agents' test."""
    case = H.agent_case(True)
    ref = H.run_agent(case)[0]["h"]
    f32 = H.run_agent(case, torch.float32)[0]["h"]
    got = H.run_agent(case, wrong="target_after")[0]["h"]
    r = H.cat(ref["exp_avg"])
    scale = float(np.abs(r).max())
    tol = max(TOL, 4 * float(np.abs(H.cat(f32["exp_avg"]) - r).max()) / scale)
    assert float(np.abs(H.cat(got["exp_avg"]) - r).max()) / scale >= 5 * tol


# ------------------------------------------------------------------------------ the restatement against the reference runs
@pytest.mark.parametrize("name", H.FIXTURES)
def test_restatement_against_the_reference_run(golden, name):
    """The float64 whole twin, running the policy itself on the recorded noise, lands within max(2e-5, 4 x the stored
    spread) of what the reference's LSIQ_H / LSIQ_HC left after four whole iq_updates: both critics, both targets, the
    POLICY (trained by the reference's two-critic _actor_loss), the seven H scalars of every iteration and the running
    maximum after each.  This is what decides the readings: the [B, B] target, H after Q's step, the expert clip with the
    updated maximum, H_step unclipped, LSIQ_HC's target read before its soft update, the actor loss over q + H with each
    critic's Standardizer fed by the policy step."""
    import gen_lsiq_h_update as gen
    g = golden(f"lsiq_h_update/{name}.npz")
    twin, out = H.fixture_whole(g, name, gen)
    st = twin.state()
    for prefix, params in (("critic", st["q"]["params"]), ("target", st["q"]["target"]), ("h", st["h"]["params"]),
                           ("h_target", st["h"]["target"]), ("policy", st["policy"]["params"])):
        err, tol = H.fixture_errors(g, gen, params, prefix), max(TOL, 4 * float(g[f"spread_{prefix}"]))
        assert err <= tol, (prefix, err, tol)
    scal = g["scalars"][:, :7]
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * float(g["spread_scalars"]))
    assert np.all(np.abs(out[:, :7] - scal) <= tol), np.abs(out[:, :7] - scal) / tol
    assert np.all(np.abs(out[:, 8] - g["maxima"]) <= max(TOL, 4 * float(g["spread_max"])) * np.abs(g["maxima"]))
    # every Standardizer's count: H takes B rows per H update and B per policy step, its target B per H update; the target
    # critic next_obs with a target and LSIQ_HC's two passes whether or not there is one
    spec, n = gen.FIXTURES[name], gen.N_ITER * gen.B
    assert g["h_colstats"][0, 0] == 2 * n and g["h_target_colstats"][0, 0] == n
    assert g["target_colstats"][0, 0] == n * (int(spec["use_target"]) + 2 * int(spec["cost"]))
    for key, rk in ((("h", "colstats"), "h_colstats"), (("h", "tcolstats"), "h_target_colstats"),
                    (("q", "colstats"), "colstats"), (("q", "tcolstats"), "target_colstats"),
                    (("policy", "colstats"), "policy_colstats")):
        assert np.array_equal(st[key[0]][key[1]][0], g[rk][0]), rk


@pytest.mark.parametrize("name", H.FIXTURES)
def test_wrong_readings_miss_the_reference_run(golden, name):
    """Every reading of the generator's list on every fixture: the stored miss is recomputed and exceeds three
    tolerances.  Only target_after is not a reading of LSIQ_H (it has no deferred target), so h_iq stores 0 for it."""
    import gen_lsiq_h_update as gen
    g = golden(f"lsiq_h_update/{name}.npz")
    scal = g["scalars"][:, :7]
    tol_par, tol_scal = max(TOL, 4 * float(g["spread_h"])), max(TOL, 4 * float(g["spread_scalars"]))
    tol_pol = max(TOL, 4 * float(g["spread_policy"]))
    tested = gen.FIXTURES[name]["wrong"] + ("h_before_q", "no_h")
    for wrong in tested:
        st, out = H.fixture_whole(g, name, gen, wrong=wrong)
        st = st.state()
        miss = max(H.fixture_errors(g, gen, st["h"]["params"], "h") / tol_par,
                   float((np.abs(out[:, :7] - scal) / np.maximum(1.0, np.abs(scal))).max()) / tol_scal,
                   H.fixture_errors(g, gen, st["policy"]["params"], "policy") / tol_pol)
        assert miss > 3.0, (wrong, miss)
        assert abs(miss - float(g["miss_" + wrong])) <= 1e-6 * float(g["miss_" + wrong]), wrong
    assert set(gen.WRONG) - set(tested) == (set() if gen.FIXTURES[name]["cost"] else {"target_after"})


# ------------------------------------------------------------------------------ the constructors' refusals
def test_the_constructors_refuse_before_they_touch_the_engine():
    """h_critic, the two rates, H_tau and H_loss_mode are checked before anything is built on the device, so stand-ins
    for the networks are enough here; the refusals that need device objects are tests/test_gpu_lsiq_h.py's."""
    from olympic_hip._ffi import OlyError
    from olympic_hip.iq import DeviceLSIQH, DeviceLSIQHC, DeviceLSIQHCSAC, DeviceLSIQHSAC, DeviceSoftQCritic
    q, h = object.__new__(DeviceSoftQCritic), object.__new__(DeviceSoftQCritic)
    args = (None, None, q, {}, 0.99, 4, True)
    for cls in (DeviceLSIQH, DeviceLSIQHSAC):
        for kw in (dict(), dict(h_critic=None), dict(h_critic="net"), dict(h_critic=q),
                   dict(h_critic=h, max_H_policy_tau_up=1.5), dict(h_critic=h, max_H_policy_tau_down=-0.1),
                   dict(h_critic=h, max_H_policy_tau_up=float("nan"))):
            with pytest.raises(OlyError, match="h_critic|max_H_policy"):
                cls(*args, **kw)
    for cls in (DeviceLSIQHC, DeviceLSIQHCSAC):
        for kw in (dict(h_critic=h), dict(h_critic=h, H_tau=None), dict(h_critic=h, H_tau=1.5), dict(h_critic=h, H_tau=-1.0),
                   dict(h_critic=h, H_tau=0.1, H_loss_mode="L1"), dict(h_critic=h, H_tau=0.1, H_loss_mode=None)):
            with pytest.raises(OlyError, match="H_tau|H_loss"):
                cls(*args, **kw)


# ------------------------------------------------------------------------------ the two-critic actor step
def test_oly_iq_pi_grew_at_its_end_and_matches_the_header(tmp_path):
    cls = _abi.IQPi
    names = [f for f, _ in cls._fields_]
    new = ["h_packed", "h_packed_floats", "h_param", "h_colstats", "h_ws", "h_ws_floats"]
    assert names[-6:] == new and names[-7] == "out"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             'printf("size %zu\\n", sizeof(oly_iq_pi));']
    lines += [f'printf("{f} %zu\\n", offsetof(oly_iq_pi, {f}));' for f in names]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for f in names:
        assert int(out[f]) == getattr(cls, f).offset, f
    assert cls.h_packed.offset == cls.out.offset + 8        # the old block ends where the new members begin
    raw = open(os.path.join(ROOT, "include", "olympic_hip.h")).read()
    assert "lsiq_h.py:104-108" in raw[raw.index("K27 :"):]
    assert "lsiq_h.py:104-108" in open(os.path.join(ROOT, "olympics-mujoco_amd", "csrc", "k27_iq_policy.hip")).read()


def test_the_whole_agents_are_exported():
    import olympic_hip
    from olympic_hip.iq import DeviceIQSAC, DeviceLSIQH, DeviceLSIQHC, DeviceLSIQHCSAC, DeviceLSIQHSAC, _PolicySide
    assert olympic_hip.DeviceLSIQHSAC is DeviceLSIQHSAC and olympic_hip.DeviceLSIQHCSAC is DeviceLSIQHCSAC
    assert "DeviceLSIQHSAC" in olympic_hip.__all__ and "DeviceLSIQHCSAC" in olympic_hip.__all__
    assert issubclass(DeviceLSIQHSAC, DeviceLSIQH) and issubclass(DeviceLSIQHCSAC, DeviceLSIQHC)
    assert issubclass(DeviceLSIQHSAC, _PolicySide) and DeviceLSIQHCSAC.update_policy is DeviceIQSAC.update_policy
    assert (DeviceLSIQHSAC.KIND, DeviceLSIQHCSAC.KIND) == ("lsiq_h_sac", "lsiq_hc_sac")


def test_the_actor_restatement_holds_in_float32_and_tells_the_loss_without_H():
    """Every case of tests/test_gpu_lsiq_h_actor.py: torch's own float32 run stays within TOL / 4 of float64 on the policy,
    and the actor loss without H (the one-critic loss) leaves it by more than five tolerances."""
    import iq_pi_restate as P
    for k in range(len(P.SHAPES)):
        for j, cfg in enumerate(P.CONFIGS):
            y = H.actor_yardstick(k, j)
            ref = H.cat(y[0]["policy"]["params"])
            assert np.abs(H.cat(y[3]["policy"]["params"]) - ref).max() <= TOL / 4, (k, j)
            wrong = H.run_actor(H.actor_case(k), cfg, wrong="no_h")
            assert np.abs(H.cat(wrong[0]["policy"]["params"]) - ref).max() >= 5 * TOL, (k, j)
            assert np.abs(wrong[1][:, 0] - y[1][:, 0]).max() >= 5 * TOL


# ------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("cost", (False, True), ids=("lsiq_h", "lsiq_hc"))
def test_the_schedule_is_the_references_call_order(cost):
    """The calls DeviceLSIQH / DeviceLSIQHC.update_Q_function issues on a logging iteration, recorded on stand-ins for the
    engine, the policy passes and the critics, against the reference's order written out from lsiq.py:33-112,
    lsiq_h.py:35-102 and lsiq_hc.py:23-88 (with _update_all_targets, which the device runs inside this call)."""
    import types
    from olympic_hip.iq import DeviceLSIQH, DeviceLSIQHC
    B, n_p, in_dim, A = 6, 3, 4, 2
    log = []
    z = torch.zeros

    class Net:
        def __init__(self, name):
            self.name, self.step, self.lr, self.tau, self.betas, self.eps, self.weight_decay = name, 0, 1e-3, 0.005, (0.9, 0.999), 1e-8, 0.0
            self.stand = self.target_stand = None
            self.param = self.exp_avg = self.exp_avg_sq = self.packed = self.target_param = self.target_packed = z(1)

        def _colstats(self, st):
            return None

        def predict_target(self, obs, act, update_stats=False):
            log.append(f"{self.name}_target(obs | {'act' if act is ACT else 'a_pi'}) stats={update_stats}")
            return z(len(obs), 1)

        def soft_update_target(self):
            log.append(f"{self.name} target update")
    ag = object.__new__(DeviceLSIQHC if cost else DeviceLSIQH)

    def iq_q_update(*a, **kw):
        log.append(f"K26 {kw['algo']} alpha={'0' if kw['alpha'] == 0.0 else 'alpha'} update_target={kw['update_target']} "
                   f"tau={kw['tau']}")
        return z(16, dtype=torch.float64)

    def policy_pass(x, eps, generator, want_log_prob=True):
        log.append(f"pi({'next_obs' if x is NXT or x.data_ptr() == NXT.data_ptr() else 'obs' if len(x) == B else 'obs[expert]'})")
        return PI_ACT[:len(x)], z(len(x))
    ag.eng = types.SimpleNamespace(iq_q_update=iq_q_update)
    ag.critic, ag.h_critic, ag.policy, ag.sw = Net("Q"), Net("H"), None, None
    ag._policy_pass, ag._workspace = policy_pass, lambda B: None
    ag._iter, ag.logging_iter, ag.use_target, ag.gamma, ag.log_alpha, ag.reg_mult = 1, 1, True, 0.99, float(np.log(0.2)), 2.0
    ag.plcy_loss_mode, ag.regularizer_mode, ag.treat_absorbing_states, ag.R_min, ag.R_max = "value", "exp_and_plcy", False, 0.0, 1.0
    ag.lossQ_type, ag.loss_mode_exp, ag.Q_exp_loss, ag.target_clipping, ag.Q_min, ag.Q_max = "iq_like", "fix", "MSE", True, -1.0, 1.0
    ag.clip_expert_entropy_to_policy_max, ag.max_H_policy_tau_up, ag.max_H_policy_tau_down = True, 1e-2, 1e-4
    ag.h_max_state, ag.H_tau, ag.H_loss_mode = z(2), 0.03, "Huber"
    OBS, NXT, ACT, PI_ACT = torch.ones(B, in_dim), torch.ones(B, in_dim) * 2, z(B, A), torch.ones(B, A)
    ag.update_Q_function(OBS, ACT, NXT, z(B), n_p)
    want = ["pi(next_obs)", "pi(obs[expert])", "pi(obs)",                 # get_targetV(next_obs), logging_loss, getV(obs)
            f"K26 lsiq alpha=0 update_target={not cost} tau=0.005",       # update_Q_parameters; LSIQ_H: Q's target in-call
            "pi(next_obs)"]                                               # update_H_function's own pass
    if cost:
        want += ["Q_target(obs | act) stats=True", "pi(obs)", "Q_target(obs | a_pi) stats=True"]     # Q_plcy, get_targetV(obs)
    want += [f"K26 lsiq_h alpha=alpha update_target=True tau={0.03 if cost else 0.005}"]           # the H step and its target
    if cost:
        want += ["Q target update"]                                       # _update_all_targets, after H read the old target
    assert log == want, log
