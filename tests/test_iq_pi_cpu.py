"""K27 without a GPU: the C ABI entries of oly_iq_pi_* and oly_iq_alpha_update, the float64 restatement of
tests/iq_pi_restate.py against the three reference-run fixtures of tests/golden/gen_iq_pi_update.py (and the two wrong
readings, which must miss them), the sweep's table held to its purpose, the argument checks and the update schedule of
DeviceIQSAC / DeviceSQILSAC on CPU tensors."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import iq_pi_restate as R
import iq_restate as Q
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = R.TOL
K27_ENTRIES = ("oly_iq_pi_ws", "oly_iq_pi_ws_values", "oly_iq_pi_update", "oly_iq_alpha_update")
FIXTURES = ("iq", "iq_own_states_alpha", "sqil")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_declares_the_k27_entry_points():
    raw = _header()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in K27_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    # additive: the new declarations lie after oly_iq_q_update and before the measurement helpers
    last_k26 = txt.index("oly_iq_q_update(")
    helpers = txt.index("oly_event_create(")
    for name in K27_ENTRIES + ("oly_iq_pi;", "oly_iq_alpha;"):
        at = txt.index(name)
        assert last_k26 < at < helpers, name
    k27 = raw[raw.index("K27 :"):]
    for cite in ("iq_sac.py:408-419", ":431-465", ":587-595", "sqil_sac.py:16-62", "networks.py:88-160", "[Bp, Bp]"):
        assert cite in k27, cite
    assert _abi.IQ_PI_TAGS[:2] == R.PI_TAGS


@pytest.mark.parametrize("cls,ctype", ((_abi.IQPi, "oly_iq_pi"), (_abi.IQAlpha, "oly_iq_alpha")))
def test_struct_layout_matches_the_header(tmp_path, cls, ctype):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             f'printf("size %zu\\n", sizeof({ctype}));']
    lines += [f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f, _ in cls._fields_]
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
    sizes = [int(L.oly_iq_pi_ws(b, 32, 11)) for b in (1, 16, 17, 64, 512, 4096)]
    assert sizes[0] == sizes[1] > 0 and all(a < b for a, b in zip(sizes[1:], sizes[2:]))
    assert int(L.oly_iq_pi_ws(64, 1, 1)) == int(L.oly_iq_pi_ws(64, 48, 16)) == sizes[3]
    # per row: 64 + 512 + 256 activations, 512 + 256 + 32 deltas; three transposed streams
    assert sizes[1] >= 16 * 1632 + 2 * 256 * 512 + 32 * 256 and sizes[5] >= 4096 * 1632 + 2 * 256 * 512 + 32 * 256
    for b in (1, 18, 4096):
        off = int(L.oly_iq_pi_ws_values(b, 12, 5))
        assert 0 < off and off + (b + 15) // 16 * 16 <= int(L.oly_iq_pi_ws(b, 12, 5))
    for bad in ((0, 12, 5), (-1, 12, 5), (4097, 12, 5), (18, 0, 5), (18, 12, 0), (18, 12, 17), (18, 60, 5), (18, 64, 1)):
        assert int(L.oly_iq_pi_ws(*bad)) == -1, bad
        assert int(L.oly_iq_pi_ws_values(*bad)) == -1, bad
    # a NULL context is refused before anything is read
    assert L.oly_iq_pi_update(None, None, None) == _abi.OLY_EINVAL
    assert L.oly_iq_pi_update(None, ctypes.byref(_abi.IQPi()), None) == _abi.OLY_EINVAL
    assert L.oly_iq_alpha_update(None, ctypes.byref(_abi.IQAlpha()), None) == _abi.OLY_EINVAL


# ------------------------------------------------------------------------------ the restatement against the reference runs
_RUNS = {}


def fixture_run(g, name, wrong=None, dtype=torch.float64):
    """The twin over the fixture's four iq_updates, computed once per (fixture, reading, dtype) and left unchanged."""
    import gen_iq_pi_update as gen
    if (name, wrong, dtype) in _RUNS:
        return _RUNS[(name, wrong, dtype)], gen
    spec = gen.FIXTURES[name]
    qcfg = Q.Cfg(algo=spec["algo"], mode=spec["mode"], reg=spec["reg"], treat=False, use_target=spec["use_target"],
                 standardizer=True, gamma=float(g["gamma"]), reg_mult=float(g["reg_mult"]), R_min=0.0, R_max=1.0,
                 lr=float(g["lr"]), tau=float(g["tau"]))
    cfg = R.PiCfg(standardizer=True, lr=float(g["lr_actor"]), own_states=spec["own_states"], learnable=spec["learnable"],
                  lr_alpha=float(g["lr_alpha"]), init_alpha=gen.gq.INIT_ALPHA, ls_min=gen.gq.LOG_STD_MIN,
                  ls_max=gen.gq.LOG_STD_MAX, target_entropy=float(g["target_entropy"]))
    pinit = [gen.gq.w2_init(11) if n == "w2" else g[f"policy_init_{n}"] for n in R.NAMES]
    cinit = [gen.gq.w2_init(12) if n == "w2" else g[f"critic_init_{n}"] for n in R.NAMES]
    central = (0.5 * (g["max_a"] + g["min_a"])).astype(np.float32)
    delta = (0.5 * (g["max_a"] - g["min_a"])).astype(np.float32)
    t = R.Twin(pinit, cinit, central, delta, cfg, qcfg=qcfg, dtype=dtype, wrong=wrong)
    for i in range(gen.N_ITER):
        t.iq_update({k: g[k][i] for k in ("obs", "act", "next_obs", "absorbing")}, int(g["n_policy"]),
                    dict(next=g["eps_next"][i], pi=g["eps_pi"][i], expert=g["eps_expert"][i], ppi=g["eps_ppi"][i],
                         plog=g["eps_plog"][i]))
    _RUNS[(name, wrong, dtype)] = t
    return t, gen


def fixture_miss(g, params, gen, prefix):
    """The largest distance of restated parameters from the stored ones (layer 2: its stored rows)."""
    worst = 0.0
    for n, a in zip(R.NAMES, params):
        r = g[f"{prefix}_w2_head"] if n == "w2" else g[f"{prefix}_{n}"]
        worst = max(worst, float(np.abs((a[:gen.W2_HEAD] if n == "w2" else a) - r).max()))
    return worst


def stats_ok(got, want, spread):
    return np.array_equal(got[0], want[0]) and \
        bool(np.all(np.abs(got - want) <= np.maximum(TOL * np.maximum(1.0, np.abs(want)), 4 * spread)))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_reference_run(golden, name):
    g = golden(f"iq_pi_update/{name}.npz")
    t, gen = fixture_run(g, name)
    st = t.state()
    tol_p, tol_c = max(TOL, 4 * float(g["spread_policy"])), max(TOL, 4 * float(g["spread_critic"]))
    err_p = fixture_miss(g, st["policy"]["params"], gen, "policy")
    err_c = fixture_miss(g, st["critic"]["params"], gen, "critic")
    print(f"{name}: policy {err_p:.3e} (tolerance {tol_p:.3e}), critic {err_c:.3e} ({tol_c:.3e})")
    assert err_p <= tol_p and err_c <= tol_c
    assert float(g["spread_policy"]) <= 1e-5 and float(g["spread_critic"]) <= 1e-5
    scal = g["scalars"]
    got = np.array([[t.scalars[i + 1][k] for k in gen.ACTOR_TAGS] for i in range(gen.N_ITER)])
    assert np.isfinite(scal).all()                      # every iteration logs every Actor/... scalar
    assert np.all(np.abs(got - scal) <= np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * float(g["spread_scalars"])))
    assert stats_ok(st["critic"]["colstats"], g["colstats"], float(g["spread_critic_stats"]))
    assert stats_ok(st["policy"]["colstats"], g["policy_colstats"], float(g["spread_policy_stats"]))
    assert R.alpha_err(st["alpha"], g["alpha_block"]) <= max(TOL, 4 * float(g["spread_alpha"]))
    # The row counts.  The critic's live Standardizer: two passes of the critic update (a target) and the policy update's
    # Bp rows.  The policy's: next_obs, the expert rows, obs, then update_policy's Bp, its logging pass on all rows and
    # get_mu_log_sigma on the two halves.
    spec, B, n_p = gen.FIXTURES[name], gen.B, gen.N_POLICY
    Bp = n_p if spec["own_states"] else B
    assert g["colstats"][0, 0] == gen.N_ITER * (2 * B + Bp)
    assert g["policy_colstats"][0, 0] == gen.N_ITER * (2 * B + (B - n_p) + Bp + B + n_p + (B - n_p))
    # the entropy lower bound is a host number from policy.iter
    assert np.allclose(scal[:, gen.ACTOR_TAGS.index("Actor/Entropy Lower Bound")], 2.0 - 1e-5 * np.arange(gen.N_ITER), atol=0)
    if spec["learnable"]:
        assert abs(g["alpha_block"][0] - np.log(gen.gq.INIT_ALPHA)) > 1e-4 and g["alpha_block"][2] > 0
    else:
        assert float(np.float32(g["alpha_block"][0])) == float(np.float32(np.log(gen.gq.INIT_ALPHA)))
        assert tuple(g["alpha_block"][1:]) == (0.0, 0.0)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_wrong_readings_miss_the_reference_run(golden, name):
    g = golden(f"iq_pi_update/{name}.npz")
    import gen_iq_pi_update as gen
    tol_p = max(TOL, 4 * float(g["spread_policy"]))
    w, _ = fixture_run(g, name, wrong="critic_stats_untouched")
    st = w.state()
    assert not stats_ok(st["critic"]["colstats"], g["colstats"], float(g["spread_critic_stats"]))
    miss = fixture_miss(g, st["policy"]["params"], gen, "policy")
    print(f"{name} critic_stats_untouched: misses the stored policy by {miss / tol_p:.1f} tolerances")
    assert miss > 10 * tol_p and float(g["miss_critic_stats_untouched_params"]) > 10 * tol_p
    assert float(g["miss_critic_stats_untouched_stats"]) > 10 * max(TOL, 4 * float(g["spread_critic_stats"]))
    tol_a = max(TOL, 4 * float(g["spread_alpha"]))
    w, _ = fixture_run(g, name, wrong="alpha_from_first_pass")
    miss = R.alpha_err(w.state()["alpha"], g["alpha_block"])
    if gen.FIXTURES[name]["learnable"]:
        print(f"{name} alpha_from_first_pass: misses the stored alpha block by {miss / tol_a:.1f} tolerances")
        assert miss > 10 * tol_a and float(g["miss_alpha_from_first_pass"]) > 10 * tol_a
    else:
        assert miss <= tol_a and float(g["miss_alpha_from_first_pass"]) == 0.0     # alpha never steps


def test_float32_restatement_of_a_fixture_lies_within_its_spread(golden):
    g = golden("iq_pi_update/iq.npz")
    t, gen = fixture_run(g, "iq", dtype=torch.float32)
    assert fixture_miss(g, t.state()["policy"]["params"], gen, "policy") <= max(TOL, 4 * float(g["spread_policy"]))


def test_the_broadcast_loss_equals_the_row_wise_one():
    """mean over [Bp, Bp] of alpha log_prob[j] - q[i] is mean(alpha log_prob) - mean(q), and so is its gradient."""
    rng = np.random.default_rng(0)
    lp = torch.tensor(rng.standard_normal(9), requires_grad=True)
    q = torch.tensor(rng.standard_normal((9, 1)), requires_grad=True)
    a = (0.3 * lp - q).mean()
    b = (0.3 * lp - q.reshape(-1)).mean()
    ga, gb = torch.autograd.grad(a, (lp, q)), torch.autograd.grad(b, (lp, q))
    assert tuple((0.3 * lp - q).shape) == (9, 9) and abs(float((a - b).detach())) < 1e-15
    assert all(float((x - y).abs().max()) < 1e-15 for x, y in zip(ga, gb))


def test_alpha_adam_is_torchs_scalar_adam():
    lps = [np.array([-3.0, 1.0], np.float32), np.array([0.5, -0.5], np.float32)]
    got = R.alpha_adam(lps, -2.0, 1e-3, init=0.5)
    # by hand: g = -exp(la) mean(lp + te); Adam with bias corrections
    la, m, v = float(np.float32(np.log(0.5))), 0.0, 0.0
    for s, lp in enumerate(lps, 1):
        gr = -np.exp(la) * float(np.mean(lp.astype(np.float64) - 2.0))
        m, v = 0.9 * m + 0.1 * gr, 0.999 * v + 0.001 * gr * gr
        la -= 1e-3 / (1 - 0.9 ** s) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** s) + 1e-8)
    assert np.allclose(got, [la, m, v], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------ the sweep's table
def test_the_sweep_is_held_to_its_purpose():
    assert R.SHAPES == ((1, 1, 1), (12, 5, 18), (16, 16, 16), (32, 11, 48), (48, 16, 33)) and R.UPDATES == 3
    bps = [s[2] for s in R.SHAPES]
    assert 1 in bps and any(b % 16 == 0 for b in bps) and any(b > 16 and b % 16 for b in bps)
    assert {c.standardizer for c in R.CONFIGS} == {True, False} and any(c.wd > 0 for c in R.CONFIGS)
    assert all(c.adam_eps == R.SWEEP_EPS == 1e-5 for c in R.CONFIGS)          # as tests/iq_restate.py's sweep; see there
    facts = [R.sweep_facts(k, j) for k in range(len(R.SHAPES)) for j in range(len(R.CONFIGS))]
    assert sum(f["clamped"] for f in facts) > 0 and sum(f["unclamped"] for f in facts) > 0
    assert any(f["dead_policy"] > 0 for f in facts) and any(f["dead_critic"] > 0 for f in facts)
    for k in range(1, len(R.SHAPES)):      # every shape with more than one action column has both kinds
        assert all(R.sweep_facts(k, j)["clamped"] > 0 and R.sweep_facts(k, j)["unclamped"] > 0 for j in range(len(R.CONFIGS)))


@pytest.mark.parametrize("k", range(len(R.SHAPES)), ids=["-".join(map(str, s)) for s in R.SHAPES])
def test_every_case_of_the_sweep_is_one_float32_can_hold(k):
    """torch's own float32 run lies within 5e-6 (TOL / 4, which leaves room for another summation order) of float64 on
    the parameters at every config, and every weight tensor moves by 10 TOL."""
    case = R.sweep_inputs(k)
    for j, cfg in enumerate(R.CONFIGS):
        ref, ref_out, _, f32, f32_out, _ = R.yardstick(k, j)
        spread = float(np.abs(R.cat(f32["policy"]["params"]) - R.cat(ref["policy"]["params"])).max())
        print(f"{R.SHAPES[k]} {R.cfg_id(cfg)}: float32 spread {spread:.3e}")
        assert spread <= 5e-6, (R.cfg_id(cfg), spread)
        for name, p0, p1 in zip(R.NAMES, case["pparams"], ref["policy"]["params"]):
            assert float(np.abs(p1 - p0.astype(np.float64)).max()) >= 10 * TOL, (j, name)
        assert np.isfinite(ref_out).all()
        # the critic does not step in a policy update
        assert all(np.array_equal(a, np.asarray(b, np.float64)) for a, b in zip(ref["critic"]["params"], case["cparams"]))


# ------------------------------------------------------------------------------ the module's argument checks and schedule
def _fake_engine():
    return types.SimpleNamespace(device=torch.device("cpu"))


def _policy(in_dim=12, act_dim=5):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy as P
    pol = object.__new__(P)
    pol.in_dim, pol.act_dim, pol.stand = in_dim, act_dim, None
    pol.param = torch.zeros(7)
    return pol


def _critic(D=17):
    from olympic_hip.iq import DeviceSoftQCritic as C
    c = object.__new__(C)
    c.D = D
    return c


def _demo(n=6, in_dim=12, A=5):
    return dict(states=np.zeros((n, in_dim)), actions=np.zeros((n, A)), next_states=np.zeros((n, in_dim)),
                absorbing=np.zeros(n))


def _mk(cls=None, **kw):
    from olympic_hip.iq import DeviceIQSAC
    return (cls or DeviceIQSAC)(_fake_engine(), _policy(), _critic(), _demo(), 0.99, 8, True, **kw)


def test_constructor_refusals_and_defaults():
    import olympic_hip
    from olympic_hip._ffi import OlyError
    from olympic_hip.iq import FOLLOW_UP, DeviceIQLearn, DeviceIQSAC, DeviceSQIL, DeviceSQILSAC
    assert issubclass(DeviceIQSAC, DeviceIQLearn) and issubclass(DeviceSQILSAC, DeviceSQIL)
    assert olympic_hip.DeviceIQSAC is DeviceIQSAC and olympic_hip.DeviceSQILSAC is DeviceSQILSAC
    assert FOLLOW_UP == ("the policy side of the SAC family (update_policy, _update_alpha) is the follow-up to the critic "
                         "update")
    for cls in (DeviceIQSAC, DeviceSQILSAC):
        with pytest.raises(OlyError, match="clipping"):
            _mk(cls, actor_optimizer=dict(lr=1e-3, clipping=dict(max_norm=1.0)))
        with pytest.raises(OlyError, match="unknown entries"):
            _mk(cls, actor_optimizer=dict(lr=1e-3, amsgrad=True))
        with pytest.raises(OlyError, match="gradient_penalty"):
            _mk(cls, gradient_penalty_lambda=0.1)
        with pytest.raises(OlyError, match="delay_pi"):
            _mk(cls, delay_pi=0)
        with pytest.raises(OlyError, match="warmup_transitions"):
            _mk(cls, warmup_transitions=-1)
    with pytest.raises(OlyError, match="v0"):
        _mk(plcy_loss_mode="v0")
    # the critic-side classes still refuse a learnable temperature, naming the follow-up
    for cls in (DeviceIQLearn, DeviceSQIL):
        with pytest.raises(OlyError, match="learnable_alpha") as e:
            cls(_fake_engine(), _policy(), _critic(), _demo(), 0.99, 8, True, learnable_alpha=True)
        assert FOLLOW_UP in str(e.value)
    a = _mk()
    assert (a.delay_pi, a.warmup_transitions, a.train_policy_only_on_own_states, a.learnable_alpha) == (1, 0, False, False)
    assert (a.pi_lr, a.pi_betas, a.pi_eps, a.pi_weight_decay) == (3e-4, (0.9, 0.999), 1e-8, 0.0)
    assert a.target_entropy == -5.0 and a.pi_step == 0 and a.alpha_step == 0 and a.KIND == "iq_sac"
    assert torch.equal(a.alpha_state, torch.tensor([np.float32(np.log(1e-3)), 0.0, 0.0]))
    assert abs(a.alpha - 1e-3) < 1e-9 and a.get_e_lb() == 2.0
    assert tuple(a.pi_exp_avg.shape) == tuple(a.pi_exp_avg_sq.shape) == (7,)
    s = _mk(DeviceSQILSAC, learnable_alpha=True, lr_alpha=1e-3, target_entropy=-3.0, init_alpha=0.5, R_min=-1.0,
            actor_optimizer=dict(lr=1e-3, betas=(0.8, 0.9), eps=1e-6, weight_decay=1e-4))
    assert (s.learnable_alpha, s.lr_alpha, s.target_entropy, s.R_min, s.KIND) == (True, 1e-3, -3.0, -1.0, "sqil_sac")
    assert (s.pi_lr, s.pi_betas, s.pi_eps, s.pi_weight_decay) == (1e-3, (0.8, 0.9), 1e-6, 1e-4)
    # a learnable alpha is read back from the block, once after each step of it
    assert abs(s.alpha - 0.5) < 1e-7
    s.alpha_state[0] = float(np.log(0.25))
    assert abs(s.alpha - 0.5) < 1e-7               # no step was taken: the host copy stands
    s._alpha_read = False
    assert abs(s.alpha - 0.25) < 1e-7 and s._alpha_read


def test_the_schedule_follows_iq_update(monkeypatch):
    """update_Q_function when _iter % delay_Q == 0; update_policy when replay.size > warmup_transitions and
    _iter % delay_pi == 0 (iq_sac.py:408-419), against those conditions restated in plain Python."""
    for delay_Q, delay_pi, warm in ((1, 1, 0), (2, 3, 5), (3, 1, 12), (1, 2, 4)):
        a = _mk(delay_Q=delay_Q, delay_pi=delay_pi, warmup_transitions=warm, max_replay_size=64)
        calls = []
        a.update_Q_function = lambda *x, **k: calls.append(("q", a._iter))
        a.update_policy = lambda *x, **k: calls.append(("pi", a._iter))
        want, size = [], 0
        for it in range(1, 14):
            size = min(64, size + 2)
            a.replay._idx = size
            assert a.replay.size == size
            a.iq_update(None, None, None, None, 4)
            if it % delay_Q == 0:
                want.append(("q", it))
            if size > warm and it % delay_pi == 0:
                want.append(("pi", it))
            a._iter += 1
        assert calls == want, (delay_Q, delay_pi, warm)
        assert any(c[0] == "pi" for c in calls) and any(c[0] == "q" for c in calls)


def test_state_dict_carries_the_policy_side():
    a = _mk(learnable_alpha=True)
    from olympic_hip.iq import _PolicySide
    assert {"state_dict", "load_state_dict", "update_policy", "iq_update", "fit", "alpha"} <= set(vars(_PolicySide))
    assert hasattr(a, "fit_Q")                        # the critic-side loop stays
