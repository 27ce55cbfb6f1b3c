"""K26's third algorithm on the MI355X: oly_iq_q_update with OLY_IQ_ALGO_LSIQ against the float64 restatement of
tests/lsiq_restate.py over iq_restate's shapes and every expert loss x clipping x target, its bits (equal to algo "iq"
where LSIQ coincides with IQ, across runs), the four reference-run fixtures through DeviceLSIQ, a DeviceLSIQSAC.fit run
against iq_pi_restate's twin, fenced and poisoned operands, the refusals, and checkpoint / resume.

Tolerances are test_gpu_iq_q.py's: 4 x the float32-against-float64 spread of the same update, never below TOL = 2e-5.
For a fixture the spread is the stored one; for a case of the sweep it is measured by running the restatement in float32
as well.  lsiq_restate.yardstick asserts the margins of every case's float64 run (no next_v within 1e-3 of a clip bound,
no Huber residual within 1e-3 of its kink, no pre-activation within 1e-6 of a relu's, two rows of every kind from
B = 16)."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import torch

import iq_pi_restate as P
import iq_restate as R
import lsiq_restate as L
from fences import Fenced, assert_untouched, assert_written, fenced
from test_gpu_iq_q import Dev, Recorder, split

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, SHAPES, cat = L.TOL, L.SHAPES, L.cat
FIXTURES = ("iq_fix", "iq_bootstrap", "sqil_value_plcy", "sqil_fix_value")


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def same_bits(a, b):
    """Two snapshots of a buffer hold the same bytes (a poisoned buffer is NaN all over, which torch.equal tells apart)."""
    return (a is None and b is None) or torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def block_of(c):
    return dict(lossQ_type=c.type, loss_mode_exp=c.exp_mode, Q_exp_loss=c.exp_loss, target_clipping=c.clip, Q_min=c.q_min,
                Q_max=c.q_max)


class LDev(Dev):
    """test_gpu_iq_q.py's fenced critic state with LSIQ's call: every input of a step is fenced at exactly the rows the
    step holds (a_pi / logp_pi at n_policy rows for sqil_like / value_plcy); a None input is passed as None."""

    def update(self, s, n_policy, **over):
        c = self.cfg
        self.inputs = {k: fenced(np.asarray(v, np.float32)) for k, v in s.items() if v is not None}
        i = {k: v.t for k, v in self.inputs.items()}
        kw = dict(algo="lsiq", plcy_loss_mode=c.mode, regularizer_mode=c.reg, treat_absorbing=c.treat,
                  use_target=c.use_target, update_target=c.update_target, gamma=c.gamma, alpha=c.alpha, reg_mult=c.reg_mult,
                  tau=c.tau, weight_decay=c.wd, eps=c.adam_eps, lsiq=block_of(c))
        kw.update(over)
        self.eng.iq_q_update(i["obs"], i["act"], i["next_obs"], i["absorbing"], i["a_next"], i["logp_next"], i.get("a_pi"),
                             i.get("logp_pi"), n_policy, self.t("colstats"), self.t("target_colstats"), self.t("param"),
                             self.t("m"), self.t("v"), self.t("packed"), self.t("target_param"), self.t("target_packed"),
                             self.t("ws"), self.step, c.lr, out=self.t("out"), **kw)
        self.step += 1
        return self.t("out").clone()


# ------------------------------------------------------------------------------ against the float64 yardstick
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["-".join(map(str, s)) for s in SHAPES])
def test_update_against_float64(eng, k):
    """Shape k with the configs tests/lsiq_restate.py gives it: over the five shapes every expert loss x clipping x target,
    every iq_like mode and regularizer and every sqil_like mode is run, with and without Standardizers and
    treat_absorbing_states."""
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = L.sweep_inputs(k)
    assert L.sweep(k)
    for j, cfg in L.sweep(k):
        ref, ref_out, f32, f32_out = L.yardstick(k, j)
        dev = LDev(eng, params, cfg, in_dim, A, B)
        out = np.stack([dev.update(s, n_policy).cpu().numpy() for s in L.case_steps(cfg, steps, n_policy)])
        got = dev.snapshot()
        dev.check_fences(L.cfg_id(cfg))
        who = f"{SHAPES[k]} {L.cfg_id(cfg)}"
        for key, rk in (("param", "params"), ("target_param", "target")):
            spread = float(np.abs(cat(f32[rk]) - cat(ref[rk])).max())
            err = float(np.abs(got[key].double().cpu().numpy() - cat(ref[rk])).max())
            print(f"{who} {key}: |kernel - f64| max {err:.3e} (float32 spread {spread:.3e})")
            assert err <= max(TOL, 4 * spread), (who, key, err, spread)
        for key, rk in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            r = cat(ref[rk])
            scale = max(float(np.abs(r).max()), 1e-300)
            spread = float(np.abs(cat(f32[rk]) - r).max()) / scale
            err = float(np.abs(got[key].double().cpu().numpy() - r).max()) / scale
            print(f"{who} {key}: relative to the largest entry {err:.3e} (spread {spread:.3e})")
            assert err <= max(TOL, 4 * spread), (who, key, err, spread)
        if cfg.standardizer:
            for key, rk in (("colstats", "colstats"), ("target_colstats", "tcolstats")):
                a, r = got[key].cpu().numpy(), ref[rk]
                assert np.array_equal(a[0], r[0]), (who, key, "counts", a[0, 0], r[0, 0])
                assert np.all(np.abs(a - r) <= 1e-12 * np.maximum(1.0, np.abs(r))), (who, key)
        spread = np.abs(f32_out - ref_out)
        tol = np.maximum(TOL * np.maximum(1.0, np.abs(ref_out)), 4 * np.where(np.isnan(spread), 0.0, spread))
        assert np.array_equal(np.isnan(out), np.isnan(ref_out)), (who, out, ref_out)
        bad = ~(np.abs(out - ref_out) <= tol) & ~np.isnan(ref_out)
        print(f"{who} scalars: worst |kernel - f64| / tolerance {np.nanmax(np.abs(out - ref_out) / tol):.3f}")
        assert not bad.any(), (who, np.argwhere(bad), out[bad], ref_out[bad])
        assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim + A)))
        assert torch.equal(got["target_packed"], eng.ilmlp_pack(*split(got["target_param"], in_dim + A)))


def test_sqil_like_value_is_refused_at_unequal_halves(eng):
    from olympic_hip._ffi import OlyError
    k = L.UNBALANCED
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = L.sweep_inputs(k)
    cfg = L.LCfg(type="sqil_like", exp_loss="MSE", mode="value", q_min=L.Q_MIN, q_max=L.Q_MAX)
    dev = LDev(eng, params, cfg, in_dim, A, B)
    before = dev.snapshot()
    with pytest.raises(OlyError):
        dev.update(steps[0], n_policy)
    after = dev.snapshot()
    for key, a in before.items():
        assert same_bits(a, after[key]), key
    assert dev.f["out"].unwritten() == 16


# ------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("use_target", (True, False), ids=("tgt", "notgt"))
def test_bits_equal_to_iq_where_lsiq_coincides_with_it(eng, use_target):
    """iq_like with bootstrap and no clipping is IQ: after 3 updates the parameters, moments, both streams, both
    statistics and out hold the bits algo "iq" leaves with the same mode and regularizer."""
    k = 1
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = L.sweep_inputs(k)
    for i, mode in enumerate(R.IQ_MODES):
        for reg in (R.REG_MODES[i], R.REG_MODES[(i + 2) % 4]):
            cfg = L.LCfg(type="iq_like", exp_mode="bootstrap", exp_loss=None, clip=False, mode=mode, reg=reg, treat=bool(i % 2),
                         use_target=use_target, tau=0.05, wd=1e-4, q_min=L.Q_MIN, q_max=L.Q_MAX)
            assert L.as_iq(cfg) is not None
            snaps = []
            for over in (dict(), dict(algo="iq", lsiq=None)):
                dev = LDev(eng, params, cfg, in_dim, A, B)
                outs = torch.stack([dev.update(s, n_policy, **over) for s in steps])
                snaps.append((dev.snapshot(), outs))
            for key, a in snaps[0][0].items():
                assert torch.equal(a, snaps[1][0][key]), (mode, reg, key)
            assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64)), (mode, reg)


def test_two_runs_give_the_same_bits(eng):
    k = 3
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = L.sweep_inputs(k)
    base = L.LCfg(q_min=L.Q_MIN, q_max=L.Q_MAX, wd=1e-4)
    for cfg in (base._replace(exp_loss="Huber", use_target=False, mode="value_q_old_policy"),
                base._replace(type="sqil_like", exp_mode="bootstrap", exp_loss="Huber", mode="value_plcy", treat=True,
                              reg_mult=2.0)):
        snaps = []
        for _ in range(2):
            dev = LDev(eng, params, cfg, in_dim, A, B)
            outs = [dev.update(s, n_policy) for s in L.case_steps(cfg, steps, n_policy)]
            snaps.append((dev.snapshot(), torch.stack(outs)))
        for key, a in snaps[0][0].items():
            assert a is None or torch.equal(a, snaps[1][0][key]), key
        assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))


# ------------------------------------------------------------------------------ the reference-run fixtures
def build_agent(eng, g, name, sw=None, logging_iter=1, sac=False, **more):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceLSIQ, DeviceLSIQSAC, DeviceSoftQCritic
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_lsiq_q_update as gen

    def lins(prefix, dims, seed):
        out = [torch.nn.Linear(i, o) for i, o in dims]
        with torch.no_grad():
            for lin, (w, b) in zip(out, (("w1", "b1"), ("w2", "b2"), ("w3", "b3"))):
                lin.weight.copy_(torch.as_tensor(gen.w2_init(seed) if w == "w2" else g[f"{prefix}_{w}"]))
                lin.bias.copy_(torch.as_tensor(g[f"{prefix}_{b}"]))
        return out
    A, in_dim, D = gen.ACT_DIM, gen.IN_DIM, gen.D
    policy = DeviceSquashedGaussianPolicy(eng, lins("policy_init", [(in_dim, 512), (512, 256), (256, 2 * A)], 11), g["min_a"],
                                          g["max_a"], standardizer=DeviceStandardizer(eng, in_dim),
                                          log_std_min=gen.G.LOG_STD_MIN, log_std_max=gen.G.LOG_STD_MAX)
    critic = DeviceSoftQCritic(eng, lins("critic_init", [(D, 512), (512, 256), (256, 1)], 12),
                               standardizer=DeviceStandardizer(eng, D), lr=float(g["lr"]), tau=float(g["tau"]))
    demo = dict(states=np.zeros((4, in_dim), np.float32), actions=np.zeros((4, A), np.float32),
                next_states=np.zeros((4, in_dim), np.float32), absorbing=np.zeros(4, np.float32))
    spec = gen.FIXTURES[name]
    kw = dict(gamma=float(g["gamma"]), batch_size=gen.N_POLICY, use_target=spec["use_target"], init_alpha=gen.INIT_ALPHA,
              reg_mult=float(g["reg_mult"]), plcy_loss_mode=spec["mode"], regularizer_mode=spec["reg"],
              logging_iter=logging_iter, sw=sw, max_replay_size=64, Q_max=float(g["Q_max"]), Q_min=float(g["Q_min"]),
              loss_mode_exp=spec["exp_mode"], Q_exp_loss=spec["exp_loss"], treat_absorbing_states=spec["treat"],
              target_clipping=spec["clip"], lossQ_type=spec["type"])
    kw.update(more)
    return (DeviceLSIQSAC if sac else DeviceLSIQ)(eng, policy, critic, demo, **kw), gen


def run_fixture(agent, g, first, last):
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    outs = []
    for i in range(first, last):
        eps = dict(next=d(g["eps_next"][i]), pi=d(g["eps_pi"][i]), expert=d(g["eps_expert"][i]))
        outs.append(agent.update_Q_function(d(g["obs"][i]), d(g["act"][i]), d(g["next_obs"][i]), d(g["absorbing"][i]),
                                            int(g["n_policy"]), eps=eps))
        agent._iter += 1
    return outs


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_the_agent(eng, golden, name):
    from olympic_hip import _abi
    g = golden(f"lsiq_q_update/{name}.npz")
    sw = Recorder()
    agent, gen = build_agent(eng, g, name, sw=sw)
    spec = gen.FIXTURES[name]
    outs = run_fixture(agent, g, 0, gen.N_ITER)
    torch.cuda.synchronize()
    c = agent.critic
    tol_p, tol_t = max(TOL, 4 * float(g["spread_params"])), max(TOL, 4 * float(g["spread_target"]))
    for flat, prefix, tol in ((c.param, "critic", tol_p), (c.target_param, "target", tol_t)):
        got = dict(zip(R.NAMES, split(flat.double().cpu().numpy(), gen.D)))
        for n in R.NAMES:
            a, r = (got[n][:gen.W2_HEAD], g[f"{prefix}_w2_head"]) if n == "w2" else (got[n], g[f"{prefix}_{n}"])
            err = float(np.abs(a - r).max())
            print(f"{name} {prefix} {n}: {err:.3e} (tolerance {tol:.3e})")
            assert err <= tol, (prefix, n, err)
    # the scalars the reference logged, from the device block and from the writer
    scal, sp = g["scalars"], float(g["spread_scalars"])
    out = np.stack([o.cpu().numpy() for o in outs])
    logged = ~np.isnan(scal)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * sp)
    assert np.all(np.abs(out - scal)[logged] <= tol[logged]), (np.abs(out - scal) / tol)
    if spec["type"] == "sqil_like":       # (loss_term1, loss_term2, 0.0) and no V scalar
        assert np.all(out[:, 2] == 0.0) and np.all(out[:, 3] == 0.0) and np.all(scal[:, 2] == 0.0)
    for i in range(gen.N_ITER):
        row = sw.rows[i + 1]
        for k, t in enumerate(_abi.IQ_Q_TAGS):
            assert (t in row) == bool(logged[i, k]) or t in ("Action-Value/Q Absorbing state exp",
                                                             "Action-Value/Q Absorbing state plcy"), (i, t)
            if logged[i, k]:
                assert row[t] == out[i, k]
        assert "IQ-Loss/Alpha" in row
        for k, t in enumerate(gen.ACTION_TAGS):
            assert abs(row[t] - g["action_scalars"][i, k]) <= TOL * max(1.0, abs(g["action_scalars"][i, k])), (i, t)
    # the Standardizers: counts exact, sums within TOL of their own size or 4 x the stored spread (test_gpu_iq_q.py)
    st_tol = lambda r: np.maximum(TOL * np.maximum(1.0, np.abs(r)), 4 * float(g["spread_stats"]))
    for got, want in ((agent.policy.stand.colstats, g["policy_colstats"]), (c.stand.colstats, g["colstats"]),
                      (c.target_stand.colstats, g["target_colstats"])):
        a = got.cpu().numpy()
        assert np.array_equal(a[0], want[0]), (a[0], want[0])
        assert np.all(np.abs(a - want) <= st_tol(want))


# ------------------------------------------------------------------------------ the whole agent
class LTwin(P.Twin):
    """iq_pi_restate's Twin with LSIQ's critic update in place of IQ's: the policy passes of the critic update in the
    order of the loss type, the rest (update_policy, the counters) inherited."""

    def __init__(self, pparams, cparams, central, delta, cfg, lcfg, dtype=torch.float64, check=False):
        super().__init__(pparams, cparams, central, delta, cfg, dtype=dtype)
        self.q = L.LSIQSoftQ(cparams, lcfg, dtype, check=check)

    def iq_update(self, s, n_policy, eps, logging=True):
        c = self.q.cfg = self.q.cfg._replace(alpha=float(self.alpha))
        obs = s["obs"]
        f = lambda t: t.detach().to(torch.float32).numpy()
        before = c.type == "iq_like"
        with torch.no_grad():
            a_next, lp_next = (f(t) for t in self.pi.act(s["next_obs"], eps["next"]))
            a_pi = lp_pi = None
            if logging and before:
                self.pi.act(obs[n_policy:], eps["expert"])
            if L.has_v(c):
                a_pi, lp_pi = (f(t) for t in self.pi.act(obs[:L.value_rows(c, len(obs), n_policy)], eps["pi"]))
            if logging and not before:
                self.pi.act(obs[n_policy:], eps["expert"])
        out_q = self.q.update(obs, s["act"], s["next_obs"], s["absorbing"], a_next, lp_next, a_pi, lp_pi, n_policy)
        out_pi = self.update_policy(obs, n_policy, dict(pi=eps["ppi"], log=eps.get("plog")), logging)
        self.iter += 1
        self.pi.iter += 1
        return out_q, out_pi


@pytest.mark.parametrize("typ,mode", (("iq_like", "value"), ("sqil_like", "value_plcy")))
def test_a_fit_run_of_the_whole_agent_against_the_twin(eng, typ, mode):
    """DeviceLSIQSAC.fit for three iterations (the dataset into the replay memory, a batch drawn from it and from the
    demonstrations, iq_update, the counters) against iq_pi_restate's twin with LSIQ's critic update.  fit draws its
    batches on the device, so iq_update is wrapped: it records the batch it was given and supplies the noise."""
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceLSIQSAC, DeviceSoftQCritic
    in_dim, A, n_b, n_iter = 12, 5, 9, 3
    B, D = 2 * n_b, in_dim + A
    case = P.case_inputs(in_dim, A, B, seed=31)
    pcfg = P.PiCfg(standardizer=True, adam_eps=P.SWEEP_EPS, ls_min=P.SWEEP_LS[0], ls_max=P.SWEEP_LS[1], lr=L.SWEEP_LR)
    cparams = [np.asarray(p, np.float32).copy() for p in case["cparams"]]
    cparams[4] *= np.float32(L.W3_SCALE)
    cparams[5] *= np.float32(L.W3_SCALE)
    lcfg = L.LCfg(type=typ, exp_mode="fix" if typ == "iq_like" else "bootstrap", exp_loss="Huber", mode=mode,
                  treat=typ == "sqil_like", reg_mult=0.5 if typ == "iq_like" else 2.0, q_min=L.Q_MIN, q_max=L.Q_MAX,
                  lr=L.SWEEP_LR, adam_eps=L.SWEEP_EPS, tau=0.05, alpha=float(np.exp(np.float32(np.log(P.ALPHA)))))

    def lins(params, dims):
        out = [torch.nn.Linear(i, o) for i, o in dims]
        with torch.no_grad():
            for j, lin in enumerate(out):
                lin.weight.copy_(torch.as_tensor(params[2 * j]))
                lin.bias.copy_(torch.as_tensor(params[2 * j + 1]))
        return out
    central, delta = case["central"].astype(np.float64), case["delta"].astype(np.float64)
    policy = DeviceSquashedGaussianPolicy(eng, lins(case["pparams"], [(in_dim, 512), (512, 256), (256, 2 * A)]),
                                          central - delta, central + delta, standardizer=DeviceStandardizer(eng, in_dim),
                                          log_std_min=pcfg.ls_min, log_std_max=pcfg.ls_max)
    critic = DeviceSoftQCritic(eng, lins(cparams, [(D, 512), (512, 256), (256, 1)]), standardizer=DeviceStandardizer(eng, D),
                               lr=lcfg.lr, eps=lcfg.adam_eps, tau=lcfg.tau)
    steps, _ = R.case_inputs(in_dim, A, 40, seed=32, updates=2)
    demo = dict(states=steps[0]["obs"], actions=steps[0]["act"], next_states=steps[0]["next_obs"],
                absorbing=steps[0]["absorbing"])
    data = dict(states=steps[1]["obs"], actions=steps[1]["act"], next_states=steps[1]["next_obs"],
                absorbing=steps[1]["absorbing"])
    agent = DeviceLSIQSAC(eng, policy, critic, demo, gamma=lcfg.gamma, batch_size=n_b, use_target=lcfg.use_target,
                          init_alpha=P.ALPHA, reg_mult=lcfg.reg_mult, plcy_loss_mode=mode, regularizer_mode=lcfg.reg,
                          Q_max=lcfg.q_max, Q_min=lcfg.q_min, loss_mode_exp=lcfg.exp_mode, Q_exp_loss=lcfg.exp_loss,
                          treat_absorbing_states=lcfg.treat, target_clipping=True, lossQ_type=typ, max_replay_size=64,
                          actor_optimizer=dict(lr=pcfg.lr, eps=pcfg.adam_eps))
    n_pi = L.value_rows(lcfg, B, n_b)
    rng = np.random.default_rng(33)
    noise = [dict(next=rng.standard_normal((B, A)), pi=rng.standard_normal((n_pi, A)), expert=rng.standard_normal((B - n_b, A)),
                  ppi=rng.standard_normal((B, A)), plog=rng.standard_normal((B, A))) for _ in range(n_iter)]
    noise = [{k: v.astype(np.float32) for k, v in e.items()} for e in noise]
    batches, inner = [], agent.iq_update
    d = lambda a: torch.as_tensor(a).cuda()

    def recording(obs, act, next_obs, absorbing, n_policy, eps=None, generator=None):
        e = noise[len(batches)]
        batches.append(dict(obs=obs.cpu().numpy(), act=act.cpu().numpy(), next_obs=next_obs.cpu().numpy(),
                            absorbing=absorbing.cpu().numpy(), n_policy=int(n_policy)))
        return inner(obs, act, next_obs, absorbing, n_policy,
                     eps=dict(q=dict(next=d(e["next"]), pi=d(e["pi"]), expert=d(e["expert"])),
                              pi=dict(pi=d(e["ppi"]), log=d(e["plog"]))))
    agent.iq_update = recording
    gen = torch.Generator(device="cuda").manual_seed(5)
    for i in range(n_iter):
        agent.fit(data if i == 0 else {k: v[:0] for k, v in data.items()}, generator=gen)
    torch.cuda.synchronize()
    assert len(batches) == n_iter and agent._iter == n_iter + 1 and agent.policy.iter == n_iter
    assert agent.replay.size == 40 and all(b["n_policy"] == n_b for b in batches)
    states = []
    for dt in (torch.float64, torch.float32):
        twin = LTwin(case["pparams"], cparams, case["central"], case["delta"], pcfg._replace(init_alpha=P.ALPHA), lcfg, dtype=dt,
                     check=dt == torch.float64)
        for b, e in zip(batches, noise):
            twin.iq_update(b, n_b, e, logging=True)
        if dt == torch.float64:
            L.assert_margins(twin.q.margins, (typ, mode), counts=False)
        states.append(twin.state())
    ref, f32 = states
    for flat, group in ((agent.critic.param, "critic"), (agent.policy.param, "policy")):
        r = cat(ref[group]["params"])
        spread = float(np.abs(cat(f32[group]["params"]) - r).max())
        err = float(np.abs(flat.double().cpu().numpy() - r).max())
        print(f"{typ} {mode} {group}: |device - f64| max {err:.3e} (float32 spread {spread:.3e})")
        assert err <= max(TOL, 4 * spread), (group, err, spread)
    for got, want in ((agent.critic.stand.colstats, ref["critic"]["colstats"]),
                      (agent.policy.stand.colstats, ref["policy"]["colstats"])):
        assert np.array_equal(got.cpu().numpy()[0], want[0]), (got[0, 0], want[0, 0])


# ------------------------------------------------------------------------------ fences, stores, refusals
@pytest.mark.parametrize("B,n_policy", ((18, 9), (2, 1)))
def test_fenced_operands_and_stores(eng, B, n_policy):
    in_dim, A = 12, 5
    steps, params = R.case_inputs(in_dim, A, B, seed=7, updates=1)
    base = L.LCfg(type="sqil_like", exp_mode="bootstrap", exp_loss="Huber", use_target=False, wd=1e-3, tau=0.5, reg_mult=2.0,
                  q_min=L.Q_MIN, q_max=L.Q_MAX)
    for cfg in (base._replace(mode="value_plcy"), base._replace(mode="q_old_policy"),
                base._replace(type="iq_like", exp_mode="fix", mode="off")):
        dev = LDev(eng, params, cfg, in_dim, A, B, target=[p + np.float32(0.01) for p in params])
        before = dev.snapshot()
        dev.f["out"] = Fenced(16, torch.float64)              # poisoned again
        s = L.case_steps(cfg, steps, n_policy)[0]             # value_plcy: a_pi / logp_pi fenced at exactly n_policy rows
        if cfg.mode == "value_plcy":
            assert s["a_pi"].shape == (n_policy, A) and s["logp_pi"].shape == (n_policy,)
        if cfg.mode == "q_old_policy":                        # no third pass: poisoned and unread
            s["a_pi"], s["logp_pi"] = np.full((B, A), np.nan, np.float32), np.full(B, np.nan, np.float32)
        dev.update(s, n_policy)
        after = dev.snapshot()
        dev.check_fences(L.cfg_id(cfg))
        assert_written(dict(out=dev.f["out"]), L.cfg_id(cfg))
        for key in ("param", "m", "v", "target_param"):       # weight decay: every element has a gradient and moves
            assert bool((after[key] != before[key]).all()), key
            assert bool(torch.isfinite(after[key]).all()), key
        assert torch.equal(after["packed"], eng.ilmlp_pack(*split(after["param"], in_dim + A)))
        assert torch.equal(after["target_packed"], eng.ilmlp_pack(*split(after["target_param"], in_dim + A)))
        out = after["out"]
        assert bool(torch.isfinite(out[:13]).all()) and bool(torch.isfinite(out[15]))
        n_v = L.value_rows(cfg, B, n_policy) if L.has_v(cfg) else 0
        assert float(after["colstats"][0, 0]) == 2 * B + n_v   # no target: X0, X1 and the value pass's rows
        for key in ("colstats", "target_colstats"):
            assert bool(torch.isfinite(after[key]).all())


def test_refusals_come_before_any_launch(eng):
    from olympic_hip import _abi
    from olympic_hip._ffi import lib
    in_dim, A, B = 12, 5, 18
    D = in_dim + A
    n_par = 512 * D + 512 + 256 * 512 + 256 + 256 + 1
    npk = int(lib().oly_ilmlp_packed_floats(D, 512, 256, 1))
    nws = int(lib().oly_iq_q_ws(B, in_dim, A))
    f32, f64 = torch.float32, torch.float64
    bufs = dict(obs=Fenced((B, in_dim), f32), act=Fenced((B, A), f32), next_obs=Fenced((B, in_dim), f32),
                absorbing=Fenced(B, f32), a_next=Fenced((B, A), f32), logp_next=Fenced(B, f32), a_pi=Fenced((B, A), f32),
                logp_pi=Fenced(B, f32), colstats=Fenced((3, D), f64), target_colstats=Fenced((3, D), f64),
                param=Fenced(n_par, f32), m=Fenced(n_par, f32), v=Fenced(n_par, f32), packed=Fenced(npk, f32),
                target_param=Fenced(n_par, f32), target_packed=Fenced(npk, f32), ws=Fenced(nws, f32), out=Fenced(16, f64))
    keep = []

    def block(ls=None, null_lsiq=False, **over):
        lk = dict(lossQ_type=0, loss_mode_exp=0, Q_exp_loss=1, target_clipping=1, Q_min=-1.0, Q_max=1.0)
        lk.update(ls or {})
        blk = _abi.LSIQ(**lk)
        keep.append(blk)
        kw = dict(in_dim=in_dim, act_dim=A, batch=B, n_policy=9, algo=_abi.IQ_ALGO["lsiq"], plcy_loss_mode=0,
                  regularizer_mode=0, treat_absorbing=0, use_target=1, update_target=1, step=0, pad=0, gamma=0.99, alpha=1e-3,
                  reg_mult=0.5, R_min=0.0, R_max=1.0, gradient_penalty_lambda=0.0, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.0, pad2=0.0, tau=0.005, packed_floats=npk, target_packed_floats=npk, ws_floats=nws,
                  lsiq=None if null_lsiq else C.pointer(blk))
        kw.update({k: b.t.data_ptr() for k, b in bufs.items()})
        kw.update(over)
        return _abi.IQQ(**kw)
    nan = float("nan")
    sq = dict(lossQ_type=1)
    bad = dict(no_block=dict(null_lsiq=True), bounds_equal=dict(ls=dict(Q_min=0.5, Q_max=0.5)),
               bounds_swapped=dict(ls=dict(Q_min=1.0, Q_max=-1.0)), q_min_nan=dict(ls=dict(Q_min=nan)),
               q_max_nan=dict(ls=dict(Q_max=nan)), fix_without_loss=dict(ls=dict(Q_exp_loss=0)),
               sqil_like_without_loss=dict(ls=dict(sq, loss_mode_exp=1, Q_exp_loss=0)),
               sqil_like_value_unequal=dict(ls=sq, n_policy=8), v0=dict(plcy_loss_mode=_abi.LSIQ_PLCY_LOSS_MODES["v0"]),
               type=dict(ls=dict(lossQ_type=2)), type_neg=dict(ls=dict(lossQ_type=-1)), exp_mode=dict(ls=dict(loss_mode_exp=2)),
               exp_loss=dict(ls=dict(Q_exp_loss=3)), exp_loss_neg=dict(ls=dict(Q_exp_loss=-1)), mode=dict(plcy_loss_mode=7),
               mode_neg=dict(plcy_loss_mode=-1), sqil_like_mode=dict(ls=sq, plcy_loss_mode=3), reg=dict(regularizer_mode=4),
               gp=dict(gradient_penalty_lambda=0.5), null_a_pi=dict(a_pi=None), null_logp_pi=dict(logp_pi=None),
               null_a_pi_off=dict(plcy_loss_mode=_abi.LSIQ_PLCY_LOSS_MODES["off"], a_pi=None),
               null_a_pi_value_plcy=dict(ls=sq, plcy_loss_mode=1, a_pi=None),
               null_logp_pi_sqil_value=dict(ls=sq, plcy_loss_mode=0, logp_pi=None))
    Lb = lib()
    for name, over in bad.items():
        f = block(**over)
        rc = Lb.oly_iq_q_update(eng.ctx.handle, C.byref(f), eng._s())
        assert rc == _abi.OLY_EINVAL, (name, rc)
    torch.cuda.synchronize()
    assert_untouched(bufs, "refused calls")


def test_the_engine_refuses_what_the_library_refuses(eng):
    from olympic_hip._ffi import OlyError
    in_dim, A, B, n_policy = SHAPES[1]
    steps, params = L.sweep_inputs(1)
    good = L.LCfg(q_min=L.Q_MIN, q_max=L.Q_MAX)
    dev = LDev(eng, params, good, in_dim, A, B)
    before = dev.snapshot()
    for over in (dict(lsiq=None), dict(lsiq=dict(block_of(good), Q_exp_loss=None)), dict(lsiq=dict(block_of(good), Q_min=2.0)),
                 dict(lsiq=dict(block_of(good), lossQ_type="other")), dict(lsiq=dict(block_of(good), extra=1)),
                 dict(plcy_loss_mode="v0"), dict(plcy_loss_mode="plcy"),
                 dict(lsiq=dict(block_of(good), lossQ_type="sqil_like"), plcy_loss_mode="value_expert"),
                 dict(algo="iq", lsiq=block_of(good))):
        with pytest.raises(OlyError):
            dev.update(steps[0], n_policy, **over)
    after = dev.snapshot()
    for key, a in before.items():
        assert same_bits(a, after[key]), key


# ------------------------------------------------------------------------------ checkpoint / resume
@pytest.mark.parametrize("name", ("iq_fix", "sqil_value_plcy"))
def test_a_saved_run_resumes_to_the_same_bits(eng, golden, tmp_path, name):
    g = golden(f"lsiq_q_update/{name}.npz")
    whole, gen = build_agent(eng, g, name)
    run_fixture(whole, g, 0, 4)
    first, _ = build_agent(eng, g, name)
    run_fixture(first, g, 0, 2)
    path = first.save(str(tmp_path / "lsiq.pt"), note="after update 2")
    resumed, _ = build_agent(eng, g, name)
    ptrs = [t.data_ptr() for t in (resumed.critic.param, resumed.critic.packed, resumed.critic.target_packed)]
    assert resumed.load(path)["note"] == "after update 2"
    assert resumed._iter == 3 and resumed.critic.step == 2
    assert ptrs == [t.data_ptr() for t in (resumed.critic.param, resumed.critic.packed, resumed.critic.target_packed)]
    run_fixture(resumed, g, 2, 4)
    torch.cuda.synchronize()
    a, b = whole.critic, resumed.critic
    for key in ("param", "target_param", "exp_avg", "exp_avg_sq", "packed", "target_packed"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert torch.equal(a.stand.colstats, b.stand.colstats) and torch.equal(a.target_stand.colstats, b.target_stand.colstats)
    assert torch.equal(whole.policy.stand.colstats, resumed.policy.stand.colstats)
    assert whole._iter == resumed._iter == 5
    # the kinds: an IQ checkpoint is not an LSIQ one, and the whole agent's is its own
    assert whole.state_dict()["kind"] == "lsiq_critic"
    sac, _ = build_agent(eng, g, name, sac=True)
    assert sac.state_dict()["kind"] == "lsiq_sac"
    from olympic_hip._ffi import OlyError
    with pytest.raises(OlyError):
        sac.load(path)
