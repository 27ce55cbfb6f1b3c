"""K27 with a second critic on the MI355X: oly_iq_pi_update with h_packed, the actor step of LSIQ_H / LSIQ_HC whose loss is
mean(alpha log_prob - (Q + H)), against the float64 restatement (tests/lsiq_h_restate.py's actor_twin on iq_pi_restate's
Twin) at iq_pi_restate's shapes (Bp = 1, 18, 16, 48, 33), three updates, with and without Standardizers; its bits (H's raw
values are the forward kernel's, a zero H leaves the one-critic call's bits, neither critic is written, two runs agree);
h_ws fenced at exactly the queried size; the refusals; and the whole agents DeviceLSIQHSAC / DeviceLSIQHCSAC: three fit
iterations against the twin, checkpoint and resume after iq_update 2 of 4.

The tolerance is test_gpu_iq_pi.py's TOL = 2e-5 (relative to the largest entry for the moments, to max(1, |value|) for the
scalars); lsiq_h_restate's float32 run of the same cases stays below TOL / 4 (tests/test_lsiq_h_cpu.py)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import iq_pi_restate as P
import lsiq_h_restate as H
from fences import Fenced, assert_untouched, fenced
from test_gpu_iq_pi import Dev, split

pytestmark = pytest.mark.gpu
TOL, SHAPES, CONFIGS, cat = P.TOL, P.SHAPES, P.CONFIGS, P.cat


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


class HPiDev(Dev):
    """test_gpu_iq_pi.py's fenced state with the second critic: its parameters, stream and statistics, and a second
    workspace of exactly oly_iq_pi_ws() floats."""

    def __init__(self, eng, case, cfg, in_dim, A, Bp, hparams=None):
        from olympic_hip._ffi import lib
        super().__init__(eng, case, cfg, in_dim, A, Bp)
        hp = case["hparams"] if hparams is None else hparams
        hflat = np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in hp])
        self.f.update(h_param=fenced(hflat), h_packed=Fenced(int(lib().oly_ilmlp_packed_floats(self.D, 512, 256, 1)), torch.float32),
                      h_ws=Fenced(self.nws, torch.float32),
                      h_colstats=fenced(np.zeros((3, self.D))) if cfg.standardizer else None)
        eng.ilmlp_pack(*split(self.t("h_param"), self.D, 1), packed=self.t("h_packed"))

    def update(self, s, alpha=P.ALPHA, with_h=True, **over):
        c = self.cfg
        self.inputs = {k: fenced(np.asarray(v, np.float32)) for k, v in s.items()}
        h = dict(packed=self.t("h_packed"), param=self.t("h_param"), colstats=self.t("h_colstats"), ws=self.t("h_ws"))
        h.update(over)
        o = self.eng.iq_pi_update(self.inputs["x"].t, self.inputs["eps"].t, self.t("central"), self.t("delta"),
                                  self.t("colstats"), self.t("param"), self.t("m"), self.t("v"), self.t("packed"),
                                  self.t("critic_packed"), self.t("critic_param"), self.t("critic_colstats"), self.t("ws"),
                                  self.step, c.lr, alpha=alpha, log_std_min=c.ls_min, log_std_max=c.ls_max,
                                  adam_eps=c.adam_eps, weight_decay=c.wd, h=h if with_h else None,
                                  out=dict(action=self.t("action"), log_prob=self.t("log_prob"), out=self.t("out")))
        self.step += 1
        return o["out"].clone()

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: None if f is None else f.t.clone() for k, f in self.f.items() if k not in ("ws", "h_ws")}


# ------------------------------------------------------------------------------ against the float64 yardstick
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["-".join(map(str, s)) for s in SHAPES])
def test_actor_step_against_float64(eng, k):
    in_dim, A, Bp = SHAPES[k]
    case = H.actor_case(k)
    for j, cfg in enumerate(CONFIGS):
        ref, ref_out, ref_acts = H.actor_yardstick(k, j)[:3]
        dev = HPiDev(eng, case, cfg, in_dim, A, Bp)
        out = np.stack([dev.update(s).cpu().numpy() for s in case["steps"]])
        got = dev.snapshot()
        dev.check_fences(P.cfg_id(cfg))
        who = f"{SHAPES[k]} {P.cfg_id(cfg)}"
        err = float(np.abs(got["param"].double().cpu().numpy() - cat(ref["policy"]["params"])).max())
        print(f"{who} param: |kernel - f64| max {err:.3e}")
        assert err <= TOL, (who, "param", err)
        r = cat(ref["policy"]["exp_avg"])
        err = float(np.abs(got["m"].double().cpu().numpy() - r).max()) / max(float(np.abs(r).max()), 1e-300)
        print(f"{who} m: relative to the largest entry {err:.3e}")
        assert err <= TOL, (who, "m", err)
        err = np.abs(out - ref_out) / np.maximum(1.0, np.abs(ref_out))
        print(f"{who} scalars: worst relative error {err.max():.3e}")
        assert np.all(err <= TOL), (who, out, ref_out)
        a_ref, lp_ref = ref_acts[-1]
        assert float(np.abs(got["action"].double().cpu().numpy() - a_ref).max()) <= TOL, who
        assert float(np.abs(got["log_prob"].double().cpu().numpy() - lp_ref).max()) <= TOL * max(1.0, np.abs(lp_ref).max()), who
        if cfg.standardizer:
            for key, want in (("colstats", ref["policy"]["colstats"]), ("critic_colstats", ref["critic"]["colstats"]),
                              ("h_colstats", ref["h"]["colstats"])):
                a = got[key].cpu().numpy()
                assert np.array_equal(a[0], want[0]), (who, key, "counts")
                assert np.all(np.abs(a - want) <= TOL * np.maximum(1.0, np.abs(want))), (who, key)
        assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim, 2 * A)))


# ------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("k", (1, 4), ids=("12-5-18", "48-16-33"))
@pytest.mark.parametrize("standardizer", (False, True), ids=("nostd", "std"))
def test_the_calls_bits(eng, k, standardizer):
    """H(x | a_new) in h_ws and Q in ws are oly_ilmlp_forward's on (x | a_new) with the statistics the call leaves each
    network; neither critic's parameters nor stream change a byte; a second run gives the same bits."""
    from olympic_hip._ffi import lib
    in_dim, A, Bp = SHAPES[k]
    case, cfg = H.actor_case(k), CONFIGS[0 if standardizer else 1]
    snaps = []
    for _ in range(2):
        dev = HPiDev(eng, case, cfg, in_dim, A, Bp)
        before = dev.snapshot()
        dev.update(case["steps"][0])
        got = dev.snapshot()
        dev.check_fences("bits")
        off = int(lib().oly_iq_pi_ws_values(Bp, in_dim, A))
        xa = torch.cat([dev.inputs["x"].t, got["action"]], dim=1).contiguous()
        q = eng.ilmlp_forward(xa, got["critic_packed"], 1, colstats=got["critic_colstats"]).reshape(-1)
        h = eng.ilmlp_forward(xa, got["h_packed"], 1, colstats=got["h_colstats"]).reshape(-1)
        assert torch.equal(dev.t("ws")[off:off + Bp], q)
        assert torch.equal(dev.t("h_ws")[off:off + Bp], h)
        assert not torch.equal(q, h) and not torch.equal(got["param"], before["param"])
        for key in ("critic_param", "critic_packed", "h_param", "h_packed", "central", "delta"):
            assert torch.equal(got[key], before[key]), key
        snaps.append(got)
    for key, a in snaps[0].items():
        if a is not None:
            assert torch.equal(a.view(torch.uint8), snaps[1][key].view(torch.uint8)), key


@pytest.mark.parametrize("standardizer", (False, True), ids=("nostd", "std"))
def test_a_zero_second_critic_leaves_the_one_critic_calls_bits(eng, standardizer):
    """With every parameter of H zero, H = 0 and its data gradient is 0: q + 0 and dX_Q / std_Q + 0 are the one-critic
    call's values, so the policy, its moments, the action, the log-probability, the scalars and the critic's statistics
    after three updates hold the bits of the call with h = None.  (That h = None itself is the call as it was is what
    tests/test_gpu_iq_pi.py holds, unchanged.)"""
    k = 3
    in_dim, A, Bp = SHAPES[k]
    case, cfg = H.actor_case(k), CONFIGS[0 if standardizer else 1]
    zero = [np.zeros_like(p) for p in case["hparams"]]
    a, b = HPiDev(eng, case, cfg, in_dim, A, Bp, hparams=zero), HPiDev(eng, case, cfg, in_dim, A, Bp, hparams=zero)
    oa = torch.stack([a.update(s) for s in case["steps"]])
    ob = torch.stack([b.update(s, with_h=False) for s in case["steps"]])
    ga, gb = a.snapshot(), b.snapshot()
    assert torch.equal(oa.view(torch.int64), ob.view(torch.int64))
    for key in ("param", "m", "v", "packed", "action", "log_prob", "colstats", "critic_colstats"):
        assert ga[key] is None and gb[key] is None or torch.equal(ga[key], gb[key]), key
    if standardizer:     # with h the second Standardizer took the rows, without it nothing touched it
        assert float(ga["h_colstats"][0, 0]) == 3 * Bp and float(gb["h_colstats"][0, 0]) == 0.0
    assert b.f["h_ws"].unwritten() == b.f["h_ws"].n


# ------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(eng):
    from olympic_hip import _abi
    from olympic_hip._ffi import OlyError, lib
    k = 1
    in_dim, A, Bp = SHAPES[k]
    case, cfg = H.actor_case(k), CONFIGS[0]
    dev = HPiDev(eng, case, cfg, in_dim, A, Bp)
    before = dev.snapshot()
    s = case["steps"][0]
    short = torch.zeros(dev.nws - 1, device="cuda")
    for over in (dict(ws=short), dict(ws=dev.t("ws")), dict(packed=dev.t("critic_packed")), dict(param=None),
                 dict(packed=None), dict(ws=None), dict(colstats=torch.zeros((3, dev.D), device="cuda")),
                 dict(param=dev.t("param"))):
        with pytest.raises(OlyError):
            dev.update(s, **over)
    with pytest.raises(OlyError):
        eng.iq_pi_update(dev.inputs["x"].t, dev.inputs["eps"].t, dev.t("central"), dev.t("delta"), dev.t("colstats"),
                         dev.t("param"), dev.t("m"), dev.t("v"), dev.t("packed"), dev.t("critic_packed"), dev.t("critic_param"),
                         dev.t("critic_colstats"), dev.t("ws"), 0, 3e-4, h=dict(packed=dev.t("h_packed")))
    # the library's own checks, under the engine's
    npk, ncpk = int(dev.t("packed").numel()), int(dev.t("h_packed").numel())
    x, e = dev.inputs["x"].t, dev.inputs["eps"].t

    def block(**over):
        kw = dict(in_dim=in_dim, act_dim=A, batch=Bp, step=0, alpha=0.2, log_std_min=-3.0, log_std_max=-0.5, lr=3e-4, beta1=0.9,
                  beta2=0.999, adam_eps=1e-5, weight_decay=0.0, x=x.data_ptr(), eps=e.data_ptr(),
                  central=dev.t("central").data_ptr(), delta=dev.t("delta").data_ptr(), colstats=dev.t("colstats").data_ptr(),
                  param=dev.t("param").data_ptr(), m=dev.t("m").data_ptr(), v=dev.t("v").data_ptr(),
                  packed=dev.t("packed").data_ptr(), packed_floats=npk, critic_packed=dev.t("critic_packed").data_ptr(),
                  critic_packed_floats=ncpk, critic_param=dev.t("critic_param").data_ptr(),
                  critic_colstats=dev.t("critic_colstats").data_ptr(), ws=dev.t("ws").data_ptr(), ws_floats=dev.nws,
                  action=dev.t("action").data_ptr(), log_prob=dev.t("log_prob").data_ptr(), out=dev.t("out").data_ptr(),
                  h_packed=dev.t("h_packed").data_ptr(), h_packed_floats=ncpk, h_param=dev.t("h_param").data_ptr(),
                  h_colstats=dev.t("h_colstats").data_ptr(), h_ws=dev.t("h_ws").data_ptr(), h_ws_floats=dev.nws)
        kw.update(over)
        return _abi.IQPi(**kw)
    bad = dict(null_param=dict(h_param=None), null_ws=dict(h_ws=None), short_ws=dict(h_ws_floats=dev.nws - 1),
               short_packed=dict(h_packed_floats=ncpk - 1), same_ws=dict(h_ws=dev.t("ws").data_ptr()),
               same_packed=dict(h_packed=dev.t("critic_packed").data_ptr()), odd_ws=dict(h_ws=dev.t("h_ws").data_ptr() + 4),
               odd_packed=dict(h_packed=dev.t("h_packed").data_ptr() + 4), odd_stats=dict(h_colstats=dev.t("h_colstats").data_ptr() + 4))
    for name, over in bad.items():
        rc = lib().oly_iq_pi_update(eng.ctx.handle, C.byref(block(**over)), eng._s())
        assert rc == _abi.OLY_EINVAL, (name, rc)
    after = dev.snapshot()
    for key, a in before.items():
        assert a is None or torch.equal(a.view(torch.uint8), after[key].view(torch.uint8)), key
    assert_untouched(dict(ws=dev.f["ws"], h_ws=dev.f["h_ws"]), "refused calls")


# ------------------------------------------------------------------------------ the whole agents
def build_whole(eng, case, **more):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceLSIQHCSAC, DeviceLSIQHSAC, DeviceSoftQCritic
    in_dim, A = case["in_dim"], case["A"]
    D, pcfg, lcfg, hcfg = in_dim + A, case["pcfg"], case["lcfg"], case["hcfg"]

    def lins(params, dims):
        out = [torch.nn.Linear(i, o) for i, o in dims]
        with torch.no_grad():
            for j, lin in enumerate(out):
                lin.weight.copy_(torch.as_tensor(params[2 * j]))
                lin.bias.copy_(torch.as_tensor(params[2 * j + 1]))
        return out
    if "min_a" in case:
        min_a, max_a = case["min_a"], case["max_a"]
    else:
        central, delta = case["central"].astype(np.float64), case["delta"].astype(np.float64)
        min_a, max_a = central - delta, central + delta
    policy = DeviceSquashedGaussianPolicy(eng, lins(case["pparams"], [(in_dim, 512), (512, 256), (256, 2 * A)]),
                                          min_a, max_a, standardizer=DeviceStandardizer(eng, in_dim),
                                          log_std_min=pcfg.ls_min, log_std_max=pcfg.ls_max)
    dims = [(D, 512), (512, 256), (256, 1)]
    critic = DeviceSoftQCritic(eng, lins(case["qparams"], dims), standardizer=DeviceStandardizer(eng, D), lr=lcfg.lr,
                               eps=lcfg.adam_eps, tau=lcfg.tau)
    h_critic = DeviceSoftQCritic(eng, lins(case["hparams"], dims), standardizer=DeviceStandardizer(eng, D), lr=hcfg.lr,
                                 eps=hcfg.adam_eps, tau=lcfg.tau)
    steps = case["steps"]
    demo = dict(states=steps[0]["obs"], actions=steps[0]["act"], next_states=steps[0]["next_obs"], absorbing=steps[0]["absorbing"])
    kw = dict(gamma=lcfg.gamma, batch_size=case["n_policy"], use_target=lcfg.use_target,
              init_alpha=case.get("init_alpha", hcfg.alpha), reg_mult=lcfg.reg_mult,
              plcy_loss_mode=lcfg.mode, regularizer_mode=lcfg.reg, Q_max=lcfg.q_max, Q_min=lcfg.q_min,
              loss_mode_exp=lcfg.exp_mode, Q_exp_loss=lcfg.exp_loss, target_clipping=True, lossQ_type=lcfg.type,
              max_replay_size=64, h_critic=h_critic, max_H_policy_tau_up=hcfg.tau_up, max_H_policy_tau_down=hcfg.tau_down,
              actor_optimizer=dict(lr=pcfg.lr, eps=pcfg.adam_eps))
    if hcfg.cost:
        kw.update(H_tau=hcfg.tau, H_loss_mode=hcfg.loss)
    kw.update(more)
    return (DeviceLSIQHCSAC if hcfg.cost else DeviceLSIQHSAC)(eng, policy, critic, demo, **kw)


def whole_noise(case, n_iter, seed=77):
    B, A, n_p = case["B"], case["A"], case["n_policy"]
    rng = np.random.default_rng(seed)
    return [{k: rng.standard_normal((B - n_p if k == "expert" else B, A)).astype(np.float32)
             for k in ("next", "expert", "pi", "h_next", "h_pi", "ppi", "plog")} for _ in range(n_iter)]


def device_eps(e):
    d = lambda a: torch.as_tensor(a).cuda()
    return dict(q={k: d(e[k]) for k in ("next", "expert", "pi", "h_next", "h_pi")}, pi=dict(pi=d(e["ppi"]), log=d(e["plog"])))


@pytest.mark.parametrize("cost", (False, True), ids=("lsiq_h", "lsiq_hc"))
def test_a_fit_run_of_the_whole_agent_against_the_twin(eng, cost):
    """DeviceLSIQHSAC / DeviceLSIQHCSAC.fit for three iterations (the dataset into the replay memory, a batch drawn from it
    and from the demonstrations, iq_update = the Q update, the H update, the two-critic policy update, the counters)
    against lsiq_h_restate's whole twin.  fit draws its batches on the device, so iq_update is wrapped: it records the
    batch it was given and supplies the noise."""
    import iq_restate as R
    case = H.agent_case(cost)
    n_iter, n_b = 3, case["n_policy"]
    agent = build_whole(eng, case)
    noise = whole_noise(case, n_iter)
    steps, _ = R.case_inputs(case["in_dim"], case["A"], 40, seed=32, updates=1)
    data = dict(states=steps[0]["obs"], actions=steps[0]["act"], next_states=steps[0]["next_obs"], absorbing=steps[0]["absorbing"])
    batches, inner = [], agent.iq_update

    def recording(obs, act, next_obs, absorbing, n_policy, eps=None, generator=None):
        e = noise[len(batches)]
        batches.append(dict(obs=obs.cpu().numpy(), act=act.cpu().numpy(), next_obs=next_obs.cpu().numpy(),
                            absorbing=absorbing.cpu().numpy(), n_policy=int(n_policy)))
        return inner(obs, act, next_obs, absorbing, n_policy, eps=device_eps(e))
    agent.iq_update = recording
    gen = torch.Generator(device="cuda").manual_seed(5)
    for i in range(n_iter):
        agent.fit(data if i == 0 else {k: v[:0] for k, v in data.items()}, generator=gen)
    torch.cuda.synchronize()
    assert len(batches) == n_iter and agent._iter == n_iter + 1 and agent.policy.iter == n_iter
    assert agent.pi_step == agent.critic.step == agent.h_critic.step == n_iter
    states = []
    for dt in (torch.float64, torch.float32):
        twin = H.whole_twin(case, dt, check=dt == torch.float64)
        for b, e in zip(batches, noise):
            twin.iq_update(b, n_b, e, logging=True)
        if dt == torch.float64:
            H.assert_margins(twin.critic.h.margins, ("whole", cost), counts=False)
        states.append(twin.state())
    ref, f32 = states
    for flat, group in ((agent.critic.param, "q"), (agent.h_critic.param, "h"), (agent.policy.param, "policy")):
        r = cat(ref[group]["params"])
        spread = float(np.abs(cat(f32[group]["params"]) - r).max())
        err = float(np.abs(flat.double().cpu().numpy() - r).max())
        print(f"{'hc' if cost else 'h'} {group}: |device - f64| max {err:.3e} (float32 spread {spread:.3e})")
        assert err <= max(TOL, 4 * spread), (group, err, spread)
    for got, want in ((agent.critic.stand.colstats, ref["q"]["colstats"]), (agent.h_critic.stand.colstats, ref["h"]["colstats"]),
                      (agent.policy.stand.colstats, ref["policy"]["colstats"])):
        assert np.array_equal(got.cpu().numpy()[0], want[0]), (got[0, 0], want[0, 0])


@pytest.mark.parametrize("cost", (False, True), ids=("lsiq_h", "lsiq_hc"))
def test_a_run_saved_after_iq_update_2_of_4_resumes_to_the_same_bits(eng, tmp_path, cost):
    from olympic_hip._ffi import OlyError
    case = H.agent_case(cost)
    steps = list(case["steps"]) + [case["steps"][0]]
    noise = whole_noise(case, 4)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()

    def run(agent, first, last):
        for s, e in list(zip(steps, noise))[first:last]:
            agent.iq_update(d(s["obs"]), d(s["act"]), d(s["next_obs"]), d(s["absorbing"]), case["n_policy"], eps=device_eps(e))
            agent._iter += 1
            agent.policy.iter = getattr(agent.policy, "iter", 0) + 1
    def warmed():      # iq_update trains the policy once the replay memory holds transitions (the checkpoint carries it)
        agent, s0 = build_whole(eng, case), steps[0]
        agent.replay.add(dict(states=d(s0["obs"]), actions=d(s0["act"]), next_states=d(s0["next_obs"]), absorbing=d(s0["absorbing"])))
        return agent
    whole = warmed()
    run(whole, 0, 4)
    first = warmed()
    run(first, 0, 2)
    path = first.save(str(tmp_path / "whole.pt"), note="after iq_update 2")
    resumed = build_whole(eng, case)
    assert resumed.load(path)["note"] == "after iq_update 2"
    assert resumed._iter == 3 and resumed.h_critic.step == 2 and resumed.pi_step == 2 and resumed.replay.size == case["B"]
    run(resumed, 2, 4)
    torch.cuda.synchronize()
    for a, b in ((whole.critic, resumed.critic), (whole.h_critic, resumed.h_critic)):
        for key in ("param", "target_param", "exp_avg", "exp_avg_sq", "packed", "target_packed"):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
        assert torch.equal(a.stand.colstats, b.stand.colstats) and torch.equal(a.target_stand.colstats, b.target_stand.colstats)
    assert torch.equal(whole.policy.param, resumed.policy.param) and torch.equal(whole.pi_exp_avg, resumed.pi_exp_avg)
    assert torch.equal(whole.h_max_state, resumed.h_max_state) and float(whole.h_max_state[1]) == 1.0
    assert whole.state_dict()["kind"] == ("lsiq_hc_sac" if cost else "lsiq_h_sac")
    from test_gpu_lsiq_h import build_agent
    with pytest.raises(OlyError):
        build_agent(eng, case).load(path)          # the critic side's kind is its own


# ------------------------------------------------------------------------------ the reference-run fixtures
@pytest.mark.parametrize("name", H.FIXTURES)
def test_fixture_through_the_whole_agent(eng, golden, name):
    """The reference's own LSIQ_H / LSIQ_HC, four whole iq_updates (tests/golden/gen_lsiq_h_update.py), repeated by
    DeviceLSIQHSAC / DeviceLSIQHCSAC from the same initial networks, batches and noise: both critics, both targets, the
    policy trained by the two-critic actor loss, the seven H scalars of every iteration, the running maximum and every
    Standardizer's count, within max(2e-5, 4 x the stored spread)."""
    import os
    import sys
    import iq_restate as R
    from test_gpu_iq_q import split as qsplit
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_lsiq_h_update as gen
    g = golden(f"lsiq_h_update/{name}.npz")
    spec = gen.FIXTURES[name]
    lcfg, hcfg = gen.twin_cfgs(spec, float(g["alpha"]))
    init = lambda prefix, seed: [gen.w2_init(seed) if n == "w2" else g[f"{prefix}_init_{n}"] for n in R.NAMES]
    order = [k for k in gen.PASSES + gen.PI_PASSES if spec["cost"] or k != "h_pi"]
    case = dict(in_dim=gen.IN_DIM, A=gen.ACT_DIM, B=gen.B, n_policy=int(g["n_policy"]), min_a=g["min_a"], max_a=g["max_a"],
                pparams=init("policy", 11), qparams=init("critic", 12), hparams=init("h", gen.H_W2_SEED),
                pcfg=P.PiCfg(lr=float(g["lr_actor"]), ls_min=gen.G.LOG_STD_MIN, ls_max=gen.G.LOG_STD_MAX), lcfg=lcfg, hcfg=hcfg,
                init_alpha=gen.INIT_ALPHA,
                steps=[{k: g[k][i] for k in ("obs", "act", "next_obs", "absorbing")} for i in range(gen.N_ITER)])
    agent = build_whole(eng, case)
    s0, d = case["steps"][0], lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    agent.replay.add(dict(states=d(s0["obs"]), actions=d(s0["act"]), next_states=d(s0["next_obs"]), absorbing=d(s0["absorbing"])))
    assert abs(agent.alpha - float(g["alpha"])) <= 1e-7 * float(g["alpha"])
    outs = []
    for i, s in enumerate(case["steps"]):
        agent.iq_update(d(s["obs"]), d(s["act"]), d(s["next_obs"]), d(s["absorbing"]), case["n_policy"],
                        eps=device_eps({k: g["eps_" + k][i] for k in order} | ({} if spec["cost"] else {"h_pi": g["eps_pi"][i]})))
        outs.append(agent.h_out.cpu().numpy())
        agent._iter += 1
        agent.policy.iter = getattr(agent.policy, "iter", 0) + 1
    torch.cuda.synchronize()
    assert agent.pi_step == agent.critic.step == agent.h_critic.step == gen.N_ITER
    host = lambda t: t.double().cpu().numpy()
    for prefix, params in (("critic", qsplit(host(agent.critic.param), gen.D)), ("target", qsplit(host(agent.critic.target_param), gen.D)),
                           ("h", qsplit(host(agent.h_critic.param), gen.D)), ("h_target", qsplit(host(agent.h_critic.target_param), gen.D)),
                           ("policy", split(host(agent.policy.param), gen.IN_DIM, 2 * gen.ACT_DIM))):
        err, tol = H.fixture_errors(g, gen, params, prefix), max(TOL, 4 * float(g[f"spread_{prefix}"]))
        print(f"{name} {prefix}: |device - reference| max {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, (prefix, err, tol)
    scal, out = g["scalars"][:, :7], np.stack(outs)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * float(g["spread_scalars"]))
    print(f"{name} H scalars: worst |device - reference| / tolerance {np.max(np.abs(out[:, :7] - scal) / tol):.3f}")
    assert np.all(np.abs(out[:, :7] - scal) <= tol), np.abs(out[:, :7] - scal) / tol
    assert np.all(np.abs(out[:, 8] - g["maxima"]) <= max(TOL, 4 * float(g["spread_max"])) * np.abs(g["maxima"]))
    for got, key in ((agent.policy.stand, "policy_colstats"), (agent.critic.stand, "colstats"),
                     (agent.critic.target_stand, "target_colstats"), (agent.h_critic.stand, "h_colstats"),
                     (agent.h_critic.target_stand, "h_target_colstats")):
        a, want = got.colstats.cpu().numpy(), g[key]
        assert np.array_equal(a[0], want[0]), (key, a[0, 0], want[0, 0])
        assert np.all(np.abs(a - want) <= np.maximum(TOL * np.maximum(1.0, np.abs(want)), 1e-9)), key
