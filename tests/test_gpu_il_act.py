"""K21 on the GPU: one acting step (oly_il_act) against K16's forward, K7's statistics, K5's controls and the float64
restatement of tests/il_act_restate.py; DeviceGaussianPolicy.act against draw_action; ILCore on the real environment.

Tolerances.  mu is K16's kernel structure: bit-equal to Engine.ilmlp_forward.  colstats and ctrl come from the same
expressions as oly_col_stats / oly_il_ctrl: bit-equal.  action against torch's float32 mu + exp(log_sigma) * eps:
1e-6 (|mu| + |sigma eps|), about 8 ulp, which covers a 1-2 ulp exp plus one rounding each for the multiply and the add.
mu against float64: the project's device tolerance 2e-5 (tests/disc_log_restate.py) relative to max(1, |mu|).  The
episode means against a float64 torch restatement: 1e-12 relative, as for K20."""
import gc

import numpy as np
import pytest
import torch

import il_act_restate as ar
from il_shapes import _columns, critic_params, guarded

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
_ref = {}


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def _dev(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


def act_case(n, D, A, seed):
    """Weights (nn.Linear's initialisation), log_sigma, columns of different scale and offset, prior statistics of 300
    other rows (non-trivial), noise."""
    rng = np.random.default_rng(seed)
    params = critic_params(D, seed, out_dim=A)
    scale, shift = _columns(rng, D)
    x = (rng.standard_normal((n, D)) * scale + shift).astype(np.float32)
    prior = (rng.standard_normal((300, D)) * scale + shift).astype(np.float32).astype(np.float64)
    cs = np.stack([np.full(D, 300.0), prior.sum(0), np.square(prior).sum(0)])
    log_sigma = rng.uniform(-1.5, 0.3, A).astype(np.float32)
    eps = rng.standard_normal((n, A)).astype(np.float32)
    return params, log_sigma, cs, x, eps


# ------------------------------------------------------------------------------ 1. shapes
#              n   in  act
# the last one is past the row count at which the forward switches to 32-row tiles (2 x 256 CUs x 32 rows), ragged,
# with two output column tiles: four output-layer waves
ACT_SHAPES = ((1, 32, 11), (15, 17, 1), (16, 32, 16), (17, 45, 17), (33, 64, 32), (257, 32, 11), (4096, 32, 11),
              (16417, 45, 17))


@pytest.mark.parametrize("update", (True, False), ids=("update", "frozen"))
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=["x".join(map(str, s)) for s in ACT_SHAPES])
def test_act_against_the_separate_kernels_and_float64(eng, shape, update):
    n, D, A = shape
    params, log_sigma, cs0, x, eps = act_case(n, D, A, seed=11 + n + D + A)
    key = (shape, update)
    if key not in _ref:
        _ref[key] = ar.restate_act(params, log_sigma, cs0, x, eps=eps, update_stats=update, device="cuda")
    ref = _ref[key]
    packed = eng.ilmlp_pack(*[_dev(p) for p in params])
    xd, ls, ed = _dev(x), _dev(log_sigma), _dev(eps)
    # the separate path: oly_col_stats, then K16's forward on those statistics
    cs_sep = _dev(cs0, F64)
    if update:
        eng.col_stats(xd, cs_sep)
    mu_sep = eng.ilmlp_forward(xd, packed, A, "identity", colstats=cs_sep)

    def run(want_mu=True, eps_t=ed):
        cs = _dev(cs0, F64)
        out = dict(action=guarded((n, A), F32), mu=guarded((n, A), F32))
        o = eng.il_act(xd, packed, ls, cs, eps=eps_t, update_stats=update, want_mu=want_mu,
                       out={k: g.t for k, g in out.items() if k != "mu" or want_mu})
        torch.cuda.synchronize()
        assert all(g.intact() for g in out.values())
        assert (o["mu"] is None) == (not want_mu) and o["ctrl"] is None
        return o, cs

    o, cs = run()
    assert torch.equal(cs, cs_sep)                                           # oly_col_stats' bits
    assert torch.equal(o["mu"], mu_sep)                                      # oly_ilmlp_forward's bits
    mu, act = o["mu"].cpu().numpy(), o["action"].cpu().numpy()
    t_act = (mu_sep + torch.exp(ls) * ed).cpu().numpy()
    bound = 1e-6 * (np.abs(mu) + np.abs(np.exp(log_sigma) * eps))
    err = np.abs(act.astype(np.float64) - t_act.astype(np.float64))
    print(f"{shape} update={update}: action vs torch max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    rel = np.abs(mu - ref["mu"]) / np.maximum(1.0, np.abs(ref["mu"]))
    print(f"{shape} update={update}: mu vs float64 max rel {rel.max():.2e}")
    assert rel.max() <= ar.DEV_TOL
    want_cs = ref["colstats"]
    assert np.all(np.abs(cs.cpu().numpy() - want_cs) <= 1e-12 * np.maximum(1.0, np.abs(want_cs)))
    assert np.abs(act - ref["action"]).max() <= 2 * ar.DEV_TOL * max(1.0, np.abs(ref["action"]).max())
    # deterministic: action has mu's bits
    od, _ = run(eps_t=None)
    assert torch.equal(od["action"], mu_sep) and torch.equal(od["mu"], mu_sep)
    # want_mu=False changes nothing else; a second run gives identical bits
    o2, cs2 = run(want_mu=False)
    assert torch.equal(o2["action"], o["action"]) and torch.equal(cs2, cs)
    o3, cs3 = run()
    assert torch.equal(o3["action"], o["action"]) and torch.equal(o3["mu"], o["mu"]) and torch.equal(cs3, cs)


# ------------------------------------------------------------------------------ 2. controls
def _spec(robot):
    from olympic_hip import specs
    if robot == "h1_arms":            # 19 actions: the columns of one action row come from two output-layer waves
        return specs.unitree_h1("walk", disable_arms=False)
    return specs.unitree_h1("walk") if robot == "h1" else specs.atlas("walk")


#                 the issue's cases                                                    two waves per row; 32-row tiles
CTRL_CASES = [(r, n) for r in ("h1", "atlas") for n in (1, 17, 257)] + [("h1_arms", 17), ("h1_arms", 16417)]


@pytest.mark.parametrize("robot,n", CTRL_CASES)
def test_controls_have_il_ctrl_s_bits(robot, n):
    from olympic_hip.engine import Engine
    spec = _spec(robot)
    e = Engine(0).il_configure(spec)
    try:
        A, D = int(spec.n_act), int(spec.n_obs)
        assert A == {"h1": 11, "h1_arms": 19}.get(robot, A)
        params, _, cs0, x, _ = act_case(n, D, A, seed=5 + n + A)
        rng = np.random.default_rng(77 + n + A)
        # sigma 2 with unit noise around a small mean: actions of std 2, a fair share clamped on both sides
        log_sigma = np.full(A, np.log(2.0), np.float32)
        eps = rng.standard_normal((n, A)).astype(np.float32)
        packed = e.ilmlp_pack(*[_dev(p) for p in params])
        for f64 in (False, True):
            g = guarded((n, spec.nu), F64 if f64 else F32)
            o = e.il_act(_dev(x), packed, _dev(log_sigma), _dev(cs0, F64), eps=_dev(eps), want_ctrl=True, ctrl_f64=f64,
                         out=dict(ctrl=g.t))
            want = e.il_ctrl(o["action"], ctrl_f64=f64)
            torch.cuda.synchronize()
            assert g.intact()
            assert o["ctrl"].dtype == (F64 if f64 else F32) and tuple(o["ctrl"].shape) == (n, spec.nu)
            assert torch.equal(o["ctrl"], want)
            ctrl64, clamped = ar.restate_ctrl(spec, o["action"].cpu().numpy())
            driven = np.zeros(spec.nu, bool)
            driven[np.asarray(spec.act_to_ctrl)] = True
            share = clamped[:, driven].mean()
            print(f"{robot} n={n} f64={f64}: clamped share {share:.3f}")
            assert 0.05 <= share <= 0.95      # checked with numpy for these seeds: 0.60 .. 0.80
            got = o["ctrl"].cpu().numpy().astype(np.float64)
            assert np.array_equal(got, ctrl64 if f64 else ctrl64.astype(np.float32).astype(np.float64))
            lo_j, hi_j = np.zeros(spec.nu), np.zeros(spec.nu)
            lo_j[np.asarray(spec.act_to_ctrl)], hi_j[np.asarray(spec.act_to_ctrl)] = spec.ctrl_lo, spec.ctrl_hi
            assert (clamped & (ctrl64 == lo_j)).any() and (clamped & (ctrl64 == hi_j)).any()      # both sides
    finally:
        torch.cuda.synchronize()
        e.ctx.close()


# ------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_the_context_usable():
    from olympic_hip._ffi import OlyError
    from olympic_hip.engine import Engine
    from olympic_hip import _abi, _ffi, specs
    import ctypes as C
    e = Engine(0)
    try:
        def call(n, D, A, want_ctrl=False, raw=False):
            x = torch.zeros((max(n, 1), D), dtype=F32, device="cuda")[:n]
            cs = torch.zeros((3, D), dtype=F64, device="cuda")
            ls = torch.zeros(A, dtype=F32, device="cuda")
            pk = torch.zeros(int(_ffi.lib().oly_ilmlp_packed_floats(32, 512, 256, 11)), device="cuda")
            if not raw:
                return e.il_act(x, pk, ls, cs, want_ctrl=want_ctrl)
            act = torch.zeros((max(n, 1), A), dtype=F32, device="cuda")
            ctrl = torch.zeros((max(n, 1), 64), dtype=F32, device="cuda")
            f = _abi.ILAct(n=n, in_dim=D, act_dim=A, update_stats=1, x=x.data_ptr(), colstats=cs.data_ptr(),
                           packed=pk.data_ptr(), log_sigma=ls.data_ptr(), eps=None, action=act.data_ptr(), mu=None,
                           ctrl=ctrl.data_ptr() if want_ctrl else None, out_flags=0, pad=0)
            e.ctx.call("oly_il_act", C.byref(f), e._s())
            return cs

        # through the engine and straight at the C entry: both refuse, and the statistics are not touched (no launch)
        for raw in (False, True):
            with pytest.raises(OlyError):
                call(4, 32, 11, want_ctrl=True, raw=raw)            # ctrl before any model is configured
            for n, D, A in ((4, 65, 11), (4, 32, 33), (0, 32, 11)):
                with pytest.raises(OlyError):
                    call(n, D, A, raw=raw)
        e.il_configure(specs.unitree_h1("walk"))
        for raw in (False, True):
            with pytest.raises(OlyError):
                call(4, 32, 10, want_ctrl=True, raw=raw)            # act_dim differs from the configured n_act
        f = _abi.ILAct(n=4, in_dim=32, act_dim=11)
        with pytest.raises(OlyError):
            e.ctx.call("oly_il_act", C.byref(f), e._s())           # NULL required pointers
        cs = call(4, 32, 11, raw=True)
        torch.cuda.synchronize()
        assert cs[0].tolist() == [4.0] * 32                         # the context is still usable: this call ran
        o = call(4, 32, 11, want_ctrl=True)
        torch.cuda.synchronize()
        assert tuple(o["ctrl"].shape) == (4, 11) and bool(torch.isfinite(o["action"]).all())
    finally:
        torch.cuda.synchronize()
        e.ctx.close()


# ------------------------------------------------------------------------------ 4. policy.act vs draw_action
def _policy(eng, D, A, seed, std_0=0.5):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceGaussianPolicy
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, A)]
    return DeviceGaussianPolicy(eng, lins, DeviceStandardizer(eng, D), std_0=std_0)


def test_policy_act_is_draw_action(eng):
    D, A, n = 32, 11, 48
    pa, pb = _policy(eng, D, A, 3), _policy(eng, D, A, 3)
    assert torch.equal(pa.theta, pb.theta)
    ga, gb = (torch.Generator(device="cuda").manual_seed(21) for _ in range(2))
    rng = np.random.default_rng(8)
    scale, shift = _columns(rng, D)
    for k in range(3):
        x = _dev((rng.standard_normal((n, D)) * scale + shift).astype(np.float32))
        a, c = pa.act(x, generator=ga)
        b = pb.draw_action(x, generator=gb)
        torch.cuda.synchronize()
        assert c is None and tuple(a.shape) == (n, A)
        assert torch.equal(pa.stand.colstats, pb.stand.colstats), k
        assert float(pa.stand.colstats[0, 0]) == (k + 1) * n and not pa.stand._fresh
        mu = pb.predict(x)
        bound = 1e-6 * (mu.abs() + (b - mu).abs()).double()
        assert bool(((a.double() - b.double()).abs() <= bound).all()), k
        assert torch.equal(ga.get_state(), gb.get_state())
    xq = _dev(rng.standard_normal((n, D)).astype(np.float32))
    assert torch.equal(pa.predict(xq), pb.predict(xq))
    # given noise and the deterministic switch
    e = torch.randn((n, A), dtype=F32, device="cuda", generator=ga)
    a1, _ = pa.act(xq, eps=e)
    mu1 = pa.predict(xq)                                          # the statistics act left
    assert bool(((a1 - (mu1 + torch.exp(pa.log_sigma) * e)).abs() <= 1e-6 * (mu1.abs() + (torch.exp(pa.log_sigma) * e).abs())).all())
    st = ga.get_state()
    a2, _ = pa.act(xq, generator=ga, deterministic=True)
    assert torch.equal(a2, pa.predict(xq)) and torch.equal(ga.get_state(), st)


# ------------------------------------------------------------------------------ 5. / 6. ILCore on the real environment
class RecordingAgent:
    def __init__(self):
        self.fits = []

    def fit(self, dataset, generator=None):
        self.fits.append({k: v.clone() for k, v in dataset.items()})
        return len(self.fits)


@pytest.fixture(scope="module")
def h1_env():
    from olympic_hip.envs import LocoEnvBase
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=48, seed=0)
    env.vec.spec.horizon = 5
    env.vec.info.horizon = 5
    yield env
    torch.cuda.synchronize()
    env.vec.eng.ctx.close()
    gc.collect()


def check_blocks(d, last, T, N):
    s, nx = d["state"], d["next_state"]
    assert tuple(s.shape) == tuple(nx.shape) == (T, N, 32) and s.dtype == F32 and s.data_ptr() != nx.data_ptr()
    m = last[:-1]
    assert torch.equal(s[1:][~m], nx[:-1][~m])                 # no reset: the next state is the state
    return m


def test_core_learn_on_the_real_environment(h1_env):
    from olympic_hip.il_core import ILCore
    vec, eng = h1_env.vec, h1_env.vec.eng
    pol = _policy(eng, vec.spec.n_obs, vec.spec.n_act, 5)
    agent = RecordingAgent()
    gen = torch.Generator(device="cuda").manual_seed(2)
    core = ILCore(agent, vec, pol, generator=gen)
    steps_seen, lasts_seen = [], []
    step0 = vec.step

    def step(actions, ctrl=None):
        out = step0(actions, ctrl=ctrl)
        steps_seen.append(vec.episode_steps.clone())            # the count after the step, before any reset
        lasts_seen.append(out[3]["last"].clone())               # what the environment reported
        return out
    vec.step = step
    try:
        assert core.learn(12, 6) == [1, 2]
    finally:
        vec.step = step0
    torch.cuda.synchronize()
    N = 48
    es, true_last = torch.stack(steps_seen), torch.stack(lasts_seen)       # [12, N]
    ab = torch.cat([agent.fits[0]["absorbing"], agent.fits[1]["absorbing"]])
    handed = true_last.clone()
    handed[5] = True
    handed[11] = True
    assert torch.equal(torch.cat([agent.fits[0]["last"], agent.fits[1]["last"]]), handed)   # set in the hand-over only
    assert torch.equal(core.blocks["last"], true_last[6:])
    # last exactly where absorbing or the episode's step count reached the horizon
    assert torch.equal(true_last, ab | (es >= 5))
    assert bool(true_last.any())
    # episode_steps restarts after each last
    for t in range(1, 12):
        want = torch.where(true_last[t - 1], torch.ones_like(es[t]), es[t - 1] + 1)
        assert torch.equal(es[t], want), t
    assert torch.equal(es[0], torch.ones_like(es[0]))
    for i, d in enumerate(agent.fits):
        check_blocks(d, true_last[6 * i:6 * i + 6], 6, N)
        assert tuple(d["action"].shape) == (6, N, 11) and tuple(d["reward"].shape) == (6, N)
    # across the fit boundary too: the second fit continues the first
    s = torch.cat([agent.fits[0]["state"], agent.fits[1]["state"]])
    nx = torch.cat([agent.fits[0]["next_state"], agent.fits[1]["next_state"]])
    m = true_last[:-1]
    assert torch.equal(s[1:][~m], nx[:-1][~m])
    # at the horizon every environment was reset together: its post-reset state is a fresh trajectory sample
    assert bool(m.any()) and not torch.equal(s[1:][m], nx[:-1][m])


def test_core_learn_with_the_real_agent(h1_env):
    from olympic_hip.gail import DeviceStandardizer, GAILDiscriminator, GAILDiscriminatorReward
    from olympic_hip.il_agent import (DeviceGAILDiscriminatorTrainer, DeviceGaussianPolicy, DeviceILCritic, DeviceTRPO,
                                      GAILAgent)
    from olympic_hip.il_core import ILCore
    env, vec, eng = h1_env, h1_env.vec, h1_env.vec.eng
    n_obs, n_act = vec.spec.n_obs, vec.spec.n_act
    mask = vec.get_kinematic_obs_mask()
    with torch.random.fork_rng(devices=[0]):
        torch.manual_seed(4)
        disc = GAILDiscriminatorReward(eng, GAILDiscriminator(len(mask)).cuda(), state_mask=mask)
        trainer = DeviceGAILDiscriminatorTrainer(disc, env.create_dataset()["states"], entcoeff=1e-3, lr=5e-6, batch_size=128)
        stand = DeviceStandardizer(eng, n_obs)
        critic = DeviceILCritic(eng, [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)],
                                stand, lr=1e-4)
        pol = DeviceGaussianPolicy(eng, [torch.nn.Linear(n_obs, 512), torch.nn.Linear(512, 256),
                                         torch.nn.Linear(256, n_act)], stand, std_0=0.8)
    trpo = DeviceTRPO(pol, max_kl=1e-2, ent_coeff=1e-3, n_epochs_cg=25)
    agent = GAILAgent(eng, disc, trainer, critic, trpo, gamma=0.99, lam=0.97, env_reward_frac=0.0, train_D_n_th_epoch=2,
                      critic_fit_params=dict(n_epochs=1, batch_size=128))
    core = ILCore(agent, vec, pol, generator=torch.Generator(device="cuda").manual_seed(6))
    trained = []
    for _ in range(2):
        (out,) = core.learn(6, 6)
        torch.cuda.synchronize()
        for k, v in out.items():
            if torch.is_tensor(v):
                assert bool(torch.isfinite(v).all()), k
        trained.append(bool(out["disc_trained"]))
    assert trained == [False, True]       # iter 1, 2 with train_D_n_th_epoch = 2: trained where iter % 2 == 0
    assert bool(torch.isfinite(pol.theta).all())


def test_core_evaluate_on_the_real_environment(h1_env):
    from olympic_hip.il_core import ILCore
    vec, eng = h1_env.vec, h1_env.vec.eng
    pol = _policy(eng, vec.spec.n_obs, vec.spec.n_act, 9)
    core = ILCore(RecordingAgent(), vec, pol, generator=torch.Generator(device="cuda").manual_seed(3))
    o, b = core.evaluate(50, return_blocks=True)
    assert o["n_episodes"] == 50 and 0 < o["L"] <= 5
    r, last = b["reward"].double(), b["last"]
    T, N = r.shape
    assert N == 48 and T <= 2 * 5
    assert last.sum(0).tolist() == [2, 2] + [1] * 46             # the quotas: 50 // 48 + (e < 50 % 48)
    assert int(last.sum()) == 50
    # float64 restatement over the returned blocks: per environment, per episode, in step order
    gamma = float(vec.info.gamma)
    R = J = 0.0
    L = 0
    rc, lc = r.cpu().numpy(), last.cpu().numpy()
    for e in range(N):
        j1 = jg = 0.0
        k = 0
        for t in range(T):
            j1 += float(rc[t, e])
            jg += gamma ** k * float(rc[t, e])
            k += 1
            if lc[t, e]:
                R, J, L = R + j1, J + jg, L + k
                j1, jg, k = 0.0, 0.0, 0
        assert j1 == 0.0                                          # what is left open past the quota returns nothing
    assert o["n_steps"] == L
    for name, want in (("R_mean", R / 50), ("J_mean", J / 50), ("L", L / 50)):
        assert abs(o[name] - want) <= 1e-12 * abs(want), (name, o[name], want)
    # the rows past a quota were zeroed, not the ones inside it
    raw = b["reward_raw"][:T]
    keep = (torch.cumsum(b["last_raw"][:T].long(), 0) - b["last_raw"][:T].long()) < torch.tensor(
        [2, 2] + [1] * 46, device=raw.device)[None]
    assert torch.equal(b["reward"][keep], raw[keep]) and bool((b["reward"][~keep] == 0).all())


# ------------------------------------------------------------------------------ 7. a physics that consumes controls
def test_step_takes_the_policy_s_controls():
    """VecLocoEnv.step(actions, ctrl=) hands the given controls to a physics with needs_ctrl and skips the K1 pre-pass;
    they are the pre-pass' own bits, and ILCore passes them on every step."""
    from olympic_hip import specs
    from olympic_hip.envs import KinematicPhysics, LocoEnvBase
    from olympic_hip.il_core import ILCore

    class CtrlPhysics(KinematicPhysics):
        needs_ctrl = True

        def __init__(self, *a):
            super().__init__(*a)
            self.seen = []

        def step(self, ctrl):
            self.seen.append(ctrl)
            return super().step(ctrl)

    N = 17
    phys = CtrlPhysics(specs.unitree_h1("walk"), N, torch.device("cuda", 0))
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=N, seed=1, physics=phys)
    vec, eng = env.vec, env.vec.eng
    try:
        vec.spec.horizon = vec.info.horizon = 4
        vec.reset()
        a = (torch.randn((N, 11), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 2).contiguous()
        calls = []
        il_step0 = eng.il_step

        def il_step(*args, **kw):
            calls.append(1)
            return il_step0(*args, **kw)
        eng.il_step = il_step
        vec.step(a)                                               # the pre-pass forms the controls: two K1 passes
        n_default = len(calls)
        given = eng.il_ctrl(a)
        vec.step(a, ctrl=given)
        eng.il_step = il_step0
        torch.cuda.synchronize()
        assert n_default == 2 and len(calls) == 3                 # the second step ran K1 once
        assert phys.seen[1] is given and torch.equal(phys.seen[0], given)
        assert bool((given.abs() == 0.95).any())                  # clamped entries among them
        with pytest.raises(Exception):
            vec.step(a, ctrl=given[:, :5])
        # the core passes the policy's controls on every step
        pol = _policy(eng, vec.spec.n_obs, vec.spec.n_act, 7, std_0=2.0)
        agent = RecordingAgent()
        phys.seen.clear()
        ILCore(agent, vec, pol, generator=torch.Generator(device="cuda").manual_seed(1)).learn(6, 6)
        torch.cuda.synchronize()
        assert len(phys.seen) == 6
        for t in range(6):
            assert torch.equal(phys.seen[t], eng.il_ctrl(agent.fits[0]["action"][t].contiguous())), t
    finally:
        torch.cuda.synchronize()
        eng.ctx.close()
