"""K27 on the MI355X: oly_iq_pi_update and oly_iq_alpha_update against the float64 restatement of tests/iq_pi_restate.py
over the issue's shapes, their bits (against oly_sg_act, oly_ilmlp_forward and oly_ilmlp_pack, across runs, the critic's),
the three reference-run fixtures through DeviceIQSAC / DeviceSQILSAC, fenced and poisoned operands, the refusals, and
checkpoint / resume.

Tolerances: TOL = 2e-5 against float64 for the sweep (tests/test_iq_pi_cpu.py holds torch's own float32 run of the same
table within a quarter of that); for a fixture max(2e-5, 4 x the stored |reference float32 - float64 twin|)
(tests/golden/gen_iq_pi_update.py's docstring)."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import torch

import iq_pi_restate as R
from fences import Fenced, assert_intact, assert_untouched, assert_written, fenced

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = R.TOL
SHAPES, CONFIGS, cfg_id, cat = R.SHAPES, R.CONFIGS, R.cfg_id, R.cat


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def shapes_of(in_dim, out_dim):
    return [(512, in_dim), (512,), (256, 512), (256,), (out_dim, 256), (out_dim,)]


def split(a, in_dim, out_dim):
    out, o = [], 0
    for s in shapes_of(in_dim, out_dim):
        n = int(np.prod(s))
        out.append(a[o:o + n].reshape(s))
        o += n
    return out


class Dev:
    """Both networks' state in fenced device buffers, the workspace of exactly the reported size."""

    def __init__(self, eng, case, cfg, in_dim, A, Bp):
        from olympic_hip._ffi import lib
        self.eng, self.cfg, self.in_dim, self.A, self.Bp, self.D = eng, cfg, in_dim, A, Bp, in_dim + A
        flat = np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in case["pparams"]])
        cflat = np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in case["cparams"]])
        z = np.zeros_like(flat)
        npk = int(lib().oly_ilmlp_packed_floats(in_dim, 512, 256, 2 * A))
        ncpk = int(lib().oly_ilmlp_packed_floats(self.D, 512, 256, 1))
        self.nws = int(lib().oly_iq_pi_ws(Bp, in_dim, A))
        self.f = dict(param=fenced(flat), m=fenced(z), v=fenced(z), packed=Fenced(npk, torch.float32),
                      critic_param=fenced(cflat), critic_packed=Fenced(ncpk, torch.float32),
                      central=fenced(case["central"]), delta=fenced(case["delta"]),
                      ws=Fenced(self.nws, torch.float32), out=Fenced(4, torch.float64),
                      action=Fenced((Bp, A), torch.float32), log_prob=Fenced(Bp, torch.float32),
                      colstats=fenced(np.zeros((3, in_dim))) if cfg.standardizer else None,
                      critic_colstats=fenced(np.zeros((3, self.D))) if cfg.standardizer else None)
        eng.ilmlp_pack(*split(self.t("param"), in_dim, 2 * A), packed=self.t("packed"))
        eng.ilmlp_pack(*split(self.t("critic_param"), self.D, 1), packed=self.t("critic_packed"))
        self.step = 0
        self.inputs = {}

    def t(self, k):
        return None if self.f[k] is None else self.f[k].t

    def update(self, s, alpha=R.ALPHA):
        c = self.cfg
        self.inputs = {k: fenced(np.asarray(v, np.float32)) for k, v in s.items()}
        o = self.eng.iq_pi_update(self.inputs["x"].t, self.inputs["eps"].t, self.t("central"), self.t("delta"),
                                  self.t("colstats"), self.t("param"), self.t("m"), self.t("v"), self.t("packed"),
                                  self.t("critic_packed"), self.t("critic_param"), self.t("critic_colstats"), self.t("ws"),
                                  self.step, c.lr, alpha=alpha, log_std_min=c.ls_min, log_std_max=c.ls_max,
                                  adam_eps=c.adam_eps, weight_decay=c.wd,
                                  out=dict(action=self.t("action"), log_prob=self.t("log_prob"), out=self.t("out")))
        self.step += 1
        return o["out"].clone()

    def check_fences(self, what):
        assert_intact(self.f, what)
        assert_intact(self.inputs, what)

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: None if f is None else f.t.clone() for k, f in self.f.items() if k != "ws"}


# ------------------------------------------------------------------------------ against the float64 yardstick
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["-".join(map(str, s)) for s in SHAPES])
def test_update_against_float64(eng, k):
    """Shape k of the issue's table, three consecutive updates, with both Standardizers and a weight decay and without."""
    in_dim, A, Bp = SHAPES[k]
    case = R.sweep_inputs(k)
    for j, cfg in enumerate(CONFIGS):
        ref, ref_out, ref_acts = R.yardstick(k, j)[:3]
        dev = Dev(eng, case, cfg, in_dim, A, Bp)
        out = np.stack([dev.update(s).cpu().numpy() for s in case["steps"]])
        got = dev.snapshot()
        dev.check_fences(cfg_id(cfg))
        who = f"{SHAPES[k]} {cfg_id(cfg)}"
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
        a_ref, lp_ref = ref_acts[-1]                         # the last update's action and log-probability
        assert float(np.abs(got["action"].double().cpu().numpy() - a_ref).max()) <= TOL, who
        assert float(np.abs(got["log_prob"].double().cpu().numpy() - lp_ref).max()) <= TOL * max(1.0, np.abs(lp_ref).max()), who
        if cfg.standardizer:
            for key, want in (("colstats", ref["policy"]["colstats"]), ("critic_colstats", ref["critic"]["colstats"])):
                a = got[key].cpu().numpy()
                assert np.array_equal(a[0], want[0]), (who, key, "counts")
                assert np.all(np.abs(a - want) <= TOL * np.maximum(1.0, np.abs(want))), (who, key)
        assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim, 2 * A)))


# ------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("k", (1, 4), ids=("12-5-18", "48-16-33"))
@pytest.mark.parametrize("standardizer", (False, True), ids=("nostd", "std"))
def test_the_calls_bits(eng, k, standardizer):
    """action and log_prob are oly_sg_act's on the same rows, noise and starting statistics; the workspace's Q is
    oly_ilmlp_forward's on (x | a_new) with the statistics the call leaves; packed is a fresh pack of param; the critic's
    parameters and stream keep their bytes; a second run gives the same bits."""
    from olympic_hip._ffi import lib
    in_dim, A, Bp = SHAPES[k]
    case, cfg = R.sweep_inputs(k), CONFIGS[0 if standardizer else 1]
    start = None
    if standardizer:     # statistics that already hold rows: (count, sum, sumsq) of 7 earlier ones
        rng = np.random.default_rng(3)
        x0 = rng.standard_normal((7, in_dim)) * 2 + 1
        start = np.stack([np.full(in_dim, 7.0), x0.sum(0), np.square(x0).sum(0)])
    snaps = []
    for _ in range(2):
        dev = Dev(eng, case, cfg, in_dim, A, Bp)
        if standardizer:
            dev.t("colstats").copy_(torch.as_tensor(start))
        before = dev.snapshot()
        s = case["steps"][0]
        dev.update(s)
        got = dev.snapshot()
        dev.check_fences("bits")
        want = eng.sg_act(dev.inputs["x"].t, before["packed"], dev.t("central"), dev.t("delta"),
                          colstats=None if not standardizer else torch.as_tensor(start).cuda(), eps=dev.inputs["eps"].t,
                          update_stats=standardizer, log_std_min=cfg.ls_min, log_std_max=cfg.ls_max)
        assert torch.equal(got["action"], want["action"])
        assert torch.equal(got["log_prob"], want["log_prob"])
        off = int(lib().oly_iq_pi_ws_values(Bp, in_dim, A))
        xa = torch.cat([dev.inputs["x"].t, got["action"]], dim=1).contiguous()
        q = eng.ilmlp_forward(xa, got["critic_packed"], 1, colstats=got["critic_colstats"]).reshape(-1)
        assert torch.equal(dev.t("ws")[off:off + Bp], q)
        assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim, 2 * A)))
        assert not torch.equal(got["param"], before["param"])
        for key in ("critic_param", "critic_packed", "central", "delta"):
            assert torch.equal(got[key], before[key]), key
        snaps.append(got)
    for key, a in snaps[0].items():
        if a is not None:
            assert torch.equal(a.view(torch.uint8), snaps[1][key].view(torch.uint8)), key


# ------------------------------------------------------------------------------ the temperature
@pytest.mark.parametrize("n", (1, 9, 18))
def test_alpha_update_against_float64(eng, n):
    rng = np.random.default_rng(50 + n)
    lps = [(rng.standard_normal(n) * 2 - 1).astype(np.float32) for _ in range(3)]
    te, lr, init = -5.0, 3e-4, 0.2
    state = fenced(np.array([np.float32(np.log(init)), 0, 0], np.float32))
    inputs = []
    for step, lp in enumerate(lps):
        inputs.append(fenced(lp))
        eng.iq_alpha_update(inputs[-1].t, state.t, step, lr, te)
    torch.cuda.synchronize()
    assert_intact(dict(state=state, **{f"lp{i}": f for i, f in enumerate(inputs)}), "alpha")
    got, want = state.t.double().cpu().numpy(), R.alpha_adam(lps, te, lr, init=init)
    print(f"n={n}: block {got}, float64 {want}")
    assert abs(got[0] - want[0]) <= TOL, (got, want)                          # log_alpha
    assert np.all(np.abs(got[1:] - want[1:]) <= TOL * np.abs(want[1:])), (got, want)   # the moments, relative to their size


# ------------------------------------------------------------------------------ fences, stores, refusals
@pytest.mark.parametrize("Bp", (18, 1))
def test_fenced_operands_and_stores(eng, Bp):
    in_dim, A = 12, 5
    case = R.case_inputs(in_dim, A, Bp, seed=9, updates=1)
    for cfg in CONFIGS:
        dev = Dev(eng, case, cfg._replace(wd=1e-3), in_dim, A, Bp)
        before = dev.snapshot()
        dev.update(case["steps"][0])
        after = dev.snapshot()
        dev.check_fences(cfg_id(cfg))
        assert_written({k: dev.f[k] for k in ("out", "action", "log_prob", "packed")}, cfg_id(cfg))
        for key in ("param", "m", "v"):                        # weight decay: every element has a gradient and moves
            assert bool((after[key] != before[key]).all()), key
            assert bool(torch.isfinite(after[key]).all()), key
        for key in ("out", "action", "log_prob", "colstats", "critic_colstats"):
            assert after[key] is None or bool(torch.isfinite(after[key]).all()), key
    # the alpha call: every input fenced, the block stored whole
    lp, state = fenced(np.linspace(-3, 1, Bp).astype(np.float32)), Fenced(3, torch.float32)
    state.t.copy_(torch.tensor([-1.5, 0.0, 0.0]))
    eng.iq_alpha_update(lp.t, state.t, 0, 3e-4, -float(A))
    torch.cuda.synchronize()
    assert_intact(dict(lp=lp, state=state), "alpha")
    assert bool(torch.isfinite(state.t).all()) and float(state.t[1]) != 0.0 and float(state.t[2]) != 0.0


def test_refusals_come_before_any_launch(eng):
    from olympic_hip import _abi
    from olympic_hip._ffi import lib
    in_dim, A, B = 12, 5, 18
    D = in_dim + A
    n_par = 512 * in_dim + 512 + 256 * 512 + 256 + 2 * A * 256 + 2 * A
    n_cpar = 512 * D + 512 + 256 * 512 + 256 + 256 + 1
    npk = int(lib().oly_ilmlp_packed_floats(in_dim, 512, 256, 2 * A))
    ncpk = int(lib().oly_ilmlp_packed_floats(D, 512, 256, 1))
    nws = int(lib().oly_iq_pi_ws(B, in_dim, A))
    f32, f64 = torch.float32, torch.float64
    bufs = dict(x=Fenced((B, in_dim), f32), eps=Fenced((B, A), f32), central=Fenced(A, f32), delta=Fenced(A, f32),
                colstats=Fenced((3, in_dim), f64), param=Fenced(n_par, f32), m=Fenced(n_par, f32), v=Fenced(n_par, f32),
                packed=Fenced(npk, f32), critic_packed=Fenced(ncpk, f32), critic_param=Fenced(n_cpar, f32),
                critic_colstats=Fenced((3, D), f64), ws=Fenced(nws, f32), action=Fenced((B, A), f32),
                log_prob=Fenced(B, f32), out=Fenced(4, f64))

    def block(**over):
        kw = dict(in_dim=in_dim, act_dim=A, batch=B, step=0, alpha=1e-3, log_std_min=-20.0, log_std_max=2.0, lr=3e-4,
                  beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0, packed_floats=npk, critic_packed_floats=ncpk,
                  ws_floats=nws)
        kw.update({k: b.t.data_ptr() for k, b in bufs.items()})
        kw.update(over)
        return _abi.IQPi(**kw)
    bad = dict(batch_0=dict(batch=0), batch_big=dict(batch=4097), in_0=dict(in_dim=0), act_0=dict(act_dim=0),
               act_17=dict(act_dim=17), wide=dict(in_dim=60), step=dict(step=-1),
               ls=dict(log_std_min=1.0, log_std_max=0.0), ls_nan=dict(log_std_min=float("nan")),
               ws_short=dict(ws_floats=nws - 1), ws_misaligned=dict(ws=bufs["ws"].t.data_ptr() + 4),
               packed_misaligned=dict(packed=bufs["packed"].t.data_ptr() + 4), packed_short=dict(packed_floats=npk - 1),
               critic_short=dict(critic_packed_floats=ncpk - 1),
               critic_misaligned=dict(critic_packed=bufs["critic_packed"].t.data_ptr() + 4))
    for k in ("x", "eps", "central", "delta", "param", "m", "v", "packed", "critic_packed", "critic_param", "ws", "action",
              "log_prob", "out"):
        bad["null_" + k] = {k: None}
    L = lib()
    for name, over in bad.items():
        f = block(**over)
        rc = L.oly_iq_pi_update(eng.ctx.handle, C.byref(f), eng._s())
        assert rc == _abi.OLY_EINVAL, (name, rc)
    assert L.oly_iq_pi_update(eng.ctx.handle, None, eng._s()) == _abi.OLY_EINVAL
    assert int(L.oly_iq_pi_ws(0, in_dim, A)) == -1 and int(L.oly_iq_pi_ws(B, 60, A)) == -1
    assert int(L.oly_iq_pi_ws(1, 1, 1)) > 0 and int(L.oly_iq_pi_ws_values(B, 60, A)) == -1
    # the alpha call
    ab = dict(log_prob=Fenced(B, f32), state=Fenced(3, f32))

    def ablock(**over):
        kw = dict(n=B, step=0, target_entropy=-5.0, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, pad=0.0,
                  log_prob=ab["log_prob"].t.data_ptr(), state=ab["state"].t.data_ptr())
        kw.update(over)
        return _abi.IQAlpha(**kw)
    for name, over in dict(n_0=dict(n=0), n_neg=dict(n=-3), step=dict(step=-1), null_state=dict(state=None),
                           null_lp=dict(log_prob=None)).items():
        f = ablock(**over)
        assert L.oly_iq_alpha_update(eng.ctx.handle, C.byref(f), eng._s()) == _abi.OLY_EINVAL, name
    assert L.oly_iq_alpha_update(eng.ctx.handle, None, eng._s()) == _abi.OLY_EINVAL
    torch.cuda.synchronize()
    assert_untouched(bufs, "refused calls")
    assert_untouched(ab, "refused alpha calls")


# ------------------------------------------------------------------------------ the reference-run fixtures
def build_agent(eng, g, name, sw=None, logging_iter=1):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceIQSAC, DeviceSoftQCritic, DeviceSQILSAC
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_iq_pi_update as gen
    gq = gen.gq

    def lins(prefix, dims, seed):
        out = [torch.nn.Linear(i, o) for i, o in dims]
        with torch.no_grad():
            for lin, (w, b) in zip(out, (("w1", "b1"), ("w2", "b2"), ("w3", "b3"))):
                lin.weight.copy_(torch.as_tensor(gq.w2_init(seed) if w == "w2" else g[f"{prefix}_{w}"]))
                lin.bias.copy_(torch.as_tensor(g[f"{prefix}_{b}"]))
        return out
    A, in_dim, D = gen.ACT_DIM, gen.IN_DIM, gen.D
    policy = DeviceSquashedGaussianPolicy(eng, lins("policy_init", [(in_dim, 512), (512, 256), (256, 2 * A)], 11), g["min_a"],
                                          g["max_a"], standardizer=DeviceStandardizer(eng, in_dim),
                                          log_std_min=gq.LOG_STD_MIN, log_std_max=gq.LOG_STD_MAX)
    critic = DeviceSoftQCritic(eng, lins("critic_init", [(D, 512), (512, 256), (256, 1)], 12),
                               standardizer=DeviceStandardizer(eng, D), lr=float(g["lr"]), tau=float(g["tau"]))
    demo = dict(states=np.zeros((4, in_dim), np.float32), actions=np.zeros((4, A), np.float32),
                next_states=np.zeros((4, in_dim), np.float32), absorbing=np.zeros(4, np.float32))
    spec = gen.FIXTURES[name]
    kw = dict(gamma=float(g["gamma"]), batch_size=gen.N_POLICY, use_target=spec["use_target"], init_alpha=gq.INIT_ALPHA,
              reg_mult=float(g["reg_mult"]), plcy_loss_mode=spec["mode"], logging_iter=logging_iter, sw=sw,
              max_replay_size=64, actor_optimizer=dict(lr=float(g["lr_actor"])),
              train_policy_only_on_own_states=spec["own_states"], learnable_alpha=spec["learnable"],
              lr_alpha=float(g["lr_alpha"]), target_entropy=float(g["target_entropy"]))
    if spec["algo"] == "iq":
        agent = DeviceIQSAC(eng, policy, critic, demo, regularizer_mode=spec["reg"], **kw)
    else:
        agent = DeviceSQILSAC(eng, policy, critic, demo, R_min=0.0, R_max=1.0, **kw)
    agent.replay.add(dict(demo))          # iq_update asks replay.size > warmup_transitions (0)
    return agent, gen


class Recorder:
    def __init__(self):
        self.rows = {}

    def add_scalar(self, name, val, it):
        self.rows.setdefault(int(it), {})[name] = float(val)


def run_fixture(agent, g, first, last):
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    for i in range(first, last):
        eps = dict(q=dict(next=d(g["eps_next"][i]), pi=d(g["eps_pi"][i]), expert=d(g["eps_expert"][i])),
                   pi=dict(pi=d(g["eps_ppi"][i]), log=d(g["eps_plog"][i])))
        agent.iq_update(d(g["obs"][i]), d(g["act"][i]), d(g["next_obs"][i]), d(g["absorbing"][i]), int(g["n_policy"]),
                        eps=eps)
        agent._iter += 1                      # fit's counters (iq_sac.py:405-406)
        agent.policy.iter = getattr(agent.policy, "iter", 0) + 1


@pytest.mark.parametrize("name", ("iq", "iq_own_states_alpha", "sqil"))
def test_fixture_through_the_agent(eng, golden, name):
    g = golden(f"iq_pi_update/{name}.npz")
    sw = Recorder()
    agent, gen = build_agent(eng, g, name, sw=sw)
    run_fixture(agent, g, 0, gen.N_ITER)
    torch.cuda.synchronize()
    c, p = agent.critic, agent.policy
    for flat, prefix, sp, shp in ((p.param, "policy", g["spread_policy"], (gen.IN_DIM, 2 * gen.ACT_DIM)),
                                  (c.param, "critic", g["spread_critic"], (gen.D, 1))):
        tol = max(TOL, 4 * float(sp))
        got = dict(zip(R.NAMES, split(flat.double().cpu().numpy(), *shp)))
        for n in R.NAMES:
            a, r = (got[n][:gen.W2_HEAD], g[f"{prefix}_w2_head"]) if n == "w2" else (got[n], g[f"{prefix}_{n}"])
            err = float(np.abs(a - r).max())
            print(f"{name} {prefix} {n}: {err:.3e} (tolerance {tol:.3e})")
            assert err <= tol, (prefix, n, err)
    # every Actor/... and Gradients/... scalar of update_policy, from the writer
    scal = g["scalars"]
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * float(g["spread_scalars"]))
    for i in range(gen.N_ITER):
        row = sw.rows[i + 1]
        for k, t in enumerate(gen.ACTOR_TAGS):
            assert abs(row[t] - scal[i, k]) <= tol[i, k], (i, t, row[t], scal[i, k])
    # the Standardizers: counts exact (the policy's pins step 5's three extra passes), sums within the stored tolerances
    for got, want, sp in ((p.stand.colstats, g["policy_colstats"], g["spread_policy_stats"]),
                          (c.stand.colstats, g["colstats"], g["spread_critic_stats"])):
        a = got.cpu().numpy()
        assert np.array_equal(a[0], want[0]), (a[0], want[0])
        assert np.all(np.abs(a - want) <= np.maximum(TOL * np.maximum(1.0, np.abs(want)), 4 * float(sp)))
    Bp = gen.N_POLICY if gen.FIXTURES[name]["own_states"] else gen.B
    assert float(p.stand.colstats[0, 0]) == gen.N_ITER * (4 * gen.B + (gen.B - gen.N_POLICY) + Bp)
    err = R.alpha_err(agent.alpha_state.double().cpu().numpy(), g["alpha_block"])
    print(f"{name} alpha block: {err:.3e}")
    assert err <= max(TOL, 4 * float(g["spread_alpha"]))
    assert agent.pi_step == gen.N_ITER and agent.alpha_step == (gen.N_ITER if gen.FIXTURES[name]["learnable"] else 0)


# ------------------------------------------------------------------------------ checkpoint / resume
def test_a_saved_run_resumes_to_the_same_bits(eng, golden, tmp_path):
    name = "iq_own_states_alpha"
    g = golden(f"iq_pi_update/{name}.npz")
    whole, gen = build_agent(eng, g, name)
    run_fixture(whole, g, 0, 4)
    first, _ = build_agent(eng, g, name)
    run_fixture(first, g, 0, 2)
    path = first.save(str(tmp_path / "iq.pt"), note="after iq_update 2")
    resumed, _ = build_agent(eng, g, name)
    ptrs = lambda a: [t.data_ptr() for t in (a.policy.param, a.policy.packed, a.critic.param, a.pi_exp_avg, a.alpha_state)]
    before = ptrs(resumed)
    assert resumed.load(path)["note"] == "after iq_update 2"
    assert resumed._iter == 3 and resumed.pi_step == 2 and resumed.alpha_step == 2 and resumed.critic.step == 2
    assert before == ptrs(resumed)
    run_fixture(resumed, g, 2, 4)
    torch.cuda.synchronize()
    for key in ("param", "target_param", "exp_avg", "exp_avg_sq", "packed", "target_packed"):
        assert torch.equal(getattr(whole.critic, key), getattr(resumed.critic, key)), key
    for key in ("param", "packed"):
        assert torch.equal(getattr(whole.policy, key), getattr(resumed.policy, key)), key
    for key in ("pi_exp_avg", "pi_exp_avg_sq", "alpha_state"):
        assert torch.equal(getattr(whole, key), getattr(resumed, key)), key
    assert torch.equal(whole.critic.stand.colstats, resumed.critic.stand.colstats)
    assert torch.equal(whole.critic.target_stand.colstats, resumed.critic.target_stand.colstats)
    assert torch.equal(whole.policy.stand.colstats, resumed.policy.stand.colstats)
    for k, v in whole.replay.blocks.items():
        assert torch.equal(v, resumed.replay.blocks[k]), k
    assert whole._iter == resumed._iter == 5 and whole.alpha == resumed.alpha
