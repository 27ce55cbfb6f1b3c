"""K26 on the MI355X: oly_iq_q_update against the float64 restatement of tests/iq_restate.py over its shapes and every
loss mode, its bits (against oly_ilmlp_forward, across runs, the target's), the three reference-run fixtures through
DeviceIQLearn / DeviceSQIL, fenced and poisoned operands, the refusals, and checkpoint / resume.

Tolerances (tests/golden/gen_iq_q_update.py's docstring): 4 x the float32-against-float64 spread of the same update, never
below 2e-5 for the parameters.  For a fixture the spread is the stored one; for a case of the sweep it is measured here
by running the restatement in float32 as well."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import torch

import iq_restate as R
from fences import Fenced, assert_intact, assert_untouched, assert_written, fenced

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = R.TOL
SHAPES, CONFIGS, UPDATES, cfg_id, cat = R.SHAPES, R.CONFIGS, R.UPDATES, R.cfg_id, R.cat


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


class Dev:
    """The critic's state in fenced device buffers, the workspace of exactly the reported size."""

    def __init__(self, eng, params, cfg, in_dim, A, B, target=None):
        from olympic_hip._ffi import lib
        self.eng, self.cfg, self.in_dim, self.A, self.B, self.D = eng, cfg, in_dim, A, B, in_dim + A
        flat = np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in params])
        tflat = flat if target is None else np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in target])
        z = np.zeros_like(flat)
        npk = int(lib().oly_ilmlp_packed_floats(self.D, 512, 256, 1))
        self.nws = int(lib().oly_iq_q_ws(B, in_dim, A))
        self.f = dict(param=fenced(flat), m=fenced(z), v=fenced(z), target_param=fenced(tflat),
                      packed=Fenced(npk, torch.float32), target_packed=Fenced(npk, torch.float32),
                      ws=Fenced(self.nws, torch.float32), out=Fenced(16, torch.float64),
                      colstats=fenced(np.zeros((3, self.D))) if cfg.standardizer else None,
                      target_colstats=fenced(np.zeros((3, self.D))) if cfg.standardizer else None)
        eng.ilmlp_pack(*self.views("param"), packed=self.f["packed"].t)
        eng.ilmlp_pack(*self.views("target_param"), packed=self.f["target_packed"].t)
        self.step = 0
        self.inputs = {}

    def t(self, k):
        return None if self.f[k] is None else self.f[k].t

    def views(self, k):
        flat, out, o = self.f[k].t, [], 0
        for s in [(512, self.D), (512,), (256, 512), (256,), (1, 256), (1,)]:
            n = int(np.prod(s))
            out.append(flat[o:o + n].view(s))
            o += n
        return out

    def update(self, s, n_policy, **over):
        c = self.cfg
        self.inputs = {k: fenced(np.asarray(v, np.float32)) for k, v in s.items()}
        i = {k: v.t for k, v in self.inputs.items()}
        kw = dict(algo=c.algo, plcy_loss_mode=c.mode, regularizer_mode=c.reg, treat_absorbing=c.treat,
                  use_target=c.use_target, update_target=c.update_target, gamma=c.gamma, alpha=c.alpha, reg_mult=c.reg_mult,
                  R_min=c.R_min, R_max=c.R_max, tau=c.tau, weight_decay=c.wd, eps=c.adam_eps)
        kw.update(over)
        self.eng.iq_q_update(i["obs"], i["act"], i["next_obs"], i["absorbing"], i["a_next"], i["logp_next"], i["a_pi"],
                             i["logp_pi"], n_policy, self.t("colstats"), self.t("target_colstats"), self.t("param"),
                             self.t("m"), self.t("v"), self.t("packed"), self.t("target_param"), self.t("target_packed"),
                             self.t("ws"), self.step, c.lr, out=self.t("out"), **kw)
        self.step += 1
        return self.t("out").clone()

    def check_fences(self, what):
        assert_intact(self.f, what)
        assert_intact(self.inputs, what)

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: None if f is None else f.t.clone() for k, f in self.f.items() if k != "ws"}


def split(a, D):
    out, o = [], 0
    for s in [(512, D), (512,), (256, 512), (256,), (1, 256), (1,)]:
        n = int(np.prod(s))
        out.append(a[o:o + n].reshape(s))
        o += n
    return out


# ------------------------------------------------------------------------------ against the float64 yardstick
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["-".join(map(str, s)) for s in SHAPES])
def test_update_against_float64(eng, k):
    """Shape k of the issue's table with the configs tests/iq_restate.py gives it: over the five shapes every loss mode,
    regularizer mode, treat_absorbing, use_target and SQIL mode is run, with and without Standardizers."""
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = R.sweep_inputs(k)
    for j, cfg in R.sweep(k):
        ref, ref_out, f32, f32_out = R.yardstick(k, j)
        dev = Dev(eng, params, cfg, in_dim, A, B)
        out = np.stack([dev.update(s, n_policy).cpu().numpy() for s in steps])
        got = dev.snapshot()
        dev.check_fences(cfg_id(cfg))
        who = f"{SHAPES[k]} {cfg_id(cfg)}"
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
                assert np.array_equal(a[0], r[0]), (who, key, "counts")
                assert np.all(np.abs(a - r) <= 1e-12 * np.maximum(1.0, np.abs(r))), (who, key)
        spread = np.abs(f32_out - ref_out)
        tol = np.maximum(TOL * np.maximum(1.0, np.abs(ref_out)), 4 * np.where(np.isnan(spread), 0.0, spread))
        assert np.array_equal(np.isnan(out), np.isnan(ref_out)), (who, out, ref_out)
        bad = ~(np.abs(out - ref_out) <= tol) & ~np.isnan(ref_out)
        print(f"{who} scalars: worst |kernel - f64| / tolerance {np.nanmax(np.abs(out - ref_out) / tol):.3f}")
        assert not bad.any(), (who, np.argwhere(bad), out[bad], ref_out[bad])
        assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim + A)))
        assert torch.equal(got["target_packed"], eng.ilmlp_pack(*split(got["target_param"], in_dim + A)))


# ------------------------------------------------------------------------------ bits
def exact_inputs(in_dim, A, B, seed):
    """One update's inputs on a grid of 1/8, so that the Standardizer's float64 sums are exact in any order."""
    steps, params = R.case_inputs(in_dim, A, B, seed=seed, updates=1)
    s = steps[0]
    for k in ("obs", "act", "next_obs", "a_next", "a_pi"):
        s[k] = (np.round(s[k] * 8) / 8).astype(np.float32)
    return s, params


@pytest.mark.parametrize("standardizer", (False, True), ids=("nostd", "std"))
def test_q_values_have_the_forward_kernels_bits(eng, standardizer):
    check_q_values_have_the_forward_kernels_bits(eng, (12, 5, 18, 9), standardizer)


def check_q_values_have_the_forward_kernels_bits(eng, shape, standardizer):
    """The raw outputs of the three passes in the workspace against oly_ilmlp_forward on the same rows with the statistics
    the Standardizer holds at each pass (tests/test_gpu_iq_big_shapes.py runs it at a larger shape)."""
    from olympic_hip._ffi import lib
    in_dim, A, B, n_policy = shape
    s, params = exact_inputs(in_dim, A, B, seed=3)
    for use_target in (True, False):
        cfg = R.Cfg(use_target=use_target, standardizer=standardizer)
        dev = Dev(eng, params, cfg, in_dim, A, B)
        packed0 = dev.t("packed").clone()
        dev.update(s, n_policy)
        torch.cuda.synchronize()
        off, BP = int(lib().oly_iq_q_ws_values(B, in_dim, A)), (B + 15) // 16 * 16
        qv = dev.t("ws")[off:off + 3 * BP].view(3, BP)[:, :B]
        x0 = np.concatenate([s["obs"], s["act"]], 1)
        x1 = np.concatenate([s["next_obs"], s["a_next"]], 1)
        x2 = np.concatenate([s["obs"], s["a_pi"]], 1)
        st = lambda xs: torch.as_tensor(sum(np.stack([np.full(x.shape[1], float(len(x))), x.astype(np.float64).sum(0),
                                                      np.square(x.astype(np.float64)).sum(0)]) for x in xs)).cuda()
        c0 = st([x0]) if standardizer else None
        c2 = st([x0, x2] if use_target else [x0, x1, x2]) if standardizer else None
        want_q = eng.ilmlp_forward(torch.as_tensor(x0).cuda(), packed0, 1, colstats=c0).reshape(-1)
        want_v = eng.ilmlp_forward(torch.as_tensor(x2).cuda(), packed0, 1, colstats=c2).reshape(-1)
        assert torch.equal(qv[0], want_q), use_target
        assert torch.equal(qv[2], want_v), use_target
        if not use_target:
            c1 = st([x0, x1]) if standardizer else None
            assert torch.equal(qv[1], eng.ilmlp_forward(torch.as_tensor(x1).cuda(), packed0, 1, colstats=c1).reshape(-1))


def test_two_runs_give_the_same_bits(eng):
    in_dim, A, B, n_policy = 32, 11, 48, 24
    steps, params = R.case_inputs(in_dim, A, B, seed=4, updates=UPDATES)
    for cfg in (R.Cfg(use_target=False, wd=1e-4), R.Cfg(algo="sqil", mode="value")):
        snaps = []
        for _ in range(2):
            dev = Dev(eng, params, cfg, in_dim, A, B)
            outs = [dev.update(s, n_policy) for s in steps]
            snaps.append((dev.snapshot(), torch.stack(outs)))
        for key, a in snaps[0][0].items():
            assert a is None or torch.equal(a, snaps[1][0][key]), key
        assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))


def test_the_targets_bits(eng):
    in_dim, A, B, n_policy = 12, 5, 18, 9
    steps, params = R.case_inputs(in_dim, A, B, seed=5, updates=1)
    target = [p + np.float32(0.01) for p in params]
    # update_target = 0 leaves the target's bits
    dev = Dev(eng, params, R.Cfg(update_target=False), in_dim, A, B, target=target)
    before = dev.snapshot()
    dev.update(steps[0], n_policy)
    after = dev.snapshot()
    assert torch.equal(before["target_param"], after["target_param"])
    assert torch.equal(before["target_packed"], after["target_packed"])
    assert not torch.equal(before["param"], after["param"])
    # tau = 1: the target is the stepped parameters
    dev = Dev(eng, params, R.Cfg(tau=1.0), in_dim, A, B, target=target)
    dev.update(steps[0], n_policy)
    got = dev.snapshot()
    assert torch.equal(got["target_param"], got["param"])
    assert torch.equal(got["target_packed"], eng.ilmlp_pack(*split(got["target_param"], in_dim + A)))
    # tau = 0.25 in float32: f32(tau) w + f32(1 - tau) t, two products and an add
    dev = Dev(eng, params, R.Cfg(tau=0.3), in_dim, A, B, target=target)
    t0 = dev.t("target_param").clone()
    dev.update(steps[0], n_policy)
    got = dev.snapshot()
    want = torch.tensor(np.float32(0.3)).cuda() * got["param"] + torch.tensor(np.float32(1 - 0.3)).cuda() * t0
    assert torch.equal(got["target_param"], want)


def test_a_target_keeps_the_next_state_pass_out_of_the_gradient(eng):
    """use_target with gamma = 0: y is 0 whatever the next-state pass gives, so another a_next changes nothing."""
    in_dim, A, B, n_policy = 12, 5, 18, 9
    steps, params = R.case_inputs(in_dim, A, B, seed=6, updates=1)
    other = dict(steps[0], a_next=-steps[0]["a_next"], logp_next=steps[0]["logp_next"] + 1)
    snaps = []
    for s in (steps[0], other):
        dev = Dev(eng, params, R.Cfg(gamma=0.0, standardizer=False), in_dim, A, B)
        out = dev.update(s, n_policy)
        snaps.append((dev.snapshot(), out))
    for key in ("param", "m", "v", "packed", "target_param"):
        assert torch.equal(snaps[0][0][key], snaps[1][0][key]), key
    assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))
    # without a target the pass carries a gradient: gamma > 0 and another a_next moves the parameters
    moved = []
    for s in (steps[0], other):
        dev = Dev(eng, params, R.Cfg(use_target=False, standardizer=False), in_dim, A, B)
        dev.update(s, n_policy)
        moved.append(dev.snapshot()["param"])
    assert not torch.equal(moved[0], moved[1])


# ------------------------------------------------------------------------------ the reference-run fixtures
def build_agent(eng, g, name, sw=None, logging_iter=1):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceIQLearn, DeviceSoftQCritic, DeviceSQIL
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_iq_q_update as gen

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
                                          log_std_min=gen.LOG_STD_MIN, log_std_max=gen.LOG_STD_MAX)
    critic = DeviceSoftQCritic(eng, lins("critic_init", [(D, 512), (512, 256), (256, 1)], 12),
                               standardizer=DeviceStandardizer(eng, D), lr=float(g["lr"]), tau=float(g["tau"]))
    demo = dict(states=np.zeros((4, in_dim), np.float32), actions=np.zeros((4, A), np.float32),
                next_states=np.zeros((4, in_dim), np.float32), absorbing=np.zeros(4, np.float32))
    spec = gen.FIXTURES[name]
    kw = dict(gamma=float(g["gamma"]), batch_size=gen.N_POLICY, use_target=spec["use_target"], init_alpha=gen.INIT_ALPHA,
              reg_mult=float(g["reg_mult"]), plcy_loss_mode=spec["mode"], logging_iter=logging_iter, sw=sw,
              max_replay_size=64)
    if spec["algo"] == "iq":
        return DeviceIQLearn(eng, policy, critic, demo, regularizer_mode=spec["reg"], **kw), gen
    return DeviceSQIL(eng, policy, critic, demo, R_min=0.0, R_max=1.0, **kw), gen


class Recorder:
    def __init__(self):
        self.rows = {}

    def add_scalar(self, name, val, it):
        self.rows.setdefault(int(it), {})[name] = float(val)


def run_fixture(agent, g, first, last):
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    outs = []
    for i in range(first, last):
        eps = dict(next=d(g["eps_next"][i]), pi=d(g["eps_pi"][i]), expert=d(g["eps_expert"][i]))
        outs.append(agent.update_Q_function(d(g["obs"][i]), d(g["act"][i]), d(g["next_obs"][i]), d(g["absorbing"][i]),
                                            int(g["n_policy"]), eps=eps))
        agent._iter += 1
    return outs


@pytest.mark.parametrize("name", ("iq_target", "iq_notarget", "sqil"))
def test_fixture_through_the_agent(eng, golden, name):
    from olympic_hip import _abi
    g = golden(f"iq_q_update/{name}.npz")
    sw = Recorder()
    agent, gen = build_agent(eng, g, name, sw=sw)
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
    tags = list(_abi.IQ_Q_TAGS)
    if gen.FIXTURES[name]["algo"] == "sqil":
        tags[0] = "IQ-Loss/LossQ"
    for i in range(gen.N_ITER):
        row = sw.rows[i + 1]
        for k, t in enumerate(tags):
            assert (t in row) == bool(logged[i, k]) or t in ("Action-Value/Q Absorbing state exp",
                                                             "Action-Value/Q Absorbing state plcy"), (i, t)
            if logged[i, k]:
                assert row[t] == out[i, k]
        for k, t in enumerate(gen.ACTION_TAGS):
            assert abs(row[t] - g["action_scalars"][i, k]) <= TOL * max(1.0, abs(g["action_scalars"][i, k])), (i, t)
    # The Standardizers.  The policy's after 4 iterations pins the extra pass of logging_loss: 4 x (18 + 9 + 18) rows.  The
    # reference sums the float32 rows in float32 before it adds to its float64 totals (networks.py:77-78): the counts are
    # exact, the sums within TOL of their own size (as test_gpu_bc_fit.py holds them) or 4 x the stored spread.
    st_tol = lambda r: np.maximum(TOL * np.maximum(1.0, np.abs(r)), 4 * float(g["spread_stats"]))
    for got, want in ((agent.policy.stand.colstats, g["policy_colstats"]), (c.stand.colstats, g["colstats"]),
                      (c.target_stand.colstats, g["target_colstats"])):
        a = got.cpu().numpy()
        assert np.array_equal(a[0], want[0]), (a[0], want[0])
        assert np.all(np.abs(a - want) <= st_tol(want))
    assert float(g["policy_colstats"][0, 0]) == gen.N_ITER * (2 * gen.B + gen.B - gen.N_POLICY)


# ------------------------------------------------------------------------------ fences, stores, refusals
@pytest.mark.parametrize("B,n_policy", ((18, 9), (2, 1)))
def test_fenced_operands_and_stores(eng, B, n_policy):
    in_dim, A = 12, 5
    steps, params = R.case_inputs(in_dim, A, B, seed=7, updates=1)
    for cfg in (R.Cfg(use_target=False, wd=1e-3, tau=0.5), R.Cfg(algo="sqil", mode="plcy", wd=1e-3, tau=0.5)):
        dev = Dev(eng, params, cfg, in_dim, A, B, target=[p + np.float32(0.01) for p in params])
        before = dev.snapshot()
        dev.f["out"] = Fenced(16, torch.float64)              # poisoned again
        s = dict(steps[0])
        if cfg.algo == "sqil":                                # plcy reads neither a_pi nor logp_pi: poisoned inputs
            s["a_pi"], s["logp_pi"] = np.full((B, A), np.nan, np.float32), np.full(B, np.nan, np.float32)
        dev.update(s, n_policy)
        after = dev.snapshot()
        dev.check_fences(cfg_id(cfg))
        assert_written(dict(out=dev.f["out"]), cfg_id(cfg))
        for key in ("param", "m", "v", "target_param"):       # weight decay: every element has a gradient and moves
            assert bool((after[key] != before[key]).all()), key
            assert bool(torch.isfinite(after[key]).all()), key
        assert torch.equal(after["packed"], eng.ilmlp_pack(*split(after["param"], in_dim + A)))
        assert torch.equal(after["target_packed"], eng.ilmlp_pack(*split(after["target_param"], in_dim + A)))
        out = after["out"]
        assert bool(torch.isfinite(out[:13]).all()) and bool(torch.isfinite(out[15]))
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

    def block(**over):
        kw = dict(in_dim=in_dim, act_dim=A, batch=B, n_policy=9, algo=0, plcy_loss_mode=0, regularizer_mode=0,
                  treat_absorbing=0, use_target=1, update_target=1, step=0, pad=0, gamma=0.99, alpha=1e-3, reg_mult=0.5,
                  R_min=0.0, R_max=1.0, gradient_penalty_lambda=0.0, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.0, pad2=0.0, tau=0.005, packed_floats=npk, target_packed_floats=npk, ws_floats=nws)
        kw.update({k: b.t.data_ptr() for k, b in bufs.items()})
        kw.update(over)
        return _abi.IQQ(**kw)
    bad = dict(batch_1=dict(batch=1, n_policy=1), batch_big=dict(batch=4097), in_0=dict(in_dim=0), act_17=dict(act_dim=17),
               wide=dict(in_dim=60), n_policy_0=dict(n_policy=0), n_policy_B=dict(n_policy=B), algo=dict(algo=2),
               mode=dict(plcy_loss_mode=5), mode_neg=dict(plcy_loss_mode=-1), v0=dict(plcy_loss_mode=_abi.IQ_PLCY_LOSS_MODES["v0"]),
               sqil_mode=dict(algo=1, plcy_loss_mode=3), reg=dict(regularizer_mode=4), gp=dict(gradient_penalty_lambda=0.5),
               tau_hi=dict(tau=1.5), tau_lo=dict(tau=-0.1), tau_nan=dict(tau=float("nan")), step=dict(step=-1),
               ws_short=dict(ws_floats=nws - 1), ws_misaligned=dict(ws=bufs["ws"].t.data_ptr() + 4),
               packed_misaligned=dict(packed=bufs["packed"].t.data_ptr() + 4), packed_short=dict(packed_floats=npk - 1),
               target_short=dict(target_packed_floats=npk - 1),
               target_misaligned=dict(target_packed=bufs["target_packed"].t.data_ptr() + 4))
    for k in ("obs", "act", "next_obs", "absorbing", "a_next", "logp_next", "a_pi", "logp_pi", "param", "m", "v", "packed",
              "target_param", "target_packed", "ws", "out"):
        bad["null_" + k] = {k: None}
    L = lib()
    for name, over in bad.items():
        f = block(**over)
        rc = L.oly_iq_q_update(eng.ctx.handle, C.byref(f), eng._s())
        assert rc == _abi.OLY_EINVAL, (name, rc)
    assert L.oly_iq_q_update(eng.ctx.handle, None, eng._s()) == _abi.OLY_EINVAL
    torch.cuda.synchronize()
    assert_untouched(bufs, "refused calls")


# ------------------------------------------------------------------------------ checkpoint / resume
def test_a_saved_run_resumes_to_the_same_bits(eng, golden, tmp_path):
    g = golden("iq_q_update/iq_target.npz")
    whole, gen = build_agent(eng, g, "iq_target")
    run_fixture(whole, g, 0, 4)
    first, _ = build_agent(eng, g, "iq_target")
    run_fixture(first, g, 0, 2)
    path = first.save(str(tmp_path / "iq.pt"), note="after update 2")
    resumed, _ = build_agent(eng, g, "iq_target")
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
