"""K26's v0 pass and all-expert batches on the MI355X: oly_iq_q_update with the block oly_iq_v0 against the float64 twin of
tests/iq_v0_restate.py over its shapes, the fourth pass's bits (oly_ilmlp_forward's on its rows, equal across runs), the
Standardizers' accounting, the NaN slots of an empty policy subset, the refusals before any launch, the reference-run
fixtures of tests/golden/gen_iq_v0.py through Engine and DeviceLSIQOffline, and fit_offline's split and checkpointed runs.

Tolerances are test_gpu_iq_q.py's: 4 x the float32-against-float64 spread of the same update, never below TOL = 2e-5.
For a fixture the spread is the stored one; for a case of the sweep it is measured by running the twin in float32 too.
Every operand is fenced (tests/fences.py) and the workspace has exactly the reported size."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import torch

import iq_restate as R
import iq_v0_restate as V
from fences import Fenced, assert_untouched, fenced
from test_gpu_iq_q import Dev, Recorder, split

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, SHAPES, cat = V.TOL, V.SHAPES, V.cat
POLICY_SLOTS = (6, 7, 10, 12, 14)      # Q, Q^2, Reward and Targets for the policy, Q Absorbing state plcy


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def block_of(c):
    return dict(lossQ_type=c.type, loss_mode_exp=c.exp_mode, Q_exp_loss=c.exp_loss, target_clipping=c.clip, Q_min=c.q_min,
                Q_max=c.q_max)


class VDev(Dev):
    """test_gpu_iq_q.py's fenced critic state with the v0 call: a_v0 / logp_v0 fenced at exactly n_v0 rows."""

    def __init__(self, eng, params, algo, cfg, in_dim, A, B):
        super().__init__(eng, params, cfg, in_dim, A, B)
        self.algo = algo

    def update(self, s, n_policy, **over):
        c = self.cfg
        self.inputs = {k: fenced(np.asarray(v, np.float32)) for k, v in s.items()}
        i = {k: v.t for k, v in self.inputs.items()}
        kw = dict(algo=self.algo, plcy_loss_mode=c.mode, regularizer_mode=c.reg, treat_absorbing=c.treat,
                  use_target=c.use_target, update_target=c.update_target, gamma=c.gamma, alpha=c.alpha, reg_mult=c.reg_mult,
                  tau=c.tau, weight_decay=c.wd, eps=c.adam_eps, lsiq=block_of(c) if self.algo == "lsiq" else None,
                  v0=(i["a_v0"], i["logp_v0"]) if "a_v0" in i else None, all_expert=n_policy == 0)
        kw.update(over)
        self.eng.iq_q_update(i["obs"], i["act"], i["next_obs"], i["absorbing"], i["a_next"], i["logp_next"], i["a_pi"],
                             i["logp_pi"], n_policy, self.t("colstats"), self.t("target_colstats"), self.t("param"),
                             self.t("m"), self.t("v"), self.t("packed"), self.t("target_param"), self.t("target_packed"),
                             self.t("ws"), self.step, c.lr, out=self.t("out"), **kw)
        self.step += 1
        return self.t("out").clone()


def against_the_twin(eng, k, algo, cfg):
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = V.sweep_inputs(k)
    ref, ref_out, f32, f32_out, _ = V.yardstick(k, algo, cfg)
    dev = VDev(eng, params, algo, cfg, in_dim, A, B)
    out = np.stack([dev.update(s, n_policy).cpu().numpy() for s in V.case_steps(cfg, steps)])
    got = dev.snapshot()
    who = f"{SHAPES[k]} {V.cfg_id(algo, cfg)}"
    dev.check_fences(who)
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
        # the live count: Q, Q' without a target, Q_pi, and the v0 pass's n_v0 rows; the target's: Q' alone
        passes = 2 if cfg.use_target else 3
        n_v0 = B - n_policy if cfg.mode == "v0" else 0
        assert float(got["colstats"][0, 0]) == V.UPDATES * (passes * B + n_v0), who
        assert float(got["target_colstats"][0, 0]) == (V.UPDATES * B if cfg.use_target else 0), who
    spread = np.abs(f32_out - ref_out)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(ref_out)), 4 * np.where(np.isnan(spread), 0.0, spread))
    assert np.array_equal(np.isnan(out), np.isnan(ref_out)), (who, out, ref_out)
    if n_policy == 0:        # NaN exactly where the subset is empty (slot 13 too where no expert row is absorbing)
        assert np.isnan(out[:, POLICY_SLOTS]).all(), (who, out)
        assert not np.isnan(np.delete(out, POLICY_SLOTS + (13,), axis=1)).any(), (who, out)
    else:
        assert not np.isnan(np.delete(out, (13, 14), axis=1)).any(), (who, out)
    bad = ~(np.abs(out - ref_out) <= tol) & ~np.isnan(ref_out)
    print(f"{who} scalars: worst |kernel - f64| / tolerance {np.nanmax(np.abs(out - ref_out) / tol):.3f}")
    assert not bad.any(), (who, np.argwhere(bad), out[bad], ref_out[bad])
    assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim + A)))
    assert torch.equal(got["target_packed"], eng.ilmlp_pack(*split(got["target_param"], in_dim + A)))


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["-".join(map(str, s)) for s in SHAPES])
def test_update_against_float64(eng, k):
    """Shape k with the four configs tests/iq_v0_restate.py gives it: over the seven shapes IQ and LSIQ fix/MSE, fix/Huber
    and bootstrap, the regularizers off, exp and exp_and_plcy, with and without a target and Standardizers, twice each."""
    assert len(V.sweep(k)) == 4
    for _, algo, cfg in V.sweep(k):
        against_the_twin(eng, k, algo, cfg)


@pytest.mark.parametrize("k", [k for k, s in enumerate(SHAPES) if s[3] == 0 and s[2] <= 33])
def test_all_expert_batches_without_v0(eng, k):
    """all_expert in the modes that draw nothing more (value, value_expert, off): the existing instantiations with
    n_policy = 0."""
    for algo, cfg in V.PLAIN_ALL_EXPERT:
        against_the_twin(eng, k, algo, cfg)


# ------------------------------------------------------------------------------ bits
def exact_inputs(k, seed):
    """One update's inputs on a grid of 1/8, so that the Standardizer's float64 sums are exact in any order."""
    steps, params = V.sweep_inputs(k, seed=seed)
    s = dict(steps[0])
    for key in ("obs", "act", "next_obs", "a_next", "a_pi", "a_v0"):
        s[key] = (np.round(s[key] * 8) / 8).astype(np.float32)
    return s, params


@pytest.mark.parametrize("k", (0, 2, 4), ids=lambda k: "-".join(map(str, SHAPES[k])))
@pytest.mark.parametrize("standardizer", (False, True), ids=("nostd", "std"))
def test_q_v0_has_the_forward_kernels_bits(eng, k, standardizer):
    """The fourth row of the workspace's values at the expert rows against oly_ilmlp_forward on (obs[expert] | a_v0) with
    the statistics the Standardizer holds at that pass; rows 0 and 2 keep theirs."""
    from olympic_hip._ffi import lib
    in_dim, A, B, n_policy = SHAPES[k]
    s, params = exact_inputs(k, seed=77 + k)
    for use_target in (True, False):
        cfg = V.iq_cfg(mode="v0", use_target=use_target, standardizer=standardizer)
        dev = VDev(eng, params, "iq", cfg, in_dim, A, B)
        packed0 = dev.t("packed").clone()
        dev.update(s, n_policy)
        torch.cuda.synchronize()
        off, BP = int(lib().oly_iq_q_ws_values(B, in_dim, A)), (B + 15) // 16 * 16
        assert off + 4 * BP <= dev.nws
        qv = dev.t("ws")[off:off + 4 * BP].view(4, BP)[:, :B]
        x0 = np.concatenate([s["obs"], s["act"]], 1)
        x1 = np.concatenate([s["next_obs"], s["a_next"]], 1)
        x2 = np.concatenate([s["obs"], s["a_pi"]], 1)
        x3 = np.concatenate([s["obs"][n_policy:], s["a_v0"]], 1)
        st = lambda xs: torch.as_tensor(sum(np.stack([np.full(x.shape[1], float(len(x))), x.astype(np.float64).sum(0),
                                                      np.square(x.astype(np.float64)).sum(0)]) for x in xs)).cuda()
        live = [x0, x2] if use_target else [x0, x1, x2]
        c0 = st([x0]) if standardizer else None
        c2 = st(live) if standardizer else None
        c3 = st(live + [x3]) if standardizer else None
        fwd = lambda x, c: eng.ilmlp_forward(torch.as_tensor(x).cuda(), packed0, 1, colstats=c).reshape(-1)
        assert torch.equal(qv[0], fwd(x0, c0)), use_target
        assert torch.equal(qv[2], fwd(x2, c2)), use_target
        assert torch.equal(qv[3][n_policy:], fwd(x3, c3)), use_target
        if standardizer:
            assert torch.equal(dev.t("colstats"), c3)


def test_two_runs_give_the_same_bits(eng):
    for k, (algo, cfg) in ((6, V.CONFIGS[13]), (5, V.CONFIGS[12]), (0, V.CONFIGS[0])):
        in_dim, A, B, n_policy = SHAPES[k]
        steps, params = V.sweep_inputs(k)
        snaps = []
        for _ in range(2):
            dev = VDev(eng, params, algo, cfg, in_dim, A, B)
            outs = [dev.update(s, n_policy) for s in steps]
            torch.cuda.synchronize()
            snaps.append((dev.snapshot(), torch.stack(outs), dev.t("ws").clone()))
        for key, a in snaps[0][0].items():
            assert a is None or torch.equal(a.view(torch.uint8), snaps[1][0][key].view(torch.uint8)), key
        assert torch.equal(snaps[0][1].view(torch.int64), snaps[1][1].view(torch.int64))


def test_a_call_without_the_block_ignores_v0_inputs(eng):
    """Mode value with n_policy = 9: the same bits with and without an (unused) all_expert=False, v0=None call path, and a
    v0 call moves the parameters elsewhere (the fourth pass carries a gradient)."""
    k = 0
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = V.sweep_inputs(k)
    cfg = V.iq_cfg(mode="value", tau=0.05)
    plain = Dev(eng, params, R.Cfg(algo="iq", mode="value", tau=0.05), in_dim, A, B)
    plain_out = plain.update({k_: v for k_, v in steps[0].items() if k_ not in ("a_v0", "logp_v0")}, n_policy)
    via = VDev(eng, params, "iq", cfg, in_dim, A, B)
    via_out = via.update(V.case_steps(cfg, steps)[0], n_policy)
    a, b = plain.snapshot(), via.snapshot()
    for key in a:
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(plain_out.view(torch.int64), via_out.view(torch.int64))
    v0 = VDev(eng, params, "iq", cfg._replace(mode="v0"), in_dim, A, B)
    v0.update(steps[0], n_policy)
    assert not torch.equal(v0.snapshot()["param"], a["param"])


# ------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(eng):
    from olympic_hip import _abi
    from olympic_hip._ffi import lib
    in_dim, A, B, n_policy = 12, 5, 18, 9
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
    v0bufs = dict(a_v0=Fenced((B, A), f32), logp_v0=Fenced(B, f32))
    V0 = _abi.IQ_PLCY_LOSS_MODES["v0"]
    keep = []

    def ext(block=True, all_expert=0, a_v0=True, logp_v0=True, pad=_abi.OLY_IQ_Q_EXT, lsiq=None, **over):
        kw = dict(in_dim=in_dim, act_dim=A, batch=B, n_policy=n_policy, algo=0, plcy_loss_mode=V0, regularizer_mode=0,
                  treat_absorbing=0, use_target=1, update_target=1, step=0, pad=pad, gamma=0.99, alpha=1e-3, reg_mult=0.5,
                  R_min=0.0, R_max=1.0, gradient_penalty_lambda=0.0, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.0, pad2=0.0, tau=0.005, packed_floats=npk, target_packed_floats=npk, ws_floats=nws)
        kw.update({k: b.t.data_ptr() for k, b in bufs.items()})
        kw.update(over)
        if lsiq is not None:
            lb = _abi.LSIQ(lossQ_type=_abi.LSIQ_LOSSQ_TYPES[lsiq], loss_mode_exp=0, Q_exp_loss=1, target_clipping=1, Q_min=-1.0,
                           Q_max=1.0, h_loss=1, h_tau_up=0.01, h_tau_down=0.01)
            keep.append(lb)
            kw["lsiq"] = C.pointer(lb)
        vb = _abi.IQV0(a_v0=v0bufs["a_v0"].t.data_ptr() if a_v0 else None,
                       logp_v0=v0bufs["logp_v0"].t.data_ptr() if logp_v0 else None, all_expert=all_expert, pad=0)
        e = _abi.IQQExt(q=_abi.IQQ(**kw), v0=C.pointer(vb) if block else None)
        keep.extend((vb, e))
        return e
    lsiq_modes = _abi.LSIQ_PLCY_LOSS_MODES
    bad = dict(sqil=ext(algo=1, plcy_loss_mode=0), sqil_like=ext(algo=2, lsiq="sqil_like", plcy_loss_mode=0),
               lsiq_h=ext(algo=3, lsiq="iq_like", plcy_loss_mode=0, regularizer_mode=0),
               n_policy_0=ext(n_policy=0), n_policy_0_plain=ext(n_policy=0, plcy_loss_mode=0, block=False),
               n_policy_0_pad_0=ext(n_policy=0, all_expert=1, pad=0),
               v0_without_the_block=ext(block=False), v0_pad_0=ext(pad=0), v0_lsiq_without=ext(algo=2, lsiq="iq_like", block=False),
               null_a_v0=ext(a_v0=False), null_logp_v0=ext(logp_v0=False),
               all_expert_value_policy=ext(n_policy=0, all_expert=1, plcy_loss_mode=2),
               all_expert_q_old_policy=ext(n_policy=0, all_expert=1, plcy_loss_mode=3),
               all_expert_both=ext(n_policy=0, all_expert=1, algo=2, lsiq="iq_like",
                                   plcy_loss_mode=lsiq_modes["value_q_old_policy"]),
               all_expert_with_rows_q_old=ext(all_expert=1, plcy_loss_mode=3),
               all_expert_reg_plcy=ext(n_policy=0, all_expert=1, regularizer_mode=_abi.IQ_REGULARIZER_MODES["plcy"]),
               n_policy_B=ext(n_policy=B, all_expert=1), gp=ext(gradient_penalty_lambda=0.5), mode_5_iq=ext(plcy_loss_mode=5),
               ws_short=ext(ws_floats=nws - 1), ws_short_all_expert=ext(n_policy=0, all_expert=1, ws_floats=nws - 1))
    L = lib()
    for name, e in bad.items():
        rc = L.oly_iq_q_update(eng.ctx.handle, C.cast(C.pointer(e), C.POINTER(_abi.IQQ)), eng._s())
        assert rc == _abi.OLY_EINVAL, (name, rc)
    torch.cuda.synchronize()
    assert_untouched(bufs, "refused calls")
    assert_untouched(v0bufs, "refused calls")


def test_the_engine_refuses_what_the_kernel_refuses(eng):
    from olympic_hip._ffi import OlyError
    k = 0
    in_dim, A, B, n_policy = SHAPES[k]
    steps, params = V.sweep_inputs(k)
    s = steps[0]
    cases = [(dict(), dict(v0=None), n_policy),                                     # v0 without the new arguments
             (dict(), dict(all_expert=False), 0),                                   # no policy rows without all_expert
             (dict(mode="value_policy"), dict(v0=None, all_expert=True), 0),
             (dict(mode="value", reg="plcy"), dict(v0=None, all_expert=True), 0),
             (dict(), dict(algo="sqil", plcy_loss_mode="plcy", lsiq=None), n_policy),
             (dict(), dict(gradient_penalty_lambda=0.5), n_policy)]
    for cfg_over, over, n_p in cases:
        cfg = V.iq_cfg(mode="v0")._replace(**cfg_over)
        dev = VDev(eng, params, "iq", cfg, in_dim, A, B)
        before = dev.snapshot()
        st = dict(s)
        if n_p == 0 and "v0" not in over:
            st["a_v0"], st["logp_v0"] = np.zeros((B, A), np.float32), np.zeros(B, np.float32)
        with pytest.raises(OlyError):
            dev.update(st, n_p, **over)
        after = dev.snapshot()
        for key, a in before.items():
            assert torch.equal(a.contiguous().view(torch.uint8), after[key].contiguous().view(torch.uint8)), key
        assert dev.f["out"].unwritten() == 16


# ------------------------------------------------------------------------------ the reference-run fixtures
def gen_module():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_iq_v0 as gen
    return gen


def compare_networks(got_by_prefix, g, gen, tols):
    for prefix, flat in got_by_prefix.items():
        D = gen.IN_DIM if prefix == "policy" else gen.D
        shapes = [(512, D), (512,), (256, 512), (256,), (2 * gen.ACT_DIM if prefix == "policy" else 1, 256),
                  (2 * gen.ACT_DIM if prefix == "policy" else 1,)]
        a, o = flat.double().cpu().numpy(), 0
        for n, s in zip(R.NAMES, shapes):
            k = int(np.prod(s))
            v = a[o:o + k].reshape(s)
            o += k
            r = g[f"{prefix}_w2_head"] if n == "w2" else g[f"{prefix}_{n}"]
            err = float(np.abs((v[:gen.W2_HEAD] if n == "w2" else v) - r).max())
            print(f"{prefix} {n}: {err:.3e} (tolerance {tols[prefix]:.3e})")
            assert err <= tols[prefix], (prefix, n, err)


def compare_stats(pairs, g, key="spread_stats"):
    for got, want in pairs:
        a = got.cpu().numpy()
        assert np.array_equal(a[0], want[0]), (a[0], want[0])
        assert np.all(np.abs(a - want) <= np.maximum(TOL * np.maximum(1.0, np.abs(want)), 4 * float(g[key])))


@pytest.mark.parametrize("name", ("iq_v0", "lsiq_v0"))
def test_fixture_through_the_engine(eng, golden, name):
    """The reference's own IQ_SAC / LSIQ updates with plcy_loss_mode v0, n_policy = 9: Engine.iq_q_update on the recorded
    policy passes against the reference's float32 networks, statistics and logged scalars."""
    gen = gen_module()
    g = golden(f"iq_v0/{name}.npz")
    spec = gen.FIXTURES[name]
    cfg = gen.twin_cfg(spec, float(g["alpha"]), lr=float(g["lr"]), tau=float(g["tau"]), gamma=float(g["gamma"]))
    init = [gen.w2_init(12) if n == "w2" else g[f"critic_init_{n}"] for n in R.NAMES]
    dev = VDev(eng, init, spec["algo"], cfg, gen.IN_DIM, gen.ACT_DIM, gen.B)
    keys = ("obs", "act", "next_obs", "absorbing", "a_next", "logp_next", "a_pi", "logp_pi", "a_v0", "logp_v0")
    out = np.stack([dev.update({k: g[k][i] for k in keys}, int(g["n_policy"])).cpu().numpy() for i in range(gen.N_ITER)])
    got = dev.snapshot()
    dev.check_fences(name)
    compare_networks(dict(critic=got["param"], target=got["target_param"]), g, gen,
                     dict(critic=max(TOL, 4 * float(g["spread_params"])), target=max(TOL, 4 * float(g["spread_target"]))))
    scal = g["scalars"]
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * float(g["spread_scalars"]))
    assert not np.isnan(scal).any() and np.all(np.abs(out - scal) <= tol), np.abs(out - scal) / tol
    compare_stats(((got["colstats"], g["colstats"]), (got["target_colstats"], g["target_colstats"])), g)


def build_offline(eng, g, gen, sw=None, logging_iter=1, **more):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceSoftQCritic
    from olympic_hip.iq_offline import DeviceLSIQOffline

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
    # the demonstrations: the fixture's own batches in order, 4 x 18 rows
    demo = dict(states=g["obs"].reshape(-1, in_dim), actions=g["act"].reshape(-1, A),
                next_states=g["next_obs"].reshape(-1, in_dim), absorbing=g["absorbing"].reshape(-1))
    kw = dict(gamma=float(g["gamma"]), batch_size=gen.B, use_target=bool(g["use_target"]), Q_max=float(g["Q_max"]),
              Q_min=float(g["Q_min"]), loss_mode_exp=gen.OFFLINE["exp_mode"], Q_exp_loss=gen.OFFLINE["exp_loss"],
              regularizer_mode=gen.OFFLINE["reg"], reg_mult=float(g["reg_mult"]), init_alpha=gen.INIT_ALPHA,
              actor_optimizer=dict(lr=float(g["lr_actor"])), logging_iter=logging_iter, sw=sw,
              Q_Q_multiplier=float(g["Q_Q_multiplier"]), abs_mult=float(g["abs_mult"]))
    kw.update(more)
    return DeviceLSIQOffline(eng, policy, critic, demo, **kw)


def run_offline_fixture(agent, g, first, last):
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    outs = []
    for i in range(first, last):
        eps = dict(q=dict(next=d(g["eps_next"][i]), expert=d(g["eps_expert"][i]), pi=d(g["eps_pi"][i]), v0=d(g["eps_v0"][i])),
                   pi=dict(pi=d(g["eps_ppi"][i]), log=d(g["eps_plog"][i])))
        outs.append(agent.iq_update(d(g["obs"][i]), d(g["act"][i]), d(g["next_obs"][i]), d(g["absorbing"][i]), eps=eps))
        agent._iter += 1
        agent.policy.iter = getattr(agent.policy, "iter", 0) + 1
    return outs


def test_offline_fixture_through_the_agent(eng, golden):
    """LSIQ_Offline whole, four logging iterations of fit_offline's loop body in the reference: DeviceLSIQOffline on the
    recorded noise against the reference's policy, critic and target, all three Standardizers and every logged scalar."""
    from olympic_hip import _abi
    gen = gen_module()
    g = golden("iq_v0/lsiq_offline.npz")
    sw = Recorder()
    agent = build_offline(eng, g, gen, sw=sw)
    outs = run_offline_fixture(agent, g, 0, gen.N_ITER)
    torch.cuda.synchronize()
    c = agent.critic
    compare_networks(dict(policy=agent.policy.param, critic=c.param, target=c.target_param), g, gen,
                     dict(policy=max(TOL, 4 * float(g["spread_policy"])), critic=max(TOL, 4 * float(g["spread_params"])),
                          target=max(TOL, 4 * float(g["spread_target"]))))
    scal = g["scalars"]
    out = np.stack([o[0].cpu().numpy() for o in outs])
    logged = ~np.isnan(scal)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(scal)), 4 * float(g["spread_scalars"]))
    assert np.all(np.abs(out - scal)[logged] <= tol[logged]), np.abs(out - scal) / tol
    assert np.isnan(out[:, POLICY_SLOTS]).all()
    ascal = g["actor_scalars"]
    atol = np.maximum(TOL * np.maximum(1.0, np.abs(ascal)), 4 * float(g["spread_actor_scalars"]))
    for i in range(gen.N_ITER):
        row = sw.rows[i + 1]
        for k, t in enumerate(_abi.IQ_Q_TAGS):
            if k == 14:                              # Q Absorbing state plcy: logged, NaN
                assert np.isnan(row[t])
            elif logged[i, k]:
                assert row[t] == out[i, k], (i, t)
            else:
                assert t not in row, (i, t)
        assert "IQ-Loss/Alpha" in row
        for k, t in enumerate(gen.ACTOR_TAGS):
            if np.isnan(ascal[i, k]):
                assert np.isnan(row[t]), (i, t)
            else:
                assert abs(row[t] - ascal[i, k]) <= atol[i, k], (i, t, row[t], ascal[i, k])
        for k, t in enumerate(gen.OFFLINE_ACTION_TAGS):
            want = g["action_scalars"][i, k]
            assert abs(row[t] - want) <= TOL * max(1.0, abs(want)), (i, t)
    compare_stats(((c.stand.colstats, g["colstats"]), (c.target_stand.colstats, g["target_colstats"])), g)
    compare_stats(((agent.policy.stand.colstats, g["policy_colstats"]),), g, "spread_policy_stats")
    # seven passes with rows and one without, per logging iteration
    assert float(agent.policy.stand.colstats[0, 0]) == gen.N_ITER * 7 * gen.B
    assert agent._iter == gen.N_ITER + 1 and c.step == gen.N_ITER and agent.pi_step == gen.N_ITER


def agent_state(agent):
    c = agent.critic
    return dict(param=c.param, target=c.target_param, m=c.exp_avg, v=c.exp_avg_sq, packed=c.packed, tpacked=c.target_packed,
                cs=c.stand.colstats, tcs=c.target_stand.colstats, pparam=agent.policy.param, ppacked=agent.policy.packed,
                pm=agent.pi_exp_avg, pv=agent.pi_exp_avg_sq, pcs=agent.policy.stand.colstats, alpha=agent.alpha_state)


def test_fit_offline_splits_and_resumes_to_the_same_bits(eng, golden, tmp_path):
    """fit_offline(4) equals four fit_offline(1) calls bit for bit, and a run checkpointed after step 2 of 4 and resumed in
    fresh objects ends torch.equal to the uninterrupted one (delay_pi = 2, a learnable temperature, logging every 2nd)."""
    gen = gen_module()
    g = golden("iq_v0/lsiq_offline.npz")
    more = dict(batch_size=7, delay_pi=2, learnable_alpha=True, logging_iter=2)
    seed = lambda: torch.Generator(device="cuda").manual_seed(3)
    whole = build_offline(eng, g, gen, **more)
    whole.fit_offline(4, generator=seed())
    split_ = build_offline(eng, g, gen, **more)
    gs = seed()
    for _ in range(4):
        split_.fit_offline(1, generator=gs)
    first = build_offline(eng, g, gen, **more)
    gf = seed()
    first.fit_offline(2, generator=gf)
    path = first.save(str(tmp_path / "offline.pt"), rng=gf.get_state())
    resumed = build_offline(eng, g, gen, **more)
    meta = resumed.load(path)
    gr = torch.Generator(device="cuda")
    gr.set_state(meta["rng"])
    assert resumed._iter == 3 and resumed.critic.step == 2 and resumed.pi_step == 1
    resumed.fit_offline(2, generator=gr)
    torch.cuda.synchronize()
    want = agent_state(whole)
    assert whole._iter == 5 and whole.critic.step == 4 and whole.pi_step == 2 and whole.alpha_step == 2
    assert float(want["cs"][0, 0]) > 0 and not torch.equal(want["param"], build_offline(eng, g, gen, **more).critic.param)
    for other in (split_, resumed):
        got = agent_state(other)
        for key, a in want.items():
            assert torch.equal(a, got[key]), key
        assert (other._iter, other.critic.step, other.pi_step, other.alpha_step) == (5, 4, 2, 2)
