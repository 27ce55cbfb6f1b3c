"""K20 on the GPU: the episode statistics (oly_episode_stats) and the agent's iteration diagnostics (oly_iter_log) against
the reference-run fixtures of tests/golden/iter_log/ and the float64 restatement of tests/iter_log_restate.py, through the
C entry points, the engine and the agents' writer.

Tolerances.  Against the fixtures: rs.tolerances of the float32-fixture-versus-float64 spread that
tests/test_iter_log_cpu.py prints (four times the spread relative to the value itself, DESIGN section 13's floor of 1e-6;
the episode means 1e-12 relative; EpLenMean exact).  Against the restatement at other shapes there is no fixture to
measure a spread on: vf_loss, entropy and kl are held to the project's device tolerance 2e-5 (tests/disc_log_restate.py),
relative to the value itself, on inputs whose KL is of order one so that the float32 rounding of the means (about 1e-6)
stays below it."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import iter_log_restate as rs
from il_shapes import guarded

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
DEV_TOL = 2e-5
_spread = {}


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


def fixture_tolerances(case):
    """(tolerances [6], the float64 restatement's output, the fixture, the arguments), computed once per case."""
    if case not in _spread:
        a, g = rs.load_case(case, device="cuda")
        ref = rs.restate_iter_log(device="cuda", **a)
        _spread[case] = (rs.tolerances(rs.rel_err(ref["scalars"][:6], g["values"])), ref, g, a)
    return _spread[case]


# ------------------------------------------------------------------------------ 1. the episode kernel
#             T    N
EP_SHAPES = ((1, 1), (1, 65), (7, 40), (33, 257), (400, 64))
_ep_ref = {}


def episode_blocks(T, N, seed):
    """Positive rewards (no cancellation in the sums) and flags with the columns that can go wrong: column 0 without a
    single `last`, column 1 all `last`, column 2 with `last` on the first and the final step only."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.1, 1.1, (T, N))
    r2 = rng.uniform(0.05, 2.0, (T, N)).astype(np.float32)
    last = rng.random((T, N)) < 0.15
    last[:, 0] = False
    if N > 1:
        last[:, 1] = True
    if N > 2:
        last[:, 2] = False
        last[0, 2] = last[-1, 2] = True
    return r, r2, last


def check_episode(got, want, two):
    for i in (3, 4, 7):
        assert got[i] == want[i], (i, got, want)                                   # counts and the sum of lengths: exact
    if want[4] == 0:
        assert np.isnan(got[2]) and np.isnan(want[2])
    else:
        assert got[2] == want[2]
    for i in (0, 5) + ((1, 6) if two else ()):
        assert abs(got[i] - want[i]) <= 1e-12 * abs(want[i]), (i, got[i], want[i])
    if not two:
        assert got[1] == 0.0 and got[6] == 0.0


@pytest.mark.parametrize("shape", EP_SHAPES, ids=[f"{t}x{n}" for t, n in EP_SHAPES])
def test_episode_stats_against_the_restatement(eng, shape):
    from olympic_hip.il_agent import episode_stats
    T, N = shape
    r, r2, last = episode_blocks(T, N, seed=3 + T + N)
    for gamma in (1.0, 0.99):
        for r64 in (False, True):
            rew = r if r64 else r.astype(np.float32)
            key = (shape, gamma, r64)
            if key not in _ep_ref:
                _ep_ref[key] = rs.episode_stats(rew, last, gamma, reward2=r2)
            want2 = _ep_ref[key]
            want1 = want2.copy()
            want1[[1, 6]] = 0.0
            for two in (False, True):
                for flag_dtype in (torch.bool, torch.uint8):
                    out = guarded(8, F64, init=np.full(8, 7.0))
                    got = episode_stats(eng, _dev(rew), _dev(last, flag_dtype), gamma=gamma,
                                        reward2=_dev(r2) if two else None)
                    assert got.shape == (8,) and got.dtype == F64 and got.is_cuda
                    eng.episode_stats(_dev(rew), _dev(last, flag_dtype), gamma=gamma, reward2=_dev(r2) if two else None,
                                      out=out.t)
                    torch.cuda.synchronize()
                    assert out.intact()
                    check_episode(got.cpu().numpy(), want2 if two else want1, two)
                    assert np.array_equal(got.cpu().numpy(), out.t.cpu().numpy(), equal_nan=True)    # two runs: identical bits
    # a column counts one return more than lengths exactly when it ends open
    ends_open = int((~last[-1]).sum())
    assert _ep_ref[(shape, 1.0, True)][3] - _ep_ref[(shape, 1.0, True)][4] == ends_open


def test_episode_stats_without_a_completed_episode(eng):
    """No `last` anywhere: every column is one open episode, a return and no length; the length mean is NaN (the
    reference would raise in int(np.round(nan)))."""
    r, r2, _ = episode_blocks(7, 40, seed=9)
    last = np.zeros((7, 40), bool)
    got = eng.episode_stats(_dev(r, F32), _dev(last), reward2=_dev(r2)).cpu().numpy()
    want = rs.episode_stats(r.astype(np.float32), last, reward2=r2)
    check_episode(got, want, True)
    assert got[3] == 40 and got[4] == 0 and got[7] == 0 and np.isnan(got[2])


# ------------------------------------------------------------------------------ 2. oly_iter_log through the engine
def device_iter_log(eng, a, ws=None, bufs=None):
    """restate_iter_log's arguments through Engine.iter_log (one C call) -> (out [8], colstats [3,D]) as numpy."""
    n, D = a["x"].shape
    cs = guarded((3, D), F64, init=a["colstats"])
    out = guarded(8, F64, init=np.full(8, 7.0))
    wsg = guarded(int(eng.iter_log_ws(n).numel()), F32) if ws is None else None
    critic = eng.ilmlp_pack(*[_dev(p, F32) for p in a["critic"]])
    policy = eng.ilmlp_pack(*[_dev(p, F32) for p in a["policy"]])
    r_env = _dev(a["r_env"])
    eng.iter_log(_dev(a["x"], F32), _dev(a["v_target"], F32), _dev(a["mu_old"], F32), _dev(a["ls_old"], F32),
                 _dev(a["log_sigma"], F32), critic, policy, r_env, _dev(a["r"], F32), _dev(a["last"]), cs.t,
                 wsg.t if ws is None else ws, out=out.t)
    torch.cuda.synchronize()
    if bufs is not None:
        bufs.update(cs=cs, out=out, **({} if wsg is None else dict(ws=wsg)))
    return out.t.cpu().numpy().copy(), cs.t.cpu().numpy().copy()


@pytest.mark.parametrize("case", rs.CASES)
def test_fixture_through_the_engine(eng, case):
    tol, ref, g, a = fixture_tolerances(case)
    bufs = {}
    got, cs = device_iter_log(eng, a, bufs=bufs)
    assert not [k for k, b in bufs.items() if not b.intact()]
    want = g["values"]
    err = rs.rel_err(got[:6], want)
    for name, x, w, e, t in zip(rs.NAMES, got, want, err, tol):
        print(f"{case} {name:14s} device {x:+.12e} fixture {w:+.12e} err {e:.2e} tol {t:.1e}")
    assert got[2] == want[2]                                                        # EpLenMean: exact
    assert np.all(err <= tol), {rs.NAMES[i]: (err[i], tol[i]) for i in range(6) if err[i] > tol[i]}
    assert got[6] == float(g["mean_length"]) and got[7] == int(g["episodes"])
    # the live statistics end at S + 2c, where the reference's Standardizer does
    n = a["x"].shape[0]
    assert cs[0, 0] - a["colstats"][0, 0] == 2 * n and np.all(cs[0] == cs[0, 0])
    assert cs[0, 0] + 1e-2 == pytest.approx(float(g["st_count"][0]), rel=1e-12)
    assert np.all(np.abs(cs[1] - g["st_sum"]) <= DEV_TOL * np.maximum(1, np.abs(g["st_sum"])))
    assert np.all(np.abs(cs[2] + 1e-2 - g["st_sumsq"]) <= DEV_TOL * np.maximum(1, np.abs(g["st_sumsq"])))
    assert np.all(np.abs(cs - ref["colstats"]) <= 1e-12 * np.maximum(1, np.abs(ref["colstats"])))
    # ... which is two accumulating oly_col_stats calls in sequence, bit for bit
    two = _dev(a["colstats"], F64)
    for _ in range(2):
        two = eng.col_stats(_dev(a["x"], F32), two)
    torch.cuda.synchronize()
    assert np.array_equal(cs, two.cpu().numpy())
    # two runs are bit-identical
    got2, cs2 = device_iter_log(eng, a)
    assert np.array_equal(got, got2) and np.array_equal(cs, cs2)


#         T    N    D   A
SHAPES = ((1, 1, 17, 1),            # one row, one action
          (255, 1, 45, 11),         # a partial reduction block
          (1, 257, 17, 32),         # a full block and one row; the action limit
          (8, 40, 45, 11),          # the agents' shape
          (16385, 1, 32, 11))       # two chunks, the last of one row


def shape_case(T, N, D, A, seed):
    rng = np.random.default_rng(seed)
    n = T * N
    scale, shift = rng.uniform(0.3, 3.0, D), rng.normal(0, 2, D)
    x = (rng.normal(0, 1, (n, D)) * scale + shift).astype(np.float32)

    def net(out_dim):
        shapes = ((512, D), (512,), (256, 512), (256,), (out_dim, 256), (out_dim,))
        return [(rng.standard_normal(s) * (1.4, 1.4, 0.5)[i // 2] / np.sqrt(s[1])).astype(np.float32) if i % 2 == 0
                else (rng.uniform(-1, 1, s) * 0.1).astype(np.float32) for i, s in enumerate(shapes)]
    st = rs.Stats(1e-2, np.zeros(D), np.full(D, 1e-2))
    st.add((rng.normal(0.5, 1.0, (500, D)) * scale * 1.5 + shift).astype(np.float32))
    policy = net(A)
    old = [(p + 0.02 * rng.standard_normal(p.shape)).astype(np.float32) for p in policy]
    far = (0.5 * rng.choice([-1.0, 1.0], (n, A))).astype(np.float32)      # half a sigma per action: a KL of order one
    ls_old = rng.normal(-0.7, 0.1, A).astype(np.float32)
    r, r2, last = episode_blocks(T, N, seed + 1)
    return dict(critic=net(1), policy=policy, log_sigma=(ls_old + rng.normal(0, 0.05, A)).astype(np.float32),
                mu_old=rs.old_means(old, st.colstats(), x, "cuda") + far, ls_old=ls_old, colstats=st.colstats(), x=x,
                v_target=(rng.normal(0, 1, n) + 0.5 * x[:, 0]).astype(np.float32), r_env=r.astype(np.float32), r=r2,
                last=last)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_shapes_against_the_restatement(eng, shape):
    a = shape_case(*shape, seed=21 + SHAPES.index(shape))
    bufs = {}
    got, cs = device_iter_log(eng, a, bufs=bufs)
    assert not [k for k, b in bufs.items() if not b.intact()]
    ref = rs.restate_iter_log(device="cuda", **a)
    want = ref["scalars"]
    for name, x, w in zip(rs.NAMES + ("mean length", "episodes"), got, want):
        print(f"{'x'.join(str(v) for v in shape):14s} {name:14s} device {x:+.12e} float64 {w:+.12e}")
    for i in rs.EPISODE:
        assert abs(got[i] - want[i]) <= rs.EP_TOL * abs(want[i])
    assert (np.isnan(got[2]) and np.isnan(want[2])) or got[2] == want[2]
    assert (np.isnan(got[6]) and np.isnan(want[6])) or got[6] == want[6]
    assert got[7] == want[7]
    assert want[5] > 0.05                                                           # the KL is of order one by design
    err = rs.rel_err(got[3:6], want[3:6])
    assert np.all(err <= DEV_TOL), dict(zip(rs.NAMES[3:], err))
    assert np.all(np.abs(cs - ref["colstats"]) <= 1e-12 * np.maximum(1, np.abs(ref["colstats"])))
    assert cs[0, 0] - a["colstats"][0, 0] == 2 * a["x"].shape[0]
    got2, cs2 = device_iter_log(eng, a)
    assert np.array_equal(got, got2, equal_nan=True) and np.array_equal(cs, cs2)


def test_a_larger_workspace_is_reused(eng):
    a = shape_case(8, 40, 45, 11, seed=5)
    big = eng.iter_log_ws(20000)
    big.fill_(float("nan"))
    got, cs = device_iter_log(eng, a, ws=big)
    want, cs2 = device_iter_log(eng, a)
    assert np.array_equal(got, want) and np.array_equal(cs, cs2)


# ------------------------------------------------------------------------------ 3. agents
def _agent(eng, case, **kw):
    """A GAILAgent / VAILAgent on test_gpu_disc_log's trainers with a real DeviceTRPO; policy and critic share one
    Standardizer."""
    import test_gpu_disc_log as dl
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceGaussianPolicy, DeviceILCritic, DeviceTRPO, GAILAgent, VAILAgent
    r, tr, _, _, _ = dl._trainer(eng, case, lr=1e-4)
    torch.manual_seed(2)
    lins = [torch.nn.Linear(dl.OBS, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
    pol_lins = [torch.nn.Linear(dl.OBS, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, dl.ACT)]
    stand = DeviceStandardizer(eng, dl.OBS)
    critic = DeviceILCritic(eng, lins, stand)
    policy = DeviceGaussianPolicy(eng, pol_lins, stand, std_0=0.8)
    step = DeviceTRPO(policy, max_kl=1e-2, ent_coeff=1e-3, n_epochs_cg=10)
    cls = GAILAgent if case.startswith("gail") else VAILAgent
    return cls(eng, r, tr, critic, step, train_D_n_th_epoch=3, start_iter=5, **kw), step, r


@pytest.mark.parametrize("case", ["gail_s", "vail_s"])
def test_agent_logs_the_iteration(eng, case):
    import test_gpu_disc_log as dl
    from olympic_hip.il_agent import DISC_LOG_NAMES, ITER_LOG_NAMES
    assert ITER_LOG_NAMES == rs.NAMES
    names = DISC_LOG_NAMES[case[:4]]
    kl_tol = max(fixture_tolerances(c)[0][5] for c in rs.CASES)
    sw_on, sw_off, sw_plain = dl.Recorder(), dl.Recorder(), dl.Recorder()
    on, step_on, _ = _agent(eng, case, sw=sw_on, iteration_log=True)
    off, step_off, r_off = _agent(eng, case, sw=sw_off, iteration_log=False)
    plain, step_plain, r_plain = _agent(eng, case, sw=sw_plain)
    T, N = 8, 40
    for call, it in enumerate((5, 6, 7)):
        ds = dl._dataset(T, N, call)
        before = len(sw_on.rows)
        outs = [ag.fit(ds, generator=torch.Generator(device="cuda").manual_seed(call)) for ag in (on, off, plain)]
        torch.cuda.synchronize()
        o1, o2, o3 = outs
        # the flag off is the agent built without the argument, bit for bit
        assert set(o2) == set(o3) and "iter_log" not in o2
        for k in ("reward", "v_target", "adv", "critic_loss"):
            assert torch.equal(o2[k], o3[k]), k
        assert sw_off.rows == sw_plain.rows
        assert torch.equal(off.standardizer.colstats, plain.standardizer.colstats)
        assert torch.equal(r_off.stand.colstats, r_plain.stand.colstats)
        assert torch.equal(step_off.policy.theta, step_plain.policy.theta)
        if it % 3 != 0:
            assert "iter_log" not in o1 and len(sw_on.rows) == before
            if it == 5:       # nothing has run yet: the twins' statistics agree
                assert torch.equal(on.standardizer.colstats, off.standardizer.colstats)
            continue
        assert o2["disc_loss"] is not None and torch.equal(o2["disc_loss"], o3["disc_loss"])
        rows = sw_on.rows[before:]
        assert [t for t, _, _ in rows] == list(names) + list(rs.NAMES)               # the discriminator's tags, then the six
        assert all(s == it // 3 for _, _, s in rows)
        assert o1["iter_log"] == {t: v for t, v, _ in rows[len(names):]} and list(o1["iter_log"]) == list(rs.NAMES)
        assert o1["disc_log"] == {t: v for t, v, _ in rows[:len(names)]}
        log = o1["iter_log"]
        assert all(np.isfinite(v) for v in log.values())
        # until the call the twins ran the same arithmetic: the diagnostics moved the shared Standardizer two batches on
        cs_on, cs_off = on.standardizer.colstats, off.standardizer.colstats
        assert float(cs_on[0, 0]) - float(cs_off[0, 0]) == 2 * T * N
        assert torch.equal(step_on.policy.theta, step_off.policy.theta)
        # every column ends its only episode at the last step
        assert log["EpLenMean"] == T
        r_env = ds["reward"].cpu().numpy()
        want = rs.episode_stats(r_env, ds["last"].cpu().numpy(), reward2=o1["reward"].cpu().numpy())
        # a randn reward sums to about zero: the rounding scales with the magnitudes added, not with their sum
        assert abs(log["EpTrueRewMean"] - want[0]) <= 1e-12 * rs.episode_stats(np.abs(r_env), ds["last"].cpu().numpy())[0]
        assert abs(log["EpRewMean"] - want[1]) <= 1e-12 * abs(want[1])
        # kl recomputed in float64 from the old distribution and the stepped policy's means at the final statistics
        mu_old, ls_old = step_on.old_distribution()
        assert mu_old.shape == (T * N, dl.ACT) and ls_old.shape == (dl.ACT,)
        assert mu_old.data_ptr() >= step_on._ws[1].data_ptr()                           # views, not copies
        flat = ds["state"].reshape(T * N, dl.OBS)
        mu = step_on.policy.predict(flat)
        kl = float(np.mean(rs.kl_rows(mu_old.cpu().numpy(), ls_old.cpu().numpy(), mu.cpu().numpy(),
                                      step_on.policy.log_sigma.cpu().numpy())))
        print(f"{case}: kl device {log['kl']:.9e} recomputed {kl:.9e}; TRPO's own {step_on.scalars()['kl']:.3e}")
        assert abs(log["kl"] - kl) <= kl_tol * abs(kl)
        assert abs(log["entropy"] - float(step_on.policy.entropy())) <= 1e-6 * abs(log["entropy"])
        s1 = cs_on - eng.col_stats(flat.contiguous())                                   # S + c, what self._V(x) saw
        v = eng.ilmlp_forward(flat.contiguous(), on.critic.packed, 1, colstats=s1.contiguous()).reshape(-1).double()
        vf = float(((v - o1["v_target"].reshape(-1).double()) ** 2).mean())
        assert abs(log["vf_loss"] - vf) <= DEV_TOL * vf
    assert len(sw_on.rows) == len(names) + 6 and len(sw_off.rows) == len(names)


# ------------------------------------------------------------------------------ 4. refusals
def test_refusals(eng):
    import test_gpu_disc_log as dl
    from olympic_hip import _abi
    from olympic_hip._ffi import OlyError, lib
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceGaussianPolicy, DeviceILCritic, DeviceTRPO, GAILAgent
    # the agents' constructor
    r, tr, _, _, _ = dl._trainer(eng, "gail_s")
    lins = lambda out: [torch.nn.Linear(dl.OBS, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, out)]   # noqa: E731
    stand = DeviceStandardizer(eng, dl.OBS)
    critic = DeviceILCritic(eng, lins(1), stand)
    step = DeviceTRPO(DeviceGaussianPolicy(eng, lins(dl.ACT), stand), max_kl=1e-2, ent_coeff=0.0, n_epochs_cg=5)
    with pytest.raises(OlyError, match="sw"):
        GAILAgent(eng, r, tr, critic, step, iteration_log=True)
    with pytest.raises(OlyError, match="old_distribution"):
        GAILAgent(eng, r, tr, critic, lambda *k: None, sw=dl.Recorder(), iteration_log=True)
    other = DeviceTRPO(DeviceGaussianPolicy(eng, lins(dl.ACT), DeviceStandardizer(eng, dl.OBS)), max_kl=1e-2, ent_coeff=0.0,
                       n_epochs_cg=5)
    with pytest.raises(OlyError, match="share one Standardizer"):
        GAILAgent(eng, r, tr, critic, other, sw=dl.Recorder(), iteration_log=True)
    GAILAgent(eng, r, tr, critic, step, sw=dl.Recorder(), iteration_log=True)
    GAILAgent(eng, r, tr, critic, other, sw=dl.Recorder())                              # without the flag nothing is asked
    with pytest.raises(OlyError, match="no step"):
        step.old_distribution()

    # the engine's checks
    a = shape_case(8, 40, 17, 11, seed=2)
    n = 320
    t = dict(x=_dev(a["x"], F32), vt=_dev(a["v_target"], F32), mo=_dev(a["mu_old"], F32), lo=_dev(a["ls_old"], F32),
             ls=_dev(a["log_sigma"], F32), pc=eng.ilmlp_pack(*[_dev(p, F32) for p in a["critic"]]),
             pp=eng.ilmlp_pack(*[_dev(p, F32) for p in a["policy"]]), re=_dev(a["r_env"], F32), r=_dev(a["r"], F32),
             last=_dev(a["last"]), cs=_dev(a["colstats"], F64), ws=eng.iter_log_ws(n))

    def engine_call(**kw):
        u = dict(t, **kw)
        return eng.iter_log(u["x"], u["vt"], u["mo"], u["lo"], u["ls"], u["pc"], u["pp"], u["re"], u["r"], u["last"], u["cs"],
                            u["ws"])
    for bad in (dict(ws=t["ws"][:-1]), dict(re=t["re"][:7].contiguous()), dict(last=t["last"].to(F32)),
                dict(vt=t["vt"][:-1].contiguous()), dict(cs=t["cs"].to(F32)), dict(r=None)):
        with pytest.raises(OlyError):
            engine_call(**bad)
    with pytest.raises(OlyError):
        eng.iter_log_ws(0)
    with pytest.raises(OlyError):
        eng.episode_stats(t["re"], t["last"][:7].contiguous())
    with pytest.raises(OlyError):
        eng.episode_stats(t["re"], t["last"], gamma=1.5)

    # the C entry points themselves, before any launch: the outputs keep their sentinels
    out = guarded(8, F64, init=np.full(8, 7.0))
    keep = t["cs"].clone()

    def call(**kw):
        f = dict(n=n, in_dim=17, act_dim=11, T=8, N=40, rew_f64=0, x=t["x"].data_ptr(), v_target=t["vt"].data_ptr(),
                 mu_old=t["mo"].data_ptr(), log_sigma_old=t["lo"].data_ptr(), log_sigma=t["ls"].data_ptr(),
                 critic_packed=t["pc"].data_ptr(), policy_packed=t["pp"].data_ptr(), rew_env=t["re"].data_ptr(),
                 rew=t["r"].data_ptr(), last=t["last"].data_ptr(), colstats=t["cs"].data_ptr(), ws=t["ws"].data_ptr(),
                 ws_floats=int(t["ws"].numel()), out=out.t.data_ptr())
        f.update(kw)
        return lib().oly_iter_log(eng.ctx.handle, C.byref(_abi.IterLog(**f)), eng._s())
    for bad in (dict(x=None), dict(mu_old=None), dict(rew=None), dict(last=None), dict(colstats=None), dict(out=None),
                dict(ws=None), dict(n=0, T=0), dict(n=-3), dict(T=7), dict(N=41), dict(n=321),
                dict(ws_floats=int(t["ws"].numel()) - 1), dict(in_dim=65), dict(in_dim=0), dict(act_dim=33)):
        assert call(**bad) == _abi.OLY_EINVAL, bad
    assert lib().oly_iter_log(eng.ctx.handle, None, eng._s()) == _abi.OLY_EINVAL
    ep = guarded(8, F64, init=np.full(8, 7.0))
    for T_, N_, rew, last, gamma, o in ((0, 40, t["re"], t["last"], 1.0, ep.t), (8, 0, t["re"], t["last"], 1.0, ep.t),
                                        (8, 40, None, t["last"], 1.0, ep.t), (8, 40, t["re"], None, 1.0, ep.t),
                                        (8, 40, t["re"], t["last"], 1.0, None), (8, 40, t["re"], t["last"], -0.1, ep.t),
                                        (65536, 65536, t["re"], t["last"], 1.0, ep.t)):
        rc = lib().oly_episode_stats(eng.ctx.handle, T_, N_, 0, gamma, None if rew is None else rew.data_ptr(), None,
                                     None if last is None else last.data_ptr(), None if o is None else o.data_ptr(), eng._s())
        assert rc == _abi.OLY_EINVAL, (T_, N_, gamma)
    torch.cuda.synchronize()
    assert out.intact() and bool((out.t == 7.0).all()) and ep.intact() and bool((ep.t == 7.0).all())
    assert torch.equal(t["cs"], keep)
    assert call() == _abi.OLY_OK
    torch.cuda.synchronize()
    assert not torch.equal(t["cs"], keep) and out.intact() and bool((out.t != 7.0).any())
