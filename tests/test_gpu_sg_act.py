"""K25 on the MI355X: oly_sg_act (the squashed-Gaussian act and log-probability in one call) against K16's forward, K5's
controls and float64; the logged fit oly_bc_fit_steps_log against the reference-run fixture
tests/golden/bc_log/bc_log.npz and the float64 restatement of tests/bc_log_restate.py, its bits across runs and across
the way a fit is cut into calls; DeviceSquashedGaussianPolicy(fused_act=True) and
DeviceBehavioralCloning(empirical_entropy=True), resume included.

Tolerances.  mu and log_sigma are K16's kernel structure: bit-equal to Engine.ilmlp_forward, split and clamped.  ctrl is
il_ctrl's expression on the action: bit-equal.  action and log_prob against float64: TOL = 2e-5 (log_prob relative to
max(|log_prob|, 1)).  This file's cases stay where the reference's all-float32 formula is well conditioned too
(|a_raw| < 4, |log_sigma| < 1, asserted), so that they can stand beside a float32 run; the kernel forms tanh, 1 - a^2
+ 1e-6 and its logarithm in fp64 and is held against float64 at saturated tanh, sigma up to exp(2) and the clamp
[-20, 2] by tests/test_gpu_sg_saturation.py on the tables of tests/sg_saturation.py.  The sampled entropy:
max(TOL max(1, |value|), 4 ent_spread), ent_spread the fixture's."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

import bc_log_restate as blr
import bc_restate as br
from il_shapes import _columns, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = br.TOL
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def eng():
    from olympic_hip import specs
    from olympic_hip.engine import Engine
    e = Engine(0).il_configure(specs.unitree_h1("walk"))      # 11 actions: the controls of the cases with A = 11
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def d(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


def split(flat, in_dim, A):
    out, o = [], 0
    for s in br.param_shapes(in_dim, A):
        n = int(np.prod(s))
        out.append(flat[o:o + n].reshape(s))
        o += n
    return out


def switch_rows():
    """The largest n that runs 16-row tiles and the smallest that runs 32-row tiles (oly_ilmlp_forward's choice:
    32-row tiles once they fill two workgroups per CU)."""
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    return 64 * cu - 32, 64 * cu - 31


def sg_case(n, D, A, seed, standardizer=True, clip=2.0):
    """nn.Linear's default initialisation (log_sigma within -+0.5), columns of different scale and offset (unit columns
    without a Standardizer), bounds of unequal widths, noise clipped to -+2 (|a_raw| < 4 at every shape of the table;
    clip=None leaves the noise as drawn, for tests/sg_saturation.py's table)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * A)]
    params = [t.detach().numpy().copy() for lin in lins for t in (lin.weight, lin.bias)]
    rng = np.random.default_rng(500 + seed)
    scale, shift = _columns(rng, D) if standardizer else (np.full(D, 0.5), np.zeros(D))
    x = (rng.standard_normal((n, D)) * scale + shift).astype(np.float32)
    min_a, max_a = -rng.uniform(0.5, 2.0, A), rng.uniform(0.5, 3.0, A)
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)
    eps = rng.standard_normal((n, A))
    eps = (eps if clip is None else np.clip(eps, -clip, clip)).astype(np.float32)
    return dict(params=params, x=x, central=central, delta=delta, eps=eps, standardizer=standardizer)


def float64_of(k, cs, A, lo=-20.0, hi=2.0):
    """mu, log_sigma, a_raw, action, log_prob in float64 on the device from the float32 parameters, the statistics cs
    (or None) and the case's noise."""
    x = d(k["x"]).double()
    if cs is not None:
        cnt = cs[0] + 1e-2
        mean = cs[1] / cnt
        std = torch.sqrt(torch.clamp((cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
        x = ((x - mean) / std).float().double()
    w = [d(p).double() for p in k["params"]]
    y = torch.relu(torch.relu(x @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5]
    mu, ls = y[:, :A], torch.clamp(y[:, A:], lo, hi)
    raw = mu + ls.exp() * d(k["eps"]).double()
    action = torch.tanh(raw) * d(k["delta"]).double() + d(k["central"]).double()
    return mu, ls, raw, action, blr.log_prob(mu, ls, raw)


def run_sg(eng, k, A, eps=True, want=("log_prob", "mu", "log_sigma"), **kw):
    n, D = k["x"].shape
    packed = eng.ilmlp_pack(*[d(p) for p in k["params"]])
    cs = torch.zeros((3, D), dtype=F64, device="cuda") if k["standardizer"] else None
    bufs = dict(action=guarded((n, A), F32), log_prob=guarded((n,), F32), mu=guarded((n, A), F32),
                log_sigma=guarded((n, A), F32))
    o = eng.sg_act(d(k["x"]), packed, d(k["central"]), d(k["delta"]), colstats=cs, eps=d(k["eps"]) if eps else None,
                   want=want, out={key: g.t for key, g in bufs.items() if key == "action" or key in want}, **kw)
    torch.cuda.synchronize()
    assert all(g.intact() for g in bufs.values()), "a write outside an output"
    return o, cs, packed


#         n, in, A, standardizer; "lo" / "hi": switch_rows(), resolved on the device
SHAPES = [(1, 1, 1, True), (45, 19, 7, True), (33, 33, 11, True), (40, 64, 16, False), ("lo", 32, 11, True), ("hi", 32, 11, True)]
SHAPE_IDS = [f"n{n}-in{D}-A{A}" + ("" if st else "-nostd") for n, D, A, st in SHAPES]


def rows_of(n):
    return switch_rows()[("lo", "hi").index(n)] if isinstance(n, str) else n


# ------------------------------------------------------------------------------ 1. oly_sg_act's bits
@pytest.mark.parametrize("n,D,A,st", SHAPES, ids=SHAPE_IDS)
def test_bits_against_the_forward_and_il_ctrl(eng, n, D, A, st):
    n = rows_of(n)
    k = sg_case(n, D, A, seed=n % 97 + D + A, standardizer=st)
    ctrl = A == 11
    want = ("log_prob", "mu", "log_sigma") + (("ctrl",) if ctrl else ())
    o, cs, packed = run_sg(eng, k, A, want=want)
    if st:
        assert float(cs[0, 0]) == n, "the call added the rows to the statistics"
        assert torch.equal(cs, eng.col_stats(d(k["x"]), None))
    y = eng.ilmlp_forward(d(k["x"]), packed, 2 * A, "identity", colstats=cs)
    assert torch.equal(o["mu"], y[:, :A]) and torch.equal(o["log_sigma"], torch.clamp(y[:, A:], -20.0, 2.0))
    if ctrl:
        assert torch.equal(o["ctrl"], eng.il_ctrl(o["action"]))
        o64, _, _ = run_sg(eng, k, A, want=("ctrl",), ctrl_f64=True)
        assert o64["ctrl"].dtype == F64 and torch.equal(o64["ctrl"], eng.il_ctrl(o64["action"], ctrl_f64=True))
        assert torch.equal(o64["action"], o["action"])
    # deterministic: the squashed mean, nothing drawn; two runs give the same bits
    det, cs2, _ = run_sg(eng, k, A, eps=False)
    assert torch.equal(det["mu"], o["mu"]) and (cs is None or torch.equal(cs2, cs))
    ref = torch.tanh(det["mu"].double()) * d(k["delta"]).double() + d(k["central"]).double()
    assert float((det["action"].double() - ref).abs().max()) <= TOL
    again, _, _ = run_sg(eng, k, A, want=want)
    for key in ("action", "log_prob", "mu", "log_sigma"):
        assert torch.equal(again[key], o[key]), key


# ------------------------------------------------------------------------------ 2. oly_sg_act against float64
@pytest.mark.parametrize("n,D,A,st", SHAPES, ids=SHAPE_IDS)
def test_action_and_log_prob_against_float64(eng, n, D, A, st):
    n = rows_of(n)
    k = sg_case(n, D, A, seed=n % 97 + D + A, standardizer=st)
    o, cs, _ = run_sg(eng, k, A)
    mu64, ls64, raw64, a64, lp64 = float64_of(k, cs, A)
    assert float(ls64.abs().max()) < 1.0 and float(raw64.abs().max()) < 4.0, "the case's conditioning"
    err_a = float((o["action"].double() - a64).abs().max())
    err_lp = float(((o["log_prob"].double() - lp64).abs() / lp64.abs().clamp(min=1.0)).max())
    print(f"n={n} in={D} A={A}: action {err_a:.3e}, log_prob relative {err_lp:.3e}")
    assert err_a <= TOL
    assert o["log_prob"].shape == (n,) and err_lp <= TOL


def test_log_sigma_past_both_clamp_bounds(eng):
    """K24's policy test case: log_sigma forced below log_std_min and above log_std_max; the clamped outputs are exact,
    the log-probability finite (its value is ill conditioned at log_sigma = -20, in torch as here)."""
    n, D, A = 45, 19, 7
    k = sg_case(n, D, A, seed=21)
    k["params"][5][A] = -25.0
    k["params"][5][A + 1] = 3.0
    o, cs, packed = run_sg(eng, k, A)
    y = eng.ilmlp_forward(d(k["x"]), packed, 2 * A, "identity", colstats=cs)
    assert torch.equal(o["log_sigma"], torch.clamp(y[:, A:], -20.0, 2.0))
    assert bool((o["log_sigma"][:, 0] == -20.0).all()) and bool((o["log_sigma"][:, 1] == 2.0).all())
    assert float(o["log_sigma"][:, 2:].abs().max()) < 1.0
    assert bool(torch.isfinite(o["log_prob"]).all()) and bool(torch.isfinite(o["action"]).all())
    mu64, ls64, raw64, a64, _ = float64_of(k, cs, A)
    assert float((o["action"].double() - a64).abs().max()) <= TOL
    # other bounds than the defaults reach the kernel
    o2, _, _ = run_sg(eng, k, A, log_std_min=-0.25, log_std_max=0.125)
    assert float(o2["log_sigma"].min()) == -0.25 and float(o2["log_sigma"].max()) == 0.125


# ------------------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing():
    import ctypes as C
    from olympic_hip import _abi, _ffi, specs
    from olympic_hip._ffi import OlyError
    from olympic_hip.engine import Engine
    e = Engine(0)
    try:
        npk = int(_ffi.lib().oly_ilmlp_packed_floats(32, 512, 256, 22))
        pk = torch.zeros(npk + 4, device="cuda")
        x = torch.ones((4, 64), dtype=F32, device="cuda")
        cs = torch.zeros((3, 64), dtype=F64, device="cuda")
        cen, dl = torch.zeros(16, device="cuda"), torch.ones(16, device="cuda")
        act = torch.full((4, 16), -3.0, device="cuda")
        ctrl = torch.zeros((4, 64), device="cuda")

        def block(**kw):
            f = dict(n=4, in_dim=32, act_dim=11, update_stats=1, x=x.data_ptr(), colstats=cs.data_ptr(),
                     packed=pk.data_ptr(), log_std_min=-20.0, log_std_max=2.0, central=cen.data_ptr(), delta=dl.data_ptr(),
                     eps=None, action=act.data_ptr(), log_prob=None, mu=None, log_sigma=None, ctrl=None, out_flags=0, pad=0)
            f.update(kw)
            return _abi.SGAct(**f)

        bad = [dict(n=0), dict(n=-1), dict(in_dim=0), dict(in_dim=65), dict(act_dim=0), dict(act_dim=17), dict(x=None),
               dict(packed=None), dict(central=None), dict(delta=None), dict(action=None),
               dict(colstats=None),                                  # update_stats without colstats
               dict(packed=pk.data_ptr() + 4),                       # not 16-byte aligned
               dict(log_std_min=2.5), dict(log_std_min=float("nan")), dict(log_std_max=float("nan")),
               dict(ctrl=ctrl.data_ptr())]                           # ctrl before any model is configured
        for kw in bad:
            with pytest.raises(OlyError):
                e.ctx.call("oly_sg_act", C.byref(block(**kw)), e._s())
        with pytest.raises(OlyError):
            e.ctx.call("oly_sg_act", None, e._s())
        e.il_configure(specs.unitree_h1("walk"))
        with pytest.raises(OlyError):
            e.ctx.call("oly_sg_act", C.byref(block(act_dim=10, ctrl=ctrl.data_ptr())), e._s())     # n_act is 11
        # the engine's own checks
        for kw in (dict(want=("ctrl", "nothing")), dict(log_std_min=3.0)):
            with pytest.raises(OlyError):
                e.sg_act(x[:, :32].contiguous(), pk[:npk], cen[:11].contiguous(), dl[:11].contiguous(), colstats=None, **kw)
        with pytest.raises(OlyError):
            e.sg_act(x[:, :32].contiguous(), pk[:npk], torch.zeros(17, device="cuda"), torch.ones(17, device="cuda"))
        torch.cuda.synchronize()
        assert float(cs.abs().max()) == 0.0 and bool((act == -3.0).all()), "a refused call launches nothing"
        # the context is still usable: this call runs
        e.ctx.call("oly_sg_act", C.byref(block(ctrl=ctrl.data_ptr())), e._s())
        torch.cuda.synchronize()
        assert cs[0, :32].tolist() == [4.0] * 32 and bool(torch.isfinite(act[:, :11].reshape(-1)[:44]).all())
    finally:
        torch.cuda.synchronize()
        e.ctx.close()


def test_logged_fit_refusals(eng):
    from olympic_hip._ffi import OlyError
    c = br.CASES[1]
    k = br.build(c)
    param = d(br.flat(k["params"]).astype(np.float32))
    z = torch.zeros_like(param)
    packed = eng.ilmlp_pack(*split(param, c.in_dim, c.A))
    ws = eng.bc_fit_log_ws(32, c.in_dim, c.A)
    args = (d(k["states"]), d(k["targets"]), d(k["idx"]), None, param, z, z.clone(), packed)
    noise = torch.zeros((3, 32, c.A), device="cuda")
    with pytest.raises(OlyError, match="ws"):
        eng.bc_fit_steps_log(*args, eng.bc_fit_ws(32, c.in_dim, c.A), 0, 1e-3, 1, 0, noise)      # the unlogged fit's workspace
    with pytest.raises(OlyError, match="logging_iter"):
        eng.bc_fit_steps_log(*args, ws, 0, 1e-3, 0, 0, noise)
    with pytest.raises(OlyError, match="iter0"):
        eng.bc_fit_steps_log(*args, ws, 0, 1e-3, 1, -1, noise)
    with pytest.raises(OlyError, match="noise"):
        eng.bc_fit_steps_log(*args, ws, 0, 1e-3, 1, 0, None)
    with pytest.raises(OlyError, match="noise"):
        eng.bc_fit_steps_log(*args, ws, 0, 1e-3, 2, 0, noise)                                     # two steps log, not three
    # straight at the C entry: eps NULL while a step logs, logging_iter 0
    import ctypes as C
    from olympic_hip import _abi
    out = torch.zeros((3, 4), dtype=F64, device="cuda")
    fit = _abi.BCFit(in_dim=c.in_dim, act_dim=c.A, batch=32, n_rows=c.n_rows, step=0, lr=1e-3, beta1=0.9, beta2=0.999,
                     eps=1e-8, weight_decay=0.0, log_std_min=-20.0, log_std_max=2.0, nll_eps=1e-6,
                     states=args[0].data_ptr(), targets=args[1].data_ptr(), idx=args[2].data_ptr(), colstats=None,
                     param=param.data_ptr(), m=args[5].data_ptr(), v=args[6].data_ptr(), packed=packed.data_ptr(),
                     ws=ws.data_ptr(), ws_floats=int(ws.numel()), out=out.data_ptr())
    for li, it0, e in ((1, 0, None), (0, 0, noise.data_ptr()), (3, 1, None)):       # (3, 1): step 2 of the call logs
        with pytest.raises(OlyError):
            eng.ctx.call("oly_bc_fit_steps_log", C.byref(_abi.BCFitLog(fit=fit, logging_iter=li, iter0=it0, eps=e)), 3, eng._s())
    torch.cuda.synchronize()
    assert torch.equal(param, d(br.flat(k["params"]).astype(np.float32))) and float(out.abs().max()) == 0.0
    # no step of the call logs: eps may be NULL, and the fit is oly_bc_fit_steps'
    eng.ctx.call("oly_bc_fit_steps_log", C.byref(_abi.BCFitLog(fit=fit, logging_iter=5, iter0=1, eps=None)), 3, eng._s())
    torch.cuda.synchronize()
    assert float(out[:, 0].min()) > 0 and float(out[:, 3].abs().max()) == 0.0


# ------------------------------------------------------------------------------ the logged fit on the device
def run_logged(eng, in_dim, A, k, steps, lr, standardizer, eps, li, cuts=None, iter0=0):
    """The logged fit on the device, cut into calls of `cuts` steps (None: one call).  Returns the device state."""
    b = k["batch"]
    param = d(br.flat(k["params"]).astype(np.float32))
    st = dict(param=param, m=torch.zeros_like(param), v=torch.zeros_like(param),
              colstats=torch.zeros((3, in_dim), dtype=F64, device="cuda") if standardizer else None,
              out=torch.full((steps, 4), float("nan"), dtype=F64, device="cuda"))
    st["packed"] = eng.ilmlp_pack(*split(param, in_dim, A))
    ws = eng.bc_fit_log_ws(b, in_dim, A)
    states, targets, idx, noise = d(k["states"]), d(k["targets"]), d(k["idx"]), d(eps)
    s = used = 0
    for n in (cuts or (steps,)):
        nl = len(blr.logged_steps(n, li, iter0 + s))
        eng.bc_fit_steps_log(states, targets, idx[s:s + n].contiguous(), st["colstats"], param, st["m"], st["v"], st["packed"],
                             ws, s, lr, li, iter0 + s, noise[used:used + nl].contiguous() if nl else None,
                             log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX, nll_eps=br.NLL_EPS, out=st["out"][s:s + n])
        s, used = s + n, used + nl
    assert s == steps and used == len(eps)
    torch.cuda.synchronize()
    return st


def same_state(a, b):
    for key in ("param", "m", "v", "packed", "colstats"):
        if a[key] is None:
            assert b[key] is None
        else:
            assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["out"].view(torch.int64), b["out"].view(torch.int64)), "out (NaN where a step does not log)"


# ------------------------------------------------------------------------------ 4. against the reference-run fixture
@pytest.mark.parametrize("li", (1, 2))
def test_logged_fit_against_the_reference_run_fixture(eng, golden, li):
    g = golden("bc_log/bc_log.npz")
    k, gen = blr.fixture_case(g)
    k["targets"] = eng.bc_targets(d(k["actions"]), d(k["central"]), d(k["delta"])).cpu().numpy()
    A, in_dim, steps = gen.ACT_DIM, gen.IN_DIM, gen.N_STEPS
    st = run_logged(eng, in_dim, A, k, steps, gen.LR, True, g[f"eps_li{li}"], li)
    cs = st["colstats"].cpu().numpy()
    assert np.all(cs[0] + 1e-2 == g[f"st_count_li{li}"][0])
    assert float(cs[0, 0]) + 1e-2 == (0.01 + 2 * 6 * 32 if li == 1 else 0.01 + 32 * (6 + 3))
    st_sum, st_sumsq = g[f"st_sum_li{li}"], g[f"st_sumsq_li{li}"]
    assert np.all(np.abs(cs[1] - st_sum) <= TOL * np.maximum(1, np.abs(st_sum)))
    assert np.all(np.abs(cs[2] + 1e-2 - st_sumsq) <= TOL * np.maximum(1, np.abs(st_sumsq)))
    got = split(st["param"], in_dim, A)
    for i, name in enumerate(NAMES):
        if name != "w2":
            err = float(np.abs(got[i].cpu().numpy().astype(np.float64) - g[f"{name}_li{li}"]).max())
            print(f"logging_iter {li} {name}: |kernel - fixture| max {err:.3e}")
            assert err <= TOL, (name, err)
    out, s = st["out"].cpu().numpy(), g[f"scalars_li{li}"]
    rel = np.abs(out[:, :3] - s[:, :3]) / np.abs(s[:, :3])
    assert rel.max() <= TOL, rel
    logged = blr.logged_steps(steps, li)
    for t in range(steps):
        if t in logged:
            err, tol = abs(out[t, 3] - s[t, 3]), blr.ent_tol(s[t, 3], g["ent_spread"])
            print(f"logging_iter {li} step {t}: entropy {s[t, 3]:.6f}, |kernel - fixture| {err:.3e}, tolerance {tol:.3e}")
            assert err <= tol
        else:
            assert np.isnan(out[t, 3])
    # the unlogged fit cannot reach these statistics
    assert float(cs[0, 0]) > 6 * 32


# ------------------------------------------------------------------------------ 5. against the float64 restatement
assert [(c.in_dim, c.A, c.batch, c.standardizer) for c in blr.TABLED] == [(1, 1, 1, True), (33, 11, 33, True), (64, 16, 256, False)]


@pytest.mark.parametrize("c", blr.RUNS, ids=[br.case_id(c) for c in blr.RUNS])
def test_logged_fit_against_float64(eng, golden, c):
    """(1, 1, 1), (33, 11, 33) and (64, 16, 256) of bc_restate.CASES as tabled, and the twins of the two saturated ones
    without the saturation (bc_log_restate.PLAIN says why and how their seed was chosen).  On a saturated case the
    float32 log-probability is no function of its float64 value, in torch as here (test_policy_log_prob_against_float64's
    docstring, tests/test_gpu_bc_fit.py): there the parameters, the statistics and the first three scalars are held to
    the restatement and the entropy to be finite; the entropy tolerance is held on the plain cases."""
    k = br.build(c)
    li = blr.logging_iter_of(c)
    eps = blr.noise(c, li)
    ref = blr.restate(c.in_dim, c.A, k, c.steps, c.lr, c.standardizer, eps, li)
    st = run_logged(eng, c.in_dim, c.A, k, c.steps, c.lr, c.standardizer, eps, li)
    assert_logged_fit_matches_float64(c, k, li, st, ref, float(golden("bc_log/bc_log.npz")["ent_spread"]))


def assert_logged_fit_matches_float64(c, k, li, st, ref, spread):
    """The device state `st` of run c after the logged fit (run_logged's keys) against the float64 restatement `ref`."""
    saturated = c.saturated
    got = [t.double().cpu().numpy() for t in split(st["param"], c.in_dim, c.A)]
    for name, a, r in zip(NAMES, got, ref["params"][-1]):
        err = float(np.abs(a - r).max())
        print(f"{br.case_id(c)} {name}: |kernel - f64| max {err:.3e}")
        assert err <= TOL, (name, err)
    if c.standardizer:
        cs = st["colstats"].cpu().numpy()
        assert np.array_equal(cs[0], ref["colstats"][0]) and float(np.abs(cs - ref["colstats"]).max()) <= TOL
        assert cs[0, 0] == k["batch"] * (c.steps + len(blr.logged_steps(c.steps, li)))
    out = st["out"].cpu().numpy()
    rel = np.abs(out[:, :3] - ref["out"][:, :3]) / np.abs(ref["out"][:, :3])
    assert rel.max() <= TOL, rel
    for t in range(c.steps):
        if t not in blr.logged_steps(c.steps, li):
            assert np.isnan(out[t, 3])
        elif saturated:
            assert np.isfinite(out[t, 3])
        else:
            err, tol = abs(out[t, 3] - ref["out"][t, 3]), blr.ent_tol(ref["out"][t, 3], spread)
            print(f"{br.case_id(c)} step {t}: entropy {ref['out'][t, 3]:.6f}, |kernel - f64| {err:.3e}, tolerance {tol:.3e}")
            assert err <= tol


# ------------------------------------------------------------------------------ 6. bits
BITS = br.CASES[3]._replace(steps=6)       # 33 rows (16 + 16 + 1), 22 output columns, a Standardizer


def test_two_runs_give_the_same_bits_and_cuts_do_not_matter(eng):
    k = br.build(BITS)
    for li in (1, 2, 3):
        eps = blr.noise(BITS, li)
        one = run_logged(eng, BITS.in_dim, BITS.A, k, 6, BITS.lr, True, eps, li)
        same_state(one, run_logged(eng, BITS.in_dim, BITS.A, k, 6, BITS.lr, True, eps, li))
        same_state(one, run_logged(eng, BITS.in_dim, BITS.A, k, 6, BITS.lr, True, eps, li, cuts=(2, 4)))
        same_state(one, run_logged(eng, BITS.in_dim, BITS.A, k, 6, BITS.lr, True, eps, li, cuts=(1,) * 6))
        out = one["out"].cpu().numpy()
        logged = blr.logged_steps(6, li)
        assert np.all(np.isfinite(out[logged, 3])) and np.all(np.isnan(np.delete(out[:, 3], logged)))
        assert float(one["colstats"][0, 0]) == 33 * (6 + len(logged))
        assert torch.equal(one["packed"], eng.ilmlp_pack(*split(one["param"], BITS.in_dim, BITS.A)))


def test_iter0_carries_the_phase_across_calls(eng):
    """logging_iter 3 from iteration 1: iterations 3 and 6 log, steps 2 and 5 of the fit; the cut (3, 3) puts a
    non-logging step between logging ones in each call, the cut (2, 1, 3) a call without a logging step."""
    k = br.build(BITS)
    eps = blr.noise(BITS, 3, iter0=1)
    assert blr.logged_steps(6, 3, 1) == [2, 5] and len(eps) == 2
    one = run_logged(eng, BITS.in_dim, BITS.A, k, 6, BITS.lr, True, eps, 3, iter0=1)
    same_state(one, run_logged(eng, BITS.in_dim, BITS.A, k, 6, BITS.lr, True, eps, 3, cuts=(3, 3), iter0=1))
    same_state(one, run_logged(eng, BITS.in_dim, BITS.A, k, 6, BITS.lr, True, eps, 3, cuts=(2, 1, 3), iter0=1))
    out = one["out"].cpu().numpy()
    assert np.isfinite(out[[2, 5], 3]).all() and np.isnan(out[[0, 1, 3, 4], 3]).all()
    assert float(one["colstats"][0, 0]) == 33 * 8
    other = run_logged(eng, BITS.in_dim, BITS.A, k, 6, BITS.lr, True, eps, 3, iter0=0)     # steps 0 and 3 log instead
    assert not torch.equal(other["param"], one["param"])


def test_without_a_standardizer_the_fit_is_the_unlogged_one(eng):
    c = br.CASES[5]._replace(steps=3)
    k = br.build(c)
    eps = blr.noise(c, 1)
    logged = run_logged(eng, c.in_dim, c.A, k, 3, c.lr, False, eps, 1)
    same_state(logged, run_logged(eng, c.in_dim, c.A, k, 3, c.lr, False, eps, 1, cuts=(1, 2)))
    param = d(br.flat(k["params"]).astype(np.float32))
    m, v = torch.zeros_like(param), torch.zeros_like(param)
    packed = eng.ilmlp_pack(*split(param, c.in_dim, c.A))
    out = eng.bc_fit_steps(d(k["states"]), d(k["targets"]), d(k["idx"]), None, param, m, v, packed,
                           eng.bc_fit_ws(k["batch"], c.in_dim, c.A), 0, c.lr)
    torch.cuda.synchronize()
    for key, t in (("param", param), ("m", m), ("v", v), ("packed", packed)):
        assert torch.equal(logged[key], t), key
    assert torch.equal(logged["out"][:, :3], out) and bool(torch.isfinite(logged["out"][:, 3]).all())
    # with a Standardizer and no logging step in the call, too
    c2 = br.CASES[1]
    k2 = br.build(c2)
    quiet = run_logged(eng, c2.in_dim, c2.A, k2, 3, c2.lr, True, np.zeros((0, 32, c2.A), np.float32), 7, iter0=1)
    param = d(br.flat(k2["params"]).astype(np.float32))
    m, v = torch.zeros_like(param), torch.zeros_like(param)
    cs = torch.zeros((3, c2.in_dim), dtype=F64, device="cuda")
    packed = eng.ilmlp_pack(*split(param, c2.in_dim, c2.A))
    out = eng.bc_fit_steps(d(k2["states"]), d(k2["targets"]), d(k2["idx"]), cs, param, m, v, packed,
                           eng.bc_fit_ws(32, c2.in_dim, c2.A), 0, c2.lr)
    torch.cuda.synchronize()
    assert torch.equal(quiet["param"], param) and torch.equal(quiet["colstats"], cs) and torch.equal(quiet["out"][:, :3], out)


# ------------------------------------------------------------------------------ 7. the trainer: logging, resume
class Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, name, value, it):
        self.rows.append((name, value, it))


def make_policy(eng, in_dim, A, seed, standardizer=True, fused_act=False, bounds_seed=77):
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lins = [torch.nn.Linear(in_dim, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * A)]
    rng = np.random.default_rng(bounds_seed)
    min_a, max_a = -rng.uniform(0.5, 2.0, A), rng.uniform(0.5, 3.0, A)
    st = DeviceStandardizer(eng, in_dim) if standardizer else None
    return DeviceSquashedGaussianPolicy(eng, lins, min_a, max_a, standardizer=st, fused_act=fused_act)


def make_trainer(eng, seed, demo, **kw):
    from olympic_hip.bc import DeviceBehavioralCloning
    pol = make_policy(eng, demo["states"].shape[1], demo["actions"].shape[1], seed)
    return DeviceBehavioralCloning(eng, pol, demo, lr=1e-3, **kw)


def trainer_state(tr):
    return [tr.policy.param, tr.policy.packed, tr.exp_avg, tr.exp_avg_sq, tr.policy.stand.colstats]


def test_trainer_logs_the_fourth_scalar_and_resumes(eng, tmp_path):
    from olympic_hip import il_checkpoint
    from olympic_hip._ffi import OlyError
    c = br.CASES[1]
    k = br.build(c)
    demo = dict(states=k["states"], actions=k["actions"])
    sw = Writer()
    straight = make_trainer(eng, 1, demo, batch_size=c.batch, logging_iter=2, sw=sw, empirical_entropy=True)
    idx = straight.draw_idx(6, generator=torch.Generator(device="cuda").manual_seed(3))
    eps = d(np.clip(np.random.default_rng(9).standard_normal((3, 32, c.A)), -2.5, 2.5).astype(np.float32))
    out = straight.fit_offline(6, idx=idx, eps=eps)
    assert straight.step == 6 and straight.iter == 6 and out.shape == (6, 4)
    host = out.cpu().numpy()
    assert [r[2] for r in sw.rows] == [0] * 4 + [2] * 4 + [4] * 4
    assert [r[0] for r in sw.rows[:4]] == ["GaussianNLLLoss", "Squashed Gaussian Entropy",
                                           "MSELoss (between mean & target actions)", "Squashed Gaussian Entropy (Empirical)"]
    assert [r[1] for r in sw.rows[4:8]] == [float(v) for v in host[2]]
    assert np.isfinite(host[[0, 2, 4], 3]).all() and np.isnan(host[[1, 3, 5], 3]).all()
    assert float(straight.policy.stand.colstats[0, 0]) == 32 * 9
    # the sampled entropy lies near the Gaussian one minus the tanh correction: of its order, not equal to it
    assert 0 < abs(host[0, 3] - host[0, 1]) < 3 * c.A
    with pytest.raises(OlyError, match="eps"):
        straight.fit_offline(2, idx=idx[:2].contiguous(), eps=eps)          # one of these two steps logs, not three
    with pytest.raises(OlyError, match="empirical_entropy"):
        make_trainer(eng, 1, demo, batch_size=c.batch).fit_offline(2, idx=idx[:2].contiguous(), eps=eps[:1])
    # resume mid-fit, after an odd number of steps: iteration 3 does not log, 4 does
    tr = make_trainer(eng, 1, demo, batch_size=c.batch, logging_iter=2, empirical_entropy=True)
    tr.fit_offline(3, idx=idx[:3].contiguous(), eps=eps[:2].contiguous())
    for how in ("state_dict", "file"):
        fresh = make_trainer(eng, 2, demo, batch_size=c.batch, logging_iter=2, empirical_entropy=True)
        assert not torch.equal(fresh.policy.param, tr.policy.param)
        if how == "state_dict":
            fresh.load_state_dict(tr.state_dict())
        else:
            path = il_checkpoint.save(str(tmp_path / "bc.pt"), tr, note="three steps")
            assert il_checkpoint.load(path, fresh)["note"] == "three steps"
        assert fresh.step == 3 and fresh.iter == 3
        out2 = fresh.fit_offline(3, idx=idx[3:].contiguous(), eps=eps[2:].contiguous())
        for a, b in zip(trainer_state(fresh), trainer_state(straight)):
            assert torch.equal(a, b)
        assert torch.equal(out2.view(torch.int64), out[3:].view(torch.int64)), "the fourth column included"
    # eps drawn from the generator after idx: two runs from one seed agree, and the draw order is idx, then eps
    runs = []
    for _ in range(2):
        t = make_trainer(eng, 1, demo, batch_size=c.batch, logging_iter=2, empirical_entropy=True)
        gen = torch.Generator(device="cuda").manual_seed(11)
        runs.append((t.fit_offline(4, generator=gen), t.policy.param.clone()))
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64)) and torch.equal(runs[0][1], runs[1][1])
    gen = torch.Generator(device="cuda").manual_seed(11)
    t = make_trainer(eng, 1, demo, batch_size=c.batch, logging_iter=2, empirical_entropy=True)
    idx4 = t.draw_idx(4, generator=gen)
    eps4 = torch.randn((2, 32, c.A), dtype=F32, device="cuda", generator=gen)
    assert torch.equal(t.fit_offline(4, idx=idx4, eps=eps4).view(torch.int64), runs[0][0].view(torch.int64))


# ------------------------------------------------------------------------------ 8. the fused policy; ILCore
def test_fused_policy_has_the_unfused_contract(eng):
    in_dim, A, n = 32, 11, 45
    rng = np.random.default_rng(5)
    x = d((rng.standard_normal((n, in_dim)) * rng.uniform(0.3, 3, in_dim) + rng.standard_normal(in_dim)).astype(np.float32))
    plain, fused = make_policy(eng, in_dim, A, 4), make_policy(eng, in_dim, A, 4, fused_act=True)
    assert torch.equal(plain.param, fused.param) and fused.fused_act and not plain.fused_act
    g1, g2 = (torch.Generator(device="cuda").manual_seed(8) for _ in range(2))
    for step in range(2):                       # twice: the statistics accumulate alike
        a1, c1 = plain.act(x, generator=g1, ctrl=True)
        a2, c2 = fused.act(x, generator=g2, ctrl=True)
        assert torch.equal(g1.get_state(), g2.get_state()), "the two modes consume the same noise"
        assert torch.equal(plain.stand.colstats, fused.stand.colstats) and float(fused.stand.colstats[0, 0]) == n * (step + 1)
        assert float((a1 - a2).abs().max()) <= TOL and a2.shape == (n, A)
        assert torch.equal(c2, eng.il_ctrl(a2)) and c1.shape == c2.shape
    d1, n1 = plain.act(x, deterministic=True)
    d2, n2 = fused.act(x, deterministic=True)
    assert n1 is None and n2 is None and float((d1 - d2).abs().max()) <= TOL
    assert torch.equal(g1.get_state(), g2.get_state()), "deterministic: nothing drawn"
    eps = d(np.clip(rng.standard_normal((n, A)), -2.5, 2.5).astype(np.float32))
    p1, l1 = plain.compute_action_and_log_prob(x, eps=eps)
    p2, l2 = fused.compute_action_and_log_prob(x, eps=eps)
    assert float((p1 - p2).abs().max()) <= TOL and l2.shape == (n,)
    assert float(((l1 - l2).abs() / l1.abs().clamp(min=1.0)).max()) <= TOL
    # get_mu_log_sigma and predict are untouched
    m1, s1 = plain.get_mu_log_sigma(x)
    m2, s2 = fused.get_mu_log_sigma(x)
    assert torch.equal(m1, m2) and torch.equal(s1, s2) and torch.equal(plain.predict(x), fused.predict(x))
    # without a Standardizer
    bare = make_policy(eng, in_dim, A, 4, standardizer=False, fused_act=True)
    ref = make_policy(eng, in_dim, A, 4, standardizer=False)
    xs = (0.3 * x).contiguous()
    assert float((bare.act(xs, eps=eps)[0] - ref.act(xs, eps=eps)[0]).abs().max()) <= TOL


class NoAgent:
    def fit(self, dataset, generator=None):
        return None


def test_core_steps_and_evaluates_with_the_fused_policy():
    from olympic_hip.envs import LocoEnvBase
    from olympic_hip.il_core import ILCore
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=64, seed=0)
    vec = env.vec
    try:
        vec.spec.horizon = vec.info.horizon = 5
        e = vec.eng
        plain = make_policy(e, vec.spec.n_obs, vec.spec.n_act, 6)
        fused = make_policy(e, vec.spec.n_obs, vec.spec.n_act, 6, fused_act=True)
        obs = vec.reset()
        acts = []
        for pol in (plain, fused):
            core = ILCore(NoAgent(), vec, pol, generator=torch.Generator(device="cuda").manual_seed(4))
            acts.append(core._step(obs, core._needs_ctrl())[0].clone())
        err = float((acts[0] - acts[1]).abs().max())
        print(f"one _step: |fused - unfused| max {err:.3e}")
        assert acts[1].shape == (64, vec.spec.n_act) and err <= TOL
        core = ILCore(NoAgent(), vec, fused, generator=torch.Generator(device="cuda").manual_seed(3))
        o = core.evaluate(64)
        assert o["n_episodes"] == 64 and 0 < o["L"] <= 5 and np.isfinite(o["R_mean"])
        assert float(fused.stand.colstats[0, 0]) >= 64 * (1 + o["L"])
    finally:
        torch.cuda.synchronize()
        vec.eng.ctx.close()
        gc.collect()


def test_example_takes_the_two_flags(tmp_path):
    import json
    import subprocess
    log = tmp_path / "bc.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bc_fit.py"), "--envs", "64", "--collect", "8",
                        "--steps", "40", "--eval-episodes", "64", "--horizon", "5", "--log", "--fused-act",
                        "--empirical-entropy", "--json", str(log)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(log.read_text())
    assert rec["steps"] == 40 and "Squashed Gaussian Entropy (Empirical)" in p.stdout
    assert rec["loss_last"] < rec["loss_first"], rec
