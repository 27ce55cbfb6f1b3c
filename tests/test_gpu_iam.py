"""The inverse action model on the MI355X, from the kernel layer to the agents (the second half of the file: the model on a
ring, the whole from-observations agents against the reference's own IQfO_SAC.fit / LSIQfO.fit run in tests/golden/iam_fit
and against iqfo_sac.py's sequence written out, their checkpoint and refusals).  The kernel layer: oly_bc_fit_steps /
oly_bc_fit_steps_log with oly_bc_fit.pair and oly_sg_act with its two-table fields, bit for bit against the same calls on the rows that torch materialises (and
oly_bc_targets un-squashes), against the float64 twins of tests/iam_restate.py, their bits across runs and cuts, every
operand fenced (tests/fences.py), and the refusals.  These are the fenced runs of the paired paths: the entry points are
K24's and K25's, whose unpaired runs tests/il_fence_ledger.py names."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import bc_restate as br
import iam_restate as ir
from fences import Bufs

pytestmark = pytest.mark.gpu
TOL = ir.TOL
F32, F64, I32 = torch.float32, torch.float64, torch.int32
IDS = [ir.case_id(c) for c in ir.CASES]
KEYS = ("param", "m", "v", "packed", "colstats", "out")


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def d(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


_BUILT = {}


def case(c):
    """The case's arrays, built once and shared; callers leave them unchanged."""
    if c not in _BUILT:
        _BUILT[c] = ir.build(c)
    return _BUILT[c]


def split(flat, in_dim, A):
    out, o = [], 0
    for s in br.param_shapes(in_dim, A):
        n = int(np.prod(s))
        out.append(flat[o:o + n].reshape(s))
        o += n
    return out


def fit_state(eng, c, k, b, n_steps, width):
    """Fenced parameter, moments, packed stream, statistics, out [n_steps, width] and a workspace of exactly the floats
    the entry point asks for."""
    from olympic_hip._ffi import lib
    D = c.d1 + c.d2
    flat = br.flat(k["params"]).astype(np.float32)
    param = b.inp("param", flat)
    b.inp("m", np.zeros_like(flat))
    b.inp("v", np.zeros_like(flat))
    b.inp("packed", eng.ilmlp_pack(*split(d(flat), D, c.A)))
    if c.standardizer:
        b.inp("colstats", np.zeros((3, D)))
    b.out("out", (n_steps, width), F64)
    ws_fn = lib().oly_bc_fit_ws if width == 3 else lib().oly_bc_fit_log_ws
    b.out("ws", (int(ws_fn(c.batch, D, c.A)),), F32)
    return param


def run_fit(eng, c, k, paired, cuts=None, n_steps=ir.STEPS, log=None, **adam):
    """n_steps fits of case c, cut into calls of `cuts` steps.  paired: the two tables, idx and the raw actions;
    else the materialised table and oly_bc_targets' targets.  log: (logging_iter, noise [n_logged, batch, A]).
    Returns the fenced buffers after the call, checked."""
    b = Bufs()
    fit_state(eng, c, k, b, n_steps, 4 if log else 3)
    idx = b.inp("idx", k["idx"][:n_steps])
    central, delta = b.inp("central", k["central"]), b.inp("delta", k["delta"])
    actions = b.inp("actions", k["actions"], gathered=True)
    if paired:
        states = b.inp("states", k["states"], gathered=True)
        pair = dict(x2=b.inp("next_states", k["next_states"], gathered=True), actions=actions, central=central, delta=delta,
                    d1=c.d1, d2=c.d2)
        targets = None
    else:
        states = b.inp("table", torch.cat([d(k["states"])[:, :c.d1], d(k["next_states"])[:, :c.d2]], dim=1), gathered=True)
        targets = b.out("targets", (len(k["actions"]), c.A), F32)
        eng.bc_targets(actions, central, delta, out=targets)
        pair = None
    noise = b.inp("noise", log[1]) if log else None
    st = {key: b[key].t if key in b else None for key in KEYS}
    s = 0
    for n in (cuts or (n_steps,)):
        kw = dict(log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX, nll_eps=br.NLL_EPS, out=st["out"][s:s + n], pair=pair,
                  **adam)
        args = (states, targets, idx[s:s + n], st["colstats"], st["param"], st["m"], st["v"], st["packed"], b["ws"].t, s, 1e-3)
        if log:
            logged = eng.bc_logged_steps(s, log[0], 0)
            eng.bc_fit_steps_log(*args, log[0], s, noise[len(logged):len(logged) + len(eng.bc_logged_steps(n, log[0], s))],
                                 **kw)
        else:
            eng.bc_fit_steps(*args, **kw)
        s += n
    assert s == n_steps
    written = [key for key in KEYS if key in b and not (log and key == "out")]
    b.done(ir.case_id(c) + (" paired" if paired else " materialised"), written=written,
           finite=[key for key in KEYS if key in b and not (log and key == "out")])
    return b


def same_fit(a, b):
    for key in KEYS:
        assert (key in a) == (key in b)
        if key in a:
            assert torch.equal(a[key].bytes, b[key].bytes), key


# ------------------------------------------------------------------------------ 1. the fit, bit for bit
@pytest.mark.parametrize("c", ir.CASES, ids=IDS)
def test_paired_fit_has_the_bits_of_the_materialised_fit(eng, c):
    k = case(c)
    one = run_fit(eng, c, k, paired=True)
    same_fit(one, run_fit(eng, c, k, paired=False))
    assert float(one["param"].t.sub(d(br.flat(k["params"]).astype(np.float32))).abs().max()) > 0, "the fit stepped"
    if c.standardizer:
        assert float(one["colstats"].t[0, 0]) == ir.STEPS * c.batch
    # 5. two runs give identical bits; three calls of one step give one call of three
    same_fit(one, run_fit(eng, c, k, paired=True))
    same_fit(one, run_fit(eng, c, k, paired=True, cuts=(1, 1, 1)))


def test_paired_fit_with_weight_decay_and_other_adam_scalars(eng):
    """The paired launch B is a kernel of its own: its Adam step with weight decay, other betas and eps."""
    c = ir.CASES[4]
    k = case(c)
    adam = dict(weight_decay=1e-2, beta1=0.8, beta2=0.99, eps=1e-5)
    one = run_fit(eng, c, k, paired=True, **adam)
    same_fit(one, run_fit(eng, c, k, paired=False, **adam))
    assert not torch.equal(one["param"].t, run_fit(eng, c, k, paired=True)["param"].t), "the scalars reach the kernel"


def test_paired_logged_fit_has_the_bits_of_the_materialised_one(eng):
    c = ir.CASES[3]
    k = case(c)
    noise = np.clip(np.random.default_rng(11).standard_normal((2, c.batch, c.A)), -2, 2).astype(np.float32)
    one = run_fit(eng, c, k, paired=True, log=(2, noise))                 # steps 0 and 2 log
    two = run_fit(eng, c, k, paired=False, log=(2, noise))
    same_fit(one, two)
    out = one["out"].t
    assert bool(torch.isfinite(out[[0, 2]]).all()) and bool(torch.isfinite(out[1, :3]).all())
    assert one["out"].unwritten() == 1, "column 3 of the step that does not log is left as it was"
    assert float(one["colstats"].t[0, 0]) == 5 * c.batch, "the logging steps' rows are taken in twice"
    same_fit(one, run_fit(eng, c, k, paired=True, cuts=(1, 2), log=(2, noise)))


# ------------------------------------------------------------------------------ 3. the fit against the float64 twin
@pytest.mark.parametrize("c", ir.CASES, ids=IDS)
def test_paired_fit_against_float64(eng, c):
    k = case(c)
    D = c.d1 + c.d2
    b = run_fit(eng, c, k, paired=True, n_steps=2)
    _, ref = ir.fit_twin(c, k, steps=2)
    for name, a, r in zip(("w1", "b1", "w2", "b2", "w3", "b3"), split(b["param"].t, D, c.A), ref["params"][-1]):
        err = float(np.abs(a.double().cpu().numpy() - r).max())
        print(f"{ir.case_id(c)} {name}: |kernel - f64| max {err:.3e}")
        assert err <= TOL, (name, err)
    if c.standardizer:
        err = float(np.abs(b["colstats"].t.cpu().numpy() - ref["colstats"]).max())
        print(f"{ir.case_id(c)} colstats: {err:.3e}")
        assert err <= TOL
    rel = np.abs(b["out"].t.cpu().numpy() - ref["out"]) / np.abs(ref["out"])
    print(f"{ir.case_id(c)} scalars: relative {rel.max(axis=0)}")
    assert rel.max() <= TOL, rel


# ------------------------------------------------------------------------------ 2. the act, bit for bit
OUTS = ("action", "log_prob", "mu", "log_sigma")


def run_act(eng, c, k, n, paired, use_idx, eps=True, clip=None, stats=None):
    """One oly_sg_act on n rows of case c.  use_idx: rows k["idx"] (tables of the ring's 40 rows); else rows 0 .. n - 1 of
    tables of exactly n rows.  stats: the statistics before the call (None: zeros).  Returns the fenced buffers."""
    b = Bufs()
    D = c.d1 + c.d2
    rows = np.resize(k["idx"].reshape(-1), n) if use_idx else np.arange(n)
    if use_idx:
        rows[0], rows[-1] = len(k["states"]) - 1, 0 if n > 1 else len(k["states"]) - 1
    take = slice(None) if use_idx else slice(0, n)
    packed = b.inp("packed", eng.ilmlp_pack(*[d(p) for p in k["params"]]))
    central, delta = b.inp("central", k["central"]), b.inp("delta", k["delta"])
    noise = b.inp("eps", k["eps"][:n]) if eps else None
    cs = b.inp("colstats", np.zeros((3, D)) if stats is None else stats) if c.standardizer else None
    out = dict(action=b.out("action", (n, c.A), F32), log_prob=b.out("log_prob", (n,), F32), mu=b.out("mu", (n, c.A), F32),
               log_sigma=b.out("log_sigma", (n, c.A), F32))
    kw = dict(colstats=cs, eps=noise, want=OUTS[1:], out=out)
    if paired:
        x = b.inp("states", k["states"][take], gathered=True)
        x2 = b.inp("next_states", k["next_states"][take], gathered=True)
        i = b.inp("idx", rows.astype(np.int32)) if use_idx else None
        lohi = (b.inp("clip_lo", clip[0]), b.inp("clip_hi", clip[1])) if clip is not None else None
        eng.sg_act(x, packed, central, delta, x2=x2, idx=i, clip=lohi, d1=c.d1, d2=c.d2, **kw)
    else:
        assert clip is None
        eng.sg_act(b.inp("x", k["table"][rows]), packed, central, delta, **kw)
    b.done(f"{ir.case_id(c)} n={n} " + ("paired" if paired else "materialised"), written=OUTS,
           finite=OUTS + ("colstats",) * bool(cs is not None))
    return b, rows


@pytest.mark.parametrize("c", ir.CASES[:5], ids=IDS[:5])
@pytest.mark.parametrize("n", (1, 17, 33))
def test_paired_act_has_the_bits_of_the_act_on_materialised_rows(eng, c, n):
    k = case(c)
    for use_idx in (True, False):
        one, rows = run_act(eng, c, k, n, True, use_idx)
        two, _ = run_act(eng, c, k, n, False, use_idx)
        for key in OUTS + ("colstats",):
            assert torch.equal(one[key].bytes, two[key].bytes), (use_idx, key)
        assert float(one["colstats"].t[0, 0]) == n
        again, _ = run_act(eng, c, k, n, True, use_idx)
        for key in OUTS + ("colstats",):
            assert torch.equal(one[key].bytes, again[key].bytes), (use_idx, key, "two runs")
    # eps = NULL: the squashed mean
    one, _ = run_act(eng, c, k, n, True, True, eps=False)
    two, _ = run_act(eng, c, k, n, False, True, eps=False)
    for key in OUTS:
        assert torch.equal(one[key].bytes, two[key].bytes), ("use_mean", key)


def test_paired_act_without_a_standardizer(eng):
    c = ir.CASES[5]
    k = case(c)
    one, _ = run_act(eng, c, k, 17, True, True)
    two, _ = run_act(eng, c, k, 17, False, True)
    for key in OUTS:
        assert torch.equal(one[key].bytes, two[key].bytes), key


@pytest.mark.parametrize("c", (ir.CASES[1], ir.CASES[3]), ids=(IDS[1], IDS[3]))
def test_clip_is_the_float64_formula(eng, c):
    k = case(c)
    n = 33
    plain, _ = run_act(eng, c, k, n, True, True)
    # bounds inside the drawn range, float64 values that float32 does not hold
    lo = k["central"].astype(np.float64) - 0.3 * k["delta"].astype(np.float64) + 1e-9
    hi = k["central"].astype(np.float64) + 0.3 * k["delta"].astype(np.float64) - 1e-9
    clipped, _ = run_act(eng, c, k, n, True, True, clip=(lo, hi))
    a = plain["action"].t.cpu().numpy()
    want = np.minimum(np.maximum(a.astype(np.float64), lo), hi).astype(np.float32)
    got = clipped["action"].t.cpu().numpy()
    assert (want != a).any() and (want == a).any(), "the clip bites on some elements and leaves others"
    assert np.array_equal(got, want)
    for key in OUTS[1:] + ("colstats",):
        assert torch.equal(plain[key].bytes, clipped[key].bytes), key


@pytest.mark.parametrize("c", ir.CASES[:5], ids=IDS[:5])
def test_paired_act_against_float64(eng, c):
    k = case(c)
    n = 33
    b, rows = run_act(eng, c, k, n, True, True)
    ref = ir.draw_twin(c, k, rows, colstats=np.zeros((3, c.d1 + c.d2)))
    for key in ("action", "mu", "log_sigma"):
        err = float(np.abs(b[key].t.double().cpu().numpy() - ref[key]).max())
        print(f"{ir.case_id(c)} {key}: |kernel - f64| max {err:.3e}")
        assert err <= TOL, (key, err)
    assert float(np.abs(b["colstats"].t.cpu().numpy() - ref["colstats"]).max()) <= TOL


# ------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(eng):
    from olympic_hip import _abi
    from olympic_hip._ffi import OlyError, lib
    c = ir.CASES[1]
    k = case(c)
    D, A, n = c.d1 + c.d2, c.A, len(k["states"])
    b = Bufs()
    flat = br.flat(k["params"]).astype(np.float32)
    param, m, v = b.inp("param", flat), b.inp("m", np.zeros_like(flat)), b.inp("v", np.zeros_like(flat))
    packed = b.inp("packed", eng.ilmlp_pack(*split(d(flat), D, A)))
    cs = b.inp("colstats", np.zeros((3, D)))
    idx = b.inp("idx", k["idx"])
    s1, s2 = b.inp("states", k["states"], gathered=True), b.inp("next_states", k["next_states"], gathered=True)
    actions = b.inp("actions", k["actions"], gathered=True)
    central, delta = b.inp("central", k["central"]), b.inp("delta", k["delta"])
    nws = int(lib().oly_bc_fit_log_ws(c.batch, D, A))
    ws, out = b.out("ws", (nws,), F32), b.out("out", (ir.STEPS, 4), F64)
    targets = b.out("targets", (n, A), F32)
    act_out, lp = b.out("action", (n, A), F32), b.out("log_prob", (n,), F32)
    lo, hi = b.inp("lo", k["min_a"]), b.inp("hi", k["max_a"])
    snap = {key: f.snapshot() for key, f in b.items()}

    def pair(**kw):
        f = dict(d1=c.d1, d2=c.d2, stride1=s1.shape[1], stride2=s2.shape[1], x2=s2.data_ptr(), actions=actions.data_ptr(),
                 central=central.data_ptr(), delta=delta.data_ptr())
        f.update(kw)
        return _abi.BCPair(**f)

    def fit(pr, **kw):
        f = dict(in_dim=D, act_dim=A, batch=c.batch, n_rows=n, step=0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                 weight_decay=0.0, log_std_min=-20.0, log_std_max=2.0, nll_eps=1e-6, states=s1.data_ptr(), targets=None,
                 idx=idx.data_ptr(), colstats=cs.data_ptr(), param=param.data_ptr(), m=m.data_ptr(), v=v.data_ptr(),
                 packed=packed.data_ptr(), ws=ws.data_ptr(), ws_floats=nws, out=out.data_ptr(), pair=C.pointer(pr))
        f.update(kw)
        return _abi.BCFit(**f)

    bad_fit = [(pair(), dict(targets=targets.data_ptr())),          # pair with targets
               (pair(x2=None), {}), (pair(actions=None), {}), (pair(central=None), {}), (pair(delta=None), {}),
               (pair(d1=0, d2=D), {}), (pair(d1=D, d2=0), {}), (pair(d1=-1, d2=D + 1), {}),
               (pair(d1=c.d1 + 1), {}), (pair(d2=c.d2 - 1), {}),    # d1 + d2 != in_dim
               (pair(), dict(in_dim=D + 1)),
               (pair(stride1=c.d1 - 1), {}), (pair(stride2=c.d2 - 1), {}), (pair(stride1=0), {})]
    for pr, kw in bad_fit:
        f = fit(pr, **kw)
        with pytest.raises(OlyError):
            eng.ctx.call("oly_bc_fit_steps", C.byref(f), ir.STEPS, eng._s())
        with pytest.raises(OlyError):
            eng.ctx.call("oly_bc_fit_steps_log", C.byref(_abi.BCFitLog(fit=f, logging_iter=1, iter0=0, eps=act_out.data_ptr())),
                         ir.STEPS, eng._s())

    def act(**kw):
        f = dict(n=n, in_dim=D, act_dim=A, update_stats=1, x=s1.data_ptr(), colstats=cs.data_ptr(), packed=packed.data_ptr(),
                 log_std_min=-20.0, log_std_max=2.0, central=central.data_ptr(), delta=delta.data_ptr(), eps=None,
                 action=act_out.data_ptr(), log_prob=lp.data_ptr(), mu=None, log_sigma=None, ctrl=None, out_flags=0, pad=0,
                 x2=s2.data_ptr(), d2=c.d2, stride1=s1.shape[1], stride2=s2.shape[1], n_rows=n, idx=None,
                 clip_lo=lo.data_ptr(), clip_hi=hi.data_ptr())
        f.update(kw)
        return _abi.SGAct(**f)

    bad_act = [dict(d2=D), dict(d2=D + 3), dict(d2=-1), dict(clip_lo=None), dict(clip_hi=None), dict(x2=None), dict(d2=0),
               dict(stride1=c.d1 - 1), dict(stride2=c.d2 - 1), dict(idx=idx.data_ptr(), n_rows=0)]
    for kw in bad_act:
        with pytest.raises(OlyError):
            eng.ctx.call("oly_sg_act", C.byref(act(**kw)), eng._s())
    # the engine's own checks
    with pytest.raises(OlyError, match="targets"):
        eng.bc_fit_steps(s1, targets, idx, cs, param, m, v, packed, ws, 0, 1e-3,
                         pair=dict(x2=s2, actions=actions, central=central, delta=delta, d1=c.d1, d2=c.d2))
    with pytest.raises(OlyError, match="pair"):
        eng.bc_fit_steps(s1, None, idx, cs, param, m, v, packed, ws, 0, 1e-3,
                         pair=dict(x2=s2, actions=actions, central=central, delta=delta, d1=c.d1, d2=99))
    torch.cuda.synchronize()
    for key, f in b.items():
        assert f.same_as(snap[key]), (key, "a refused call launches nothing")
    # the context is still usable: the same blocks, valid, run
    eng.ctx.call("oly_bc_fit_steps", C.byref(fit(pair())), ir.STEPS, eng._s())
    eng.ctx.call("oly_sg_act", C.byref(act()), eng._s())
    b.done("after the refusals", written=("action", "log_prob"), finite=("param", "colstats", "action", "log_prob"))
    assert b["out"].unwritten() == ir.STEPS, "three of the four columns of every step"


def test_an_index_outside_the_ring_is_clamped(eng):
    """The tables have exactly n_rows rows between NaN fences and NaN in the strides' padding, so a read past a row or a
    table shows in every sum; an index outside [0, n_rows) is clamped to its ends, not followed."""
    c = ir.CASES[1]
    k = dict(case(c))
    idx = k["idx"].copy()
    idx[0, 2], idx[1, 2] = -5, len(k["states"]) + 7
    want = idx.copy()
    want[0, 2], want[1, 2] = 0, len(k["states"]) - 1
    same_fit(run_fit(eng, c, dict(k, idx=idx), paired=True), run_fit(eng, c, dict(k, idx=want), paired=True))


# ------------------------------------------------------------------------------ the host layer: the model on a ring
def _model(eng, c, k, standardizer=True, **kw):
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iqfo import DeviceGaussianInvActionModel
    D = c.d1 + c.d2
    lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * c.A)]
    with torch.no_grad():
        for p, v in zip([t for lin in lins for t in (lin.weight, lin.bias)], k["params"]):
            p.copy_(torch.as_tensor(v))
    return DeviceGaussianInvActionModel(eng, lins, k["min_a"], k["max_a"], 1e-3, batch_size=c.batch,
                                        standardizer=DeviceStandardizer(eng, D) if standardizer else None,
                                        log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX, **kw)


def test_model_on_a_replay_ring_equals_the_composed_path(eng, tmp_path):
    """DeviceGaussianInvActionModel.fit and draw_action on (ring, sample_idx) against what today's entry points compose:
    torch gathers, cat, oly_bc_targets, oly_bc_fit_steps on the materialised table, oly_sg_act on materialised rows."""
    from olympic_hip.iq import DeviceReplayMemory
    c = ir.IAMCase(6, 6, 5, 7, 0, 0, True, 9)          # the fixtures' setting: in = 6 (row width 12), A = 5, batch 7
    k = ir.build(c)
    ring = DeviceReplayMemory(eng, 5, ir.RING, c.d1, c.A)
    ring.add(dict(states=k["states"], actions=k["actions"], next_states=k["next_states"], absorbing=np.zeros(ir.RING)))
    g1, g2 = torch.Generator(device="cuda").manual_seed(3), torch.Generator(device="cuda").manual_seed(3)
    idx = torch.stack([ring.sample_idx(c.batch, g1) for _ in range(2)])
    assert idx.dtype == I32 and idx.shape == (2, c.batch)
    same = [ring.get(c.batch, g2) for _ in range(2)]
    S, NS, ACT = ring.blocks["states"], ring.blocks["next_states"], ring.blocks["actions"]
    assert torch.equal(same[1][0], S[idx[1].long()]), "sample_idx draws what get draws"
    model, twin = _model(eng, c, k), _model(eng, c, k)
    out = model.fit(S, NS, ACT, idx)
    table = torch.cat([S, NS], dim=1)
    targets = eng.bc_targets(ACT, twin.central, twin.delta)
    ref = eng.bc_fit_steps(table, targets, idx, twin._colstats(), twin.param, twin.exp_avg, twin.exp_avg_sq, twin.packed,
                           eng.bc_fit_ws(c.batch, 12, c.A), 0, 1e-3, log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX)
    for a, b in ((out, ref), (model.param, twin.param), (model.exp_avg, twin.exp_avg), (model.exp_avg_sq, twin.exp_avg_sq),
                 (model.packed, twin.packed), (model.stand.colstats, twin.stand.colstats)):
        assert torch.equal(a, b)
    assert model.step == 2 and float(model.stand.colstats[0, 0]) == 2 * c.batch
    # the expert draw: rows of a demonstration table, LSIQfO's clip against the float64 action space
    eps = d(k["eps"][:9])
    rows = d(np.array([39, 0, 5, 5, 17, 1, 2, 3, 39], np.int32))
    lo, hi = k["min_a"] * 0.25, k["max_a"] * 0.25
    drawn = model.draw_action(S, NS, idx=rows, eps=eps, clip=(lo, hi))
    o = eng.sg_act(table[rows.long()], twin.packed, twin.central, twin.delta, colstats=twin.stand.colstats, eps=eps, want=())
    want = np.minimum(np.maximum(o["action"].cpu().numpy().astype(np.float64), lo), hi).astype(np.float32)
    assert np.array_equal(drawn.cpu().numpy(), want) and (want != o["action"].cpu().numpy()).any()
    assert torch.equal(model.stand.colstats, twin.stand.colstats), "the expert draw feeds the Standardizer"
    # get_mu_log_sigma, entropy and use_mean feed it too and read the same network
    mu, ls = model.get_mu_log_sigma(S, NS, idx=rows)
    o = eng.sg_act(table[rows.long()], twin.packed, twin.central, twin.delta, colstats=twin.stand.colstats, eps=None,
                   want=("mu", "log_sigma"))
    assert torch.equal(mu, o["mu"]) and torch.equal(ls, o["log_sigma"])
    ent = model.entropy(S, NS, idx=rows)               # a forward of its own: the rows go into the statistics once more
    o = eng.sg_act(table[rows.long()], twin.packed, twin.central, twin.delta, colstats=twin.stand.colstats, eps=None,
                   want=("log_sigma",))
    assert float(model.stand.colstats[0, 0]) == 2 * c.batch + 27 and torch.equal(model.stand.colstats, twin.stand.colstats)
    assert abs(float(ent) - (0.5 + 0.5 * np.log(2 * np.pi) + float(o["log_sigma"].double().mean()))) <= 1e-6
    model.use_mean = True
    before = model.stand.colstats.clone()
    mean = model.draw_action(S, NS, idx=rows)
    o = eng.sg_act(table[rows.long()], model.packed, model.central, model.delta, colstats=before, eps=None, want=("mu",))
    assert torch.equal(mean, o["action"]) and torch.equal(before, model.stand.colstats)
    squashed = torch.tanh(o["mu"].double()) * model.delta.double() + model.central.double()
    assert float((mean.double() - squashed).abs().max()) <= TOL
    # a checkpoint: the state goes into a fresh model in place and the next fit has the same bits
    fresh = _model(eng, c, k)
    ptrs = (fresh.param.data_ptr(), fresh.packed.data_ptr(), fresh.stand.colstats.data_ptr())
    model.save(str(tmp_path / "action_model.pt"), iteration=2)          # through il_checkpoint's file
    assert fresh.load(str(tmp_path / "action_model.pt"))["iteration"] == 2
    assert ptrs == (fresh.param.data_ptr(), fresh.packed.data_ptr(), fresh.stand.colstats.data_ptr()) and fresh.use_mean
    a, b = model.fit(S, NS, ACT, idx), fresh.fit(S, NS, ACT, idx)
    assert torch.equal(a, b) and torch.equal(model.param, fresh.param) and torch.equal(model.exp_avg_sq, fresh.exp_avg_sq)
    assert torch.equal(model.stand.colstats, fresh.stand.colstats) and fresh.step == 4


def test_model_refusals(eng):
    from olympic_hip._ffi import OlyError
    c = ir.CASES[1]
    k = case(c)
    m = _model(eng, c, k)
    S, NS, ACT = d(k["states"]), d(k["next_states"]), d(k["actions"])
    with pytest.raises(OlyError, match="columns"):
        m.fit(S, NS, ACT, d(k["idx"]))                       # the tables' full widths do not add up to the network's
    with pytest.raises(OlyError, match="idx"):
        m.fit(S, NS, ACT, d(k["idx"])[:, :3].contiguous(), d1=c.d1, d2=c.d2)
    with pytest.raises(OlyError):
        _model(eng, c, k, nll_eps=0.0)
    with pytest.raises(OlyError, match="batch_size 4097 > 4096"):            # the limit is named at construction, as
        _model(eng, c._replace(batch=4097), k)                               # DeviceBehavioralCloning names it
    out = m.fit(S, NS, ACT, d(k["idx"]), d1=c.d1, d2=c.d2)   # the wide tables with their widths named
    assert out.shape == (ir.STEPS, 3) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------ the whole agents
# The issue's setting: in = 6 (row width 12), A = 5, batch 9, action-model batch 7, fits_per_step = 2, Standardizers on all
# networks, four iterations, every one logging.
AG_IN, AG_A, AG_B, AG_AMB, AG_FITS, AG_ITERS = 6, 5, 9, 7, 2, 4
AG_LO, AG_HI = -np.array([0.6, 0.9, 0.5, 0.8, 0.7]), np.array([0.7, 0.5, 0.9, 0.6, 0.8])


def _transitions(n, seed, actions=True):
    rng = np.random.default_rng(seed)
    out = dict(states=rng.standard_normal((n, AG_IN)).astype(np.float32) * 2 + 1,
               next_states=rng.standard_normal((n, AG_IN)).astype(np.float32) * 2 + 1,
               absorbing=(rng.uniform(0, 1, n) < 0.1).astype(np.float32))
    if actions:       # raw actions: some beyond the bounds
        out["actions"] = (1.2 * np.tanh(rng.standard_normal((n, AG_A))) * AG_HI).astype(np.float32)
    return out


def _agent(eng, kind, fo, demo, **extra):
    """A whole agent of `kind` ("iq", "lsiq", "lsiq_h", "lsiq_hc") on fresh, identically initialised networks; fo: the
    from-observations class with its action model, else the base class and a model beside it.  Returns (agent, model)."""
    from olympic_hip import iq, iqfo
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    D, A = AG_IN, AG_A
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        lin = torch.nn.Linear
        p, c, h, a = ([lin(i, 512), lin(512, 256), lin(256, o)] for i, o in ((D, 2 * A), (D + A, 1), (D + A, 1), (2 * D, 2 * A)))
    policy = DeviceSquashedGaussianPolicy(eng, p, AG_LO, AG_HI, standardizer=DeviceStandardizer(eng, D))
    critic = iq.DeviceSoftQCritic(eng, c, standardizer=DeviceStandardizer(eng, D + A), lr=3e-4, tau=0.005)
    model = iqfo.DeviceGaussianInvActionModel(eng, a, AG_LO, AG_HI, 1e-3, batch_size=AG_AMB,
                                              standardizer=DeviceStandardizer(eng, 2 * D))
    kw = dict(gamma=0.99, batch_size=AG_B, use_target=True, logging_iter=1, initial_replay_size=10, max_replay_size=64,
              actor_optimizer=dict(lr=3e-4), init_alpha=0.1)
    if kind.startswith("lsiq"):
        kw.update(Q_exp_loss="MSE")
    if kind in ("lsiq_h", "lsiq_hc"):
        kw["h_critic"] = iq.DeviceSoftQCritic(eng, h, standardizer=DeviceStandardizer(eng, D + A), lr=3e-4, tau=0.005)
    if kind == "lsiq_hc":
        kw.update(H_tau=0.005)
    if fo:
        kw.update(action_model=model, action_model_fit_params=dict(fits_per_step=AG_FITS, init_epochs=0))
    kw.update(extra)
    if fo:
        cls = dict(iq=iqfo.DeviceIQfOSAC, lsiq=iqfo.DeviceLSIQfOSAC, lsiq_h=iqfo.DeviceLSIQfOHSAC, lsiq_hc=iqfo.DeviceLSIQfOHCSAC)
        return cls[kind](eng, policy, critic, demo, **kw), model
    cls = dict(iq=iq.DeviceIQSAC, lsiq=iq.DeviceLSIQSAC, lsiq_h=iq.DeviceLSIQHSAC, lsiq_hc=iq.DeviceLSIQHCSAC)
    return cls[kind](eng, policy, critic, dict(demo, actions=np.zeros((len(demo["states"]), A), np.float32)), **kw), model


def _agent_tensors(agent, model):
    out = dict(policy=agent.policy.param, policy_stats=agent.policy.stand.colstats, critic=agent.critic.param,
               critic_target=agent.critic.target_param, critic_stats=agent.critic.stand.colstats, model=model.param,
               model_m=model.exp_avg, model_v=model.exp_avg_sq, model_stats=model.stand.colstats, pi_m=agent.pi_exp_avg)
    if getattr(agent, "h_critic", None) is not None:
        out["h"] = agent.h_critic.param
    return out


def _by_hand(eng, agent, model, demo_actions, dataset, g, clip):
    """One IQfO_SAC.fit (iqfo_sac.py:59-120 with train_action_model :174-264, every iteration logging) written out on
    the base agent with today's unpaired entry points: torch gathers, cat, oly_bc_targets, oly_bc_fit_steps and oly_sg_act
    on materialised rows, np.clip's formula in torch float64.  Returns the logged scalars."""
    ring, d = agent.replay, agent.demo
    ring.add(dataset)
    if not ring.initialized:
        agent._iter += 1
        agent.policy.iter = getattr(agent.policy, "iter", 0) + 1
        return None
    S, NS, ACT = ring.blocks["states"], ring.blocks["next_states"], ring.blocks["actions"]
    own = torch.arange(AG_AMB, device="cuda", dtype=I32).reshape(1, AG_AMB)
    ws = eng.bc_fit_ws(AG_AMB, 2 * AG_IN, AG_A)

    def rows_of(s_tbl, ns_tbl, i):
        return torch.cat([s_tbl[i.long()], ns_tbl[i.long()]], dim=1)

    def act(s_tbl, ns_tbl, i, noise, want=()):
        return eng.sg_act(rows_of(s_tbl, ns_tbl, i), model.packed, model.central, model.delta, colstats=model._colstats(),
                          eps=noise, log_std_min=model.log_std_min, log_std_max=model.log_std_max, want=want)

    def randn(n):
        return torch.randn((n, AG_A), dtype=F32, device="cuda", generator=g)
    idx = torch.stack([ring.sample_idx(AG_AMB, g) for _ in range(AG_FITS)])
    for i in idx:
        eng.bc_fit_steps(rows_of(S, NS, i), eng.bc_targets(ACT[i.long()], model.central, model.delta), own, model._colstats(),
                         model.param, model.exp_avg, model.exp_avg_sq, model.packed, ws, model.step, model.lr,
                         log_std_min=model.log_std_min, log_std_max=model.log_std_max)
        model.stand._fresh = False
        model.step += 1
    ip, ie = ring.sample_idx(AG_AMB, g), agent.draw_demo_idx(AG_AMB, g)
    log = {}
    log["Action-Model/Loss Policy"] = torch.mean((act(S, NS, ip, randn(AG_AMB))["action"] - ACT[ip.long()]) ** 2)
    pred = act(d["states"], d["next_states"], ie, randn(AG_AMB))["action"]
    log["Action-Model/Loss Exp"] = torch.mean((pred - demo_actions[ie]) ** 2)
    half = 0.5 + 0.5 * float(np.log(2 * np.pi))
    log["Action-Model/Entropy Plcy"] = half + act(S, NS, ip, None, ("log_sigma",))["log_sigma"].mean()
    log["Action-Model/Entropy Exp"] = half + act(d["states"], d["next_states"], ie, None, ("log_sigma",))["log_sigma"].mean()
    last = act(S, NS, idx[-1], None, ("mu", "log_sigma"))
    exp = act(d["states"], d["next_states"], ie, None, ("mu", "log_sigma"))
    log["Action-Model/Std Exp"], log["Action-Model/Std"] = exp["log_sigma"].exp().mean(), last["log_sigma"].exp().mean()
    log["Action-Model/Mu Exp"], log["Action-Model/Mu"] = exp["mu"].mean(), last["mu"].mean()
    ip = ring.sample_idx(AG_B, g).long()
    ie = agent.draw_demo_idx(AG_B, g)
    demo_act = act(d["states"], d["next_states"], ie, randn(AG_B))["action"]
    if clip:
        lo, hi = torch.as_tensor(AG_LO).cuda(), torch.as_tensor(AG_HI).cuda()
        demo_act = torch.minimum(torch.maximum(demo_act.double(), lo), hi).float()
    agent.iq_update(torch.cat([S[ip], d["states"][ie]]), torch.cat([ACT[ip], demo_act]), torch.cat([NS[ip], d["next_states"][ie]]),
                    torch.cat([ring.blocks["absorbing"][ip], d["absorbing"][ie]]), AG_B, generator=g)
    agent._iter += 1
    agent.policy.iter = getattr(agent.policy, "iter", 0) + 1
    return log


@pytest.mark.parametrize("kind", ("iq", "lsiq"))
def test_agent_fit_is_the_reference_sequence_written_out(eng, kind):
    """DeviceIQfOSAC / DeviceLSIQfOSAC.fit for four logging iterations against the same sequence written out from
    iqfo_sac.py / lsiqfo.py on the base agent and the unpaired entry points: all networks, moments, statistics and logged
    scalars bit for bit, and the rows the action model's Standardizer has seen."""
    demo = _transitions(30, 1)
    agent, model = _agent(eng, kind, True, demo)
    base, twin = _agent(eng, kind, False, demo)
    from olympic_hip.iqfo import AM_LOG_TAGS
    demo_actions = d(demo["actions"])
    g1, g2 = torch.Generator(device="cuda").manual_seed(8), torch.Generator(device="cuda").manual_seed(8)
    assert type(agent).CLIP_DRAW == (kind == "lsiq")
    seen = 0
    for it in range(AG_ITERS):
        data = _transitions(8 if it == 0 else 12, 50 + it)          # the first dataset leaves the memory uninitialised
        out = agent.fit(data, generator=g1)
        log = _by_hand(eng, base, twin, demo_actions, data, g2, clip=kind == "lsiq")
        assert (out is None) == (it == 0) == (log is None)
        if it:
            seen += AG_FITS * AG_AMB + 6 * AG_AMB + AG_B         # the fits, the six logging passes, the expert draw
            assert tuple(agent.am_log) == AM_LOG_TAGS and set(log) == set(AM_LOG_TAGS)
            for key in log:
                assert torch.equal(agent.am_log[key], log[key].to(agent.am_log[key].dtype)), (it, key)
        assert float(model.stand.colstats[0, 0]) == seen, "every pass feeds the action model's Standardizer"
        for (key, a), b in zip(_agent_tensors(agent, model).items(), _agent_tensors(base, twin).values()):
            assert torch.equal(a, b), (it, key)
    assert agent._iter == base._iter == 1 + AG_ITERS and agent.critic.step == 3 and model.step == 3 * AG_FITS


def test_agent_without_demonstration_actions_and_with_interpolation(eng):
    demo = _transitions(30, 1, actions=False)
    agent, model = _agent(eng, "iq", True, demo, interpolate_expert_states=True, interpolation_coef=0.7)
    g = torch.Generator(device="cuda").manual_seed(2)
    for it in range(3):
        out = agent.fit(_transitions(12, 60 + it), generator=g)
    assert "Action-Model/Loss Exp" not in agent.am_log and len(agent.am_log) == 7
    assert float(model.stand.colstats[0, 0]) == 3 * (AG_FITS * AG_AMB + 5 * AG_AMB + AG_B)
    assert all(bool(torch.isfinite(t).all()) for t in _agent_tensors(agent, model).values()) and out[0] is not None


@pytest.mark.parametrize("kind", ("lsiq_h", "lsiq_hc"))
def test_h_agents_fit_and_do_not_clip(eng, kind):
    agent, model = _agent(eng, kind, True, _transitions(30, 1))
    assert not type(agent).CLIP_DRAW
    g = torch.Generator(device="cuda").manual_seed(2)
    for it in range(3):
        agent.fit(_transitions(12, 70 + it), generator=g)
    assert all(bool(torch.isfinite(t).all()) for t in _agent_tensors(agent, model).values())
    assert agent.h_critic.step > 0 and model.step == 3 * AG_FITS


def test_agent_checkpoint_resumes_bit_for_bit(eng, tmp_path):
    """DeviceIQfOSAC saved after iteration 2 of 4 and resumed in fresh objects ends equal to the uninterrupted run."""
    from olympic_hip import il_checkpoint
    demo = _transitions(30, 1)
    data = [_transitions(12, 80 + it) for it in range(4)]
    whole, m_whole = _agent(eng, "iq", True, demo)
    g = torch.Generator(device="cuda").manual_seed(4)
    for it in range(4):
        whole.fit(data[it], generator=g)
    first, m_first = _agent(eng, "iq", True, demo)
    g = torch.Generator(device="cuda").manual_seed(4)
    for it in range(2):
        first.fit(data[it], generator=g)
    il_checkpoint.save(str(tmp_path / "iqfo.pt"), first, None, generator=g.get_state())
    resumed, m_res = _agent(eng, "iq", True, demo)
    meta = il_checkpoint.load(str(tmp_path / "iqfo.pt"), resumed, None)
    g2 = torch.Generator(device="cuda")
    g2.set_state(meta["generator"])
    for it in range(2, 4):
        resumed.fit(data[it], generator=g2)
    for (key, a), b in zip(_agent_tensors(whole, m_whole).items(), _agent_tensors(resumed, m_res).values()):
        assert torch.equal(a, b), key
    assert resumed._iter == whole._iter and m_res.step == m_whole.step
    for key in whole.am_log:
        assert torch.equal(whole.am_log[key], resumed.am_log[key]), key


def test_agent_refusals_name_what_they_refuse(eng):
    from olympic_hip._ffi import OlyError
    demo = _transitions(30, 1)
    for extra, why in ((dict(add_noise_to_obs=True), "add_noise_to_obs"),
                       (dict(ext_normalizer_action_model=object()), "ext_normalizer_action_model"),
                       (dict(interpolate_expert_states=True, state_mask=list(range(AG_IN))), "state_mask"),
                       (dict(action_model="KLGaussianInvActionModel"), "KL-Gaussian"), (dict(action_model="GCPActionModel"), "GCP"),
                       (dict(action_model="KLGCPActionModel"), "KL-GCP"),
                       (dict(action_model="LearnableVarGaussianInvActionModel"), "learnable-variance"),
                       (dict(action_model="FixedVarGaussianInvActionModel"), "fixed-variance"),
                       (dict(action_model=None), "DeviceGaussianInvActionModel"),
                       (dict(action_model_fit_params=dict(fits_per_step=1, epochs=3)), "action_model_fit_params")):
        with pytest.raises(OlyError, match=why):
            _agent(eng, "iq", True, demo, **extra)
    with pytest.raises(OlyError, match="states"):
        _agent(eng, "iq", True, {k: v for k, v in demo.items() if k != "states"})


# ------------------------------------------------------------------------------ the model against the reference run
@pytest.mark.parametrize("name", ("iqfo", "lsiqfo"))
def test_model_against_the_reference_run_fixture(eng, golden, name):
    """DeviceGaussianInvActionModel through the calls four logging iterations of IQfO_SAC.fit / LSIQfO.fit make on the
    action model, against tests/golden/iam_fit (the reference's own GaussianInvActionModel, executed): parameters,
    statistics, logged scalars and the drawn expert actions, within max(2e-5, 4 x the stored spread)."""
    import test_iam_cpu as cpu
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iqfo import DeviceGaussianInvActionModel
    g = golden(f"iam_fit/{name}.npz")
    A, D = ir.SEQ_A, 2 * ir.SEQ_IN
    lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * A)]
    with torch.no_grad():
        for p, v in zip([t for lin in lins for t in (lin.weight, lin.bias)], cpu.fixture_params(g)):
            p.copy_(torch.as_tensor(v))
    m = DeviceGaussianInvActionModel(eng, lins, g["min_a"], g["max_a"], ir.SEQ_LR, batch_size=ir.SEQ_AMB,
                                     standardizer=DeviceStandardizer(eng, D))
    assert (m.log_std_min, m.log_std_max) == (ir.SEQ_LO, ir.SEQ_HI), "the reference's defaults"
    S, NS, ACT, DS, DNS, DA = (d(g[k]) for k in ("ring_s", "ring_ns", "ring_a", "demo_s", "demo_ns", "demo_a"))
    i32 = lambda a: d(a.astype(np.int32))
    half = 0.5 + 0.5 * np.log(2 * np.pi)
    got = dict(params=[], colstats=[], scalars=[], drawn=[])
    for it in range(ir.SEQ_ITERS):
        out = m.fit(S, NS, ACT, i32(g["fit_idx"][it]))
        ip, ie = i32(g["ip"][it]), i32(g["ie"][it])
        row = [float(v) for v in out[:, 0]]
        row.append(float(((m.draw_action(S, NS, idx=ip, eps=d(g["eps_plcy"][it])) - ACT[ip.long()]).double() ** 2).mean()))
        row.append(float(((m.draw_action(DS, DNS, idx=ie, eps=d(g["eps_exp"][it])) - DA[ie.long()]).double() ** 2).mean()))
        row += [float(m.entropy(S, NS, idx=ip)), float(m.entropy(DS, DNS, idx=ie))]
        mu, ls = m.get_mu_log_sigma(S, NS, idx=i32(g["fit_idx"][it, -1]))
        mu_e, ls_e = m.get_mu_log_sigma(DS, DNS, idx=ie)
        row += [float(ls_e.exp().mean()), float(ls.exp().mean()), float(mu_e.mean()), float(mu.mean())]
        a = m.draw_action(DS, DNS, idx=i32(g["ie_draw"][it]), eps=d(g["eps_draw"][it]), clip=m.bounds if name == "lsiqfo" else None)
        got["drawn"].append(a.double().cpu().numpy())
        got["params"].append([t.double().cpu().numpy() for t in m._views()])
        got["colstats"].append(m.stand.colstats.cpu().numpy())
        got["scalars"].append(row)
    got = {k: (v if k == "params" else np.asarray(v)) for k, v in got.items()}
    miss = cpu.fixture_miss(g, got)
    print(name, miss)
    for group, v in miss.items():
        assert v <= cpu.tolerance(g, group), (group, v)
    assert np.abs(got["colstats"][:, 0] - g["colstats"][:, 0]).max() <= 1e-9      # stored as the reference's _count - 1e-2
    assert np.all(np.abs(got["colstats"] - g["colstats"]) <= 2e-5 * np.maximum(1, np.abs(g["colstats"])))


@pytest.mark.parametrize("c", (ir.CASES[1], ir.CASES[3]), ids=(IDS[1], IDS[3]))
def test_paired_statistics_over_several_blocks(eng, c):
    """5000 gathered rows: oly_col_stats splits them into several blocks' slabs (its scalar kernel at 17 columns, its
    four-column kernel at 64), and the paired launch must choose and add as it does."""
    k = case(c)
    one, _ = run_act(eng, c, k, 5000, True, True, eps=False)
    two, _ = run_act(eng, c, k, 5000, False, True, eps=False)
    for key in OUTS + ("colstats",):
        assert torch.equal(one[key].bytes, two[key].bytes), key
    assert float(one["colstats"].t[0, 0]) == 5000


# ------------------------------------------------------------------------------ the agents against the reference run
class _Writer:
    def __init__(self):
        self.rows = {}

    def add_scalar(self, name, val, it):
        self.rows.setdefault(int(it), {})[name] = float(val)


@pytest.mark.parametrize("name", ("iqfo", "lsiqfo"))
def test_agents_against_the_reference_run_fixtures(eng, golden, name):
    """DeviceIQfOSAC / DeviceLSIQfOSAC.fit for four logging iterations on the samples and noise of the reference's own
    IQfO_SAC.fit / LSIQfO.fit run (tests/golden/iam_fit): the action model, the policy, the critic and its target, all
    statistics and the logged scalars, within max(2e-5, 4 x the stored spread)."""
    import test_iam_cpu as cpu
    from olympic_hip import iq, iqfo
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.gail import DeviceStandardizer
    g = golden(f"iam_fit/{name}.npz")
    A, IN, F = ir.SEQ_A, ir.SEQ_IN, ir.FO

    def lins(dims, params):
        out = [torch.nn.Linear(i, o) for i, o in dims]
        with torch.no_grad():
            for p, v in zip([t for lin in out for t in (lin.weight, lin.bias)], params):
                p.copy_(torch.as_tensor(v))
        return out
    policy = DeviceSquashedGaussianPolicy(eng, lins([(IN, 512), (512, 256), (256, 2 * A)], cpu.agent_params(g, "policy")),
                                          g["min_a"], g["max_a"], standardizer=DeviceStandardizer(eng, IN),
                                          log_std_min=F["ls_min"], log_std_max=F["ls_max"])
    critic = iq.DeviceSoftQCritic(eng, lins([(IN + A, 512), (512, 256), (256, 1)], cpu.agent_params(g, "critic")),
                                  standardizer=DeviceStandardizer(eng, IN + A), lr=F["lr"], tau=F["tau"])
    model = iqfo.DeviceGaussianInvActionModel(eng, lins([(2 * IN, 512), (512, 256), (256, 2 * A)], cpu.fixture_params(g)),
                                              g["min_a"], g["max_a"], ir.SEQ_LR, batch_size=ir.SEQ_AMB,
                                              standardizer=DeviceStandardizer(eng, 2 * IN))
    sw = _Writer()
    kw = dict(gamma=F["gamma"], batch_size=ir.SEQ_B, use_target=True, init_alpha=F["init_alpha"], reg_mult=F["reg_mult"],
              logging_iter=1, sw=sw, max_replay_size=len(g["ring_s"]), actor_optimizer=dict(lr=F["lr_actor"]),
              action_model=model, action_model_fit_params=dict(fits_per_step=ir.SEQ_FITS, init_epochs=0))
    demo = dict(states=g["demo_s"], next_states=g["demo_ns"], absorbing=g["demo_abs"], actions=g["demo_a"])
    if name == "lsiqfo":
        agent = iqfo.DeviceLSIQfOSAC(eng, policy, critic, demo, Q_max=F["Q_max"], Q_min=F["Q_min"], loss_mode_exp="fix",
                                     Q_exp_loss="MSE", target_clipping=True, lossQ_type="iq_like", **kw)
    else:
        agent = iqfo.DeviceIQfOSAC(eng, policy, critic, demo, **kw)
    agent.replay.add(dict(states=g["ring_s"], actions=g["ring_a"], next_states=g["ring_ns"], absorbing=g["ring_abs"]))
    i32 = lambda a: d(a.astype(np.int32))
    got = dict(params=[], colstats=[], scalars=[], drawn=[])
    for it in range(ir.SEQ_ITERS):
        upd = dict(q=dict(next=d(g["eps_next"][it]), pi=d(g["eps_pi"][it]), expert=d(g["eps_expert"][it])),
                   pi=dict(pi=d(g["eps_ppi"][it]), log=d(g["eps_plog"][it])))
        samples = dict(fit_idx=i32(g["fit_idx"][it]), ip=i32(g["ip"][it]), ie=i32(g["ie"][it]), eps_plcy=d(g["eps_plcy"][it]),
                       eps_exp=d(g["eps_exp"][it]), idx_policy=i32(g["ip_fit"][it]), idx_demo=i32(g["ie_draw"][it]),
                       eps_draw=d(g["eps_draw"][it]), eps_update=upd)
        drawn = []
        draw0 = model.draw_action
        model.draw_action = lambda *a, **k: drawn.append(draw0(*a, **k)) or drawn[-1]      # the expert draw is the last
        try:
            out = agent.fit(dict(states=np.zeros((0, IN), np.float32)), samples=samples)
        finally:
            del model.draw_action
        assert out[0] is not None and out[1] is not None
        got["drawn"].append(drawn[-1].double().cpu().numpy())
        got["params"].append([t.double().cpu().numpy() for t in model._views()])
        got["colstats"].append(model.stand.colstats.cpu().numpy())
        got["scalars"].append([float(agent.am_log[t]) for t in iqfo.AM_LOG_TAGS])
    got = {k: (v if k == "params" else np.asarray(v)) for k, v in got.items()}
    miss = cpu.fixture_miss(g, got)
    pol = split(policy.param.double().cpu().numpy(), IN, A)

    def critic_split(flat):
        flat, out, o = flat.double().cpu().numpy(), [], 0
        for s in [(512, IN + A), (512,), (256, 512), (256,), (1, 256), (1,)]:
            n = int(np.prod(s))
            out.append(flat[o:o + n].reshape(s))
            o += n
        return out
    miss.update(cpu.agent_miss(g, dict(policy=pol, critic=critic_split(critic.param), target=critic_split(critic.target_param)),
                               sw.rows))
    print(name, miss)
    for group, v in miss.items():
        assert v <= cpu.tolerance(g, group), (group, v)
    for key, st in (("colstats", model.stand), ("policy_colstats", policy.stand), ("critic_colstats", critic.stand),
                    ("target_colstats", critic.target_stand)):
        a, want = st.colstats.cpu().numpy(), g[key][-1] if key == "colstats" else g[key]
        assert np.abs(a[0] - want[0]).max() <= 1e-9, key
        assert np.all(np.abs(a - want) <= 2e-5 * np.maximum(1, np.abs(want))), key
    assert agent._iter == 1 + ir.SEQ_ITERS and agent.pi_step == critic.step == ir.SEQ_ITERS
