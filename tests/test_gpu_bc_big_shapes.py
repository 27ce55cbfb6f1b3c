"""K24 and its paired path (K28's launch B, K24's paired prologue and rows kernel, K25 over the pair) at large batches on the
MI355X: oly_bc_fit_steps and oly_bc_fit_steps_log, with and without oly_bc_fit.pair, at the shapes and seeds of
tests/bc_big_shapes.py (257 to 4096 rows, two steps each) against the float64 restatements the small tables use, every operand
fenced (tests/fences.py, through tests/test_gpu_iam.py's helpers) and the workspace of exactly the reported size; the paired
call bit for bit against the materialised one, a second run and the cut (1, 1); an index outside the ring and the refusal of
4097 rows at the limit; the two host classes at 4096 rows against the engine calls.

The rule is bc_big_shapes.fit_errors: per tensor |kernel - f64| <= max(TOL, 4 |f32 - f64|) with TOL = 2e-5, the moments
relative to their largest entry, the count exact, the sums within TOL of their size, the scalars TOL relative from 1 upwards or
4 x the float32 run's spread.  tests/test_bc_big_shapes_cpu.py holds the float32 run of every case within TOL / 4 and shows
that a misread index position, scalars of the first 256 rows and statistics of one row per chain each miss this rule ten times
over.  Every test prints error, tolerance and their ratio before it asserts."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import bc_big_shapes as S
import bc_restate as br
import iam_restate as ir
from fences import Bufs
from test_gpu_bc_fit import make_trainer, trainer_state
from test_gpu_iam import KEYS, _model, d, fit_state, run_fit, same_fit, split

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BC = range(len(S.BC_SHAPES))
IAM = range(len(S.IAM_SHAPES))
BC_IDS = ["-".join(str(int(v)) for v in s) for s in S.BC_SHAPES]
IAM_IDS = ["-".join(str(int(v)) for v in s) + f"-ring{n}" for s, n in zip(S.IAM_SHAPES, S.RINGS)]


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    e = Engine(0)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def report(who, errs):
    for name, e, t in errs:
        print(f"{who} {name}: |kernel - f64| {e:.3e}, tolerance {t:.3e}, ratio {e / t:.3f}")
    groups = {}
    for name, e, t in errs:
        key = "params" if name in S.NAMES else name.split()[0]
        groups[key] = max(groups.get(key, 0.0), e / t)
    print(f"RATIOS {who}: " + ", ".join(f"{k} {v:.3f}" for k, v in groups.items()))
    bad = [(n, e, t) for n, e, t in errs if not e <= t]
    assert not bad, (who, bad)


def got_of(b, in_dim, A):
    """bc_big_shapes.fit_errors' `got` from the fenced buffers of a run."""
    h64 = lambda key: [t.double().cpu().numpy() for t in split(b[key].t, in_dim, A)]
    return dict(params=h64("param"), m=h64("m"), v=h64("v"), colstats=b["colstats"].t.cpu().numpy() if "colstats" in b else None,
                out=b["out"].t.cpu().numpy())


def check_run(eng, b, run, logged=False, fourth=True):
    """The fenced buffers of a run against its float64 yardstick; the packed stream is ilmlp_pack of the parameters."""
    bc = run["bc"]
    who = ("logged " if logged else "") + run["kind"] + " " + run["who"]
    report(who, S.fit_errors(got_of(b, bc.in_dim, bc.A), S.yardstick(run, logged), fourth=fourth))
    assert b["out"].unwritten() == 0, (who, "every scalar of both steps is stored")
    assert torch.equal(b["packed"].t, eng.ilmlp_pack(*split(b["param"].t, bc.in_dim, bc.A))), who
    if bc.standardizer:
        assert float(b["colstats"].t[0, 0]) == (4 if logged else 2) * bc.batch, who


def run_bc(eng, run, logged=False):
    """The unpaired fit of a run of bc_big_shapes.unpaired, both steps in one call, in test_gpu_iam.run_fit's fenced state:
    every operand fenced, out poisoned, ws of exactly the floats the entry point asks for.  Returns the buffers, checked."""
    c, k = run["c"], run["k"]
    assert k["batch"] == c.batch
    b = Bufs()
    fit_state(eng, ir.IAMCase(c.in_dim, 0, c.A, c.batch, 0, 0, c.standardizer, c.seed), k, b, S.UPDATES, 4 if logged else 3)
    idx = b.inp("idx", k["idx"])
    states, targets = b.inp("states", k["states"], gathered=True), b.inp("targets", k["targets"], gathered=True)
    st = {key: b[key].t if key in b else None for key in KEYS}
    kw = dict(log_std_min=br.LOG_STD_MIN, log_std_max=br.LOG_STD_MAX, nll_eps=br.NLL_EPS, out=st["out"])
    args = (states, targets, idx, st["colstats"], st["param"], st["m"], st["v"], st["packed"], b["ws"].t, 0, c.lr)
    if logged:
        eng.bc_fit_steps_log(*args, 1, 0, b.inp("noise", S.noise_of(c)), **kw)
    else:
        eng.bc_fit_steps(*args, **kw)
    keys = [key for key in KEYS if key in b]
    b.done(run["who"] + (" logged" if logged else ""), written=keys, finite=keys)
    return b


def run_iam(eng, run, paired, cuts=None, logged=False, k=None):
    """test_gpu_iam.run_fit on a run of bc_big_shapes.paired: both steps, logging_iter = 1 when logged."""
    return run_fit(eng, run["c"], run["k"] if k is None else k, paired, cuts=cuts, n_steps=S.UPDATES,
                   log=(1, S.noise_of(run["bc"])) if logged else None)


# ------------------------------------------------------------------------------ the unpaired fit against float64
@pytest.mark.parametrize("i", BC, ids=BC_IDS)
def test_unpaired_fit_against_float64(eng, i):
    run = S.unpaired(i)
    check_run(eng, run_bc(eng, run), run)


# ------------------------------------------------------------------------------ the paired fit: float64 and bits
@pytest.mark.parametrize("i", IAM, ids=IAM_IDS)
def test_paired_fit_against_float64_and_the_materialised_call(eng, i):
    """One paired call against float64 (iam_restate.fit_twin); against the call on the table torch gathers with
    oly_bc_targets' targets, a second paired run and the cut (1, 1), bit for bit on param, m, v, packed, colstats and out."""
    run = S.paired(i)
    one = run_iam(eng, run, True)
    check_run(eng, one, run)
    same_fit(one, run_iam(eng, run, False))
    same_fit(one, run_iam(eng, run, True))
    same_fit(one, run_iam(eng, run, True, cuts=(1, 1)))


# ------------------------------------------------------------------------------ the logged fit, both steps logging
@pytest.mark.parametrize("i", S.BC_LOGGED, ids=[BC_IDS[i] for i in S.BC_LOGGED])
def test_unpaired_logged_fit_against_float64(eng, i):
    """All four scalars and the doubled statistics.  On the saturated case the float32 log-probability is no function of its
    float64 value (bc_log_restate, bc_big_shapes.bc_twin): there the sampled entropy is asked to be finite and is held on
    the unsaturated twin, which runs here too."""
    run = S.unpaired(i)
    saturated = run["c"].saturated
    check_run(eng, run_bc(eng, run, logged=True), run, logged=True, fourth=not saturated)
    if saturated:
        twin = S.unpaired(i, twin=True)
        assert not twin["c"].saturated and twin["c"][:6] == run["c"][:6]
        check_run(eng, run_bc(eng, twin, logged=True), twin, logged=True)


@pytest.mark.parametrize("i", S.IAM_LOGGED, ids=[IAM_IDS[i] for i in S.IAM_LOGGED])
def test_paired_logged_fit_against_float64_and_the_materialised_call(eng, i):
    run = S.paired(i)
    one = run_iam(eng, run, True, logged=True)
    check_run(eng, one, run, logged=True)
    same_fit(one, run_iam(eng, run, False, logged=True))


# ------------------------------------------------------------------------------ an index outside the ring
def test_an_index_outside_the_ring_is_clamped_at_the_limit(eng):
    """(32, 32, 16, 4096) with strides wider than the widths: positions in the last tile of step 1 hold -5 and n_rows + 7.
    The tables lie between NaN fences with NaN in the strides' padding, so a read outside a row or a table shows in every
    sum (run_fit asks every result to be free of NaN); the result has the bits of the clamped indices."""
    run = S.paired(3)
    c, k, n = run["c"], run["k"], S.RINGS[3]
    assert c[:6] == (32, 32, 16, S.MAX_BATCH, 4, 9) and k["idx"].shape == (S.UPDATES, S.MAX_BATCH)
    idx = k["idx"].copy()
    last = S.MAX_BATCH - S.TILE
    idx[1, last + 2], idx[1, last + 7], idx[1, -1] = -5, n + 7, n + 7
    want = idx.copy()
    want[1, last + 2], want[1, last + 7], want[1, -1] = 0, n - 1, n - 1
    got = run_iam(eng, run, True, k=dict(k, idx=idx))
    same_fit(got, run_iam(eng, run, True, k=dict(k, idx=want)))
    assert not torch.equal(got["param"].bytes, run_iam(eng, run, True)["param"].bytes), "the three positions reach the fit"


# ------------------------------------------------------------------------------ the limit is a limit
def test_4097_rows_are_refused_and_nothing_is_written(eng):
    from olympic_hip import _abi
    from olympic_hip._ffi import OlyError, lib
    run = S.paired(0)
    c, k = run["c"], run["k"]
    D, A, n, batch = c.d1 + c.d2, c.A, S.RINGS[0], S.MAX_BATCH + 1
    b = Bufs()
    flat = br.flat(k["params"]).astype(np.float32)
    param, m, v = b.inp("param", flat), b.inp("m", np.zeros_like(flat)), b.inp("v", np.zeros_like(flat))
    packed = b.inp("packed", eng.ilmlp_pack(*split(d(flat), D, A)))
    cs = b.inp("colstats", np.zeros((3, D)))
    idx = b.inp("idx", np.resize(k["idx"].reshape(-1), (S.UPDATES, batch)).astype(np.int32))
    s1, s2 = b.inp("states", k["states"], gathered=True), b.inp("next_states", k["next_states"], gathered=True)
    table = b.inp("table", k["table"], gathered=True)
    actions, targets = b.inp("actions", k["actions"], gathered=True), b.inp("targets", k["targets"], gathered=True)
    central, delta = b.inp("central", k["central"]), b.inp("delta", k["delta"])
    noise = b.inp("noise", np.zeros((S.UPDATES, batch, A), np.float32))
    assert int(lib().oly_bc_fit_ws(batch, D, A)) == -1 and int(lib().oly_bc_fit_log_ws(batch, D, A)) == -1
    nws = int(lib().oly_bc_fit_log_ws(S.MAX_BATCH, D, A)) + 16
    ws, out = b.out("ws", (nws,), F32), b.out("out", (S.UPDATES, 4), F64)
    snap = {key: f.snapshot() for key, f in b.items()}
    pr = _abi.BCPair(d1=c.d1, d2=c.d2, stride1=s1.shape[1], stride2=s2.shape[1], x2=s2.data_ptr(), actions=actions.data_ptr(),
                     central=central.data_ptr(), delta=delta.data_ptr())

    def fit(paired, rows):
        return _abi.BCFit(in_dim=D, act_dim=A, batch=rows, n_rows=n, step=0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                          weight_decay=0.0, log_std_min=-20.0, log_std_max=2.0, nll_eps=1e-6,
                          states=(s1 if paired else table).data_ptr(), targets=None if paired else targets.data_ptr(),
                          idx=idx.data_ptr(), colstats=cs.data_ptr(), param=param.data_ptr(), m=m.data_ptr(), v=v.data_ptr(),
                          packed=packed.data_ptr(), ws=ws.data_ptr(), ws_floats=nws, out=out.data_ptr(),
                          pair=C.pointer(pr) if paired else None)

    for paired in (False, True):
        f = fit(paired, batch)
        with pytest.raises(OlyError, match="batch"):
            eng.ctx.call("oly_bc_fit_steps", C.byref(f), S.UPDATES, eng._s())
        with pytest.raises(OlyError, match="batch"):
            eng.ctx.call("oly_bc_fit_steps_log", C.byref(_abi.BCFitLog(fit=f, logging_iter=1, iter0=0, eps=noise.data_ptr())),
                         S.UPDATES, eng._s())
    torch.cuda.synchronize()
    for key, f in b.items():
        assert f.same_as(snap[key]), (key, "a refused call launches nothing")
    # one row fewer is accepted, on the same blocks (idx read with the pitch of 4096)
    for paired in (False, True):
        eng.ctx.call("oly_bc_fit_steps", C.byref(fit(paired, S.MAX_BATCH)), 1, eng._s())
    b.done("4096 rows after the refusals", finite=("param", "m", "v", "packed", "colstats"))
    assert float(cs[0, 0]) == 2 * S.MAX_BATCH and b["out"].unwritten() == 2 * 4 - 3


# ------------------------------------------------------------------------------ the host layer at 4096 rows
def test_action_model_on_a_ring_of_5000_rows_equals_the_engine_calls(eng):
    """DeviceGaussianInvActionModel(batch_size=4096).fit on a DeviceReplayMemory of 5000 rows with sample_idx against
    oly_bc_targets and oly_bc_fit_steps on the table torch concatenates, bit for bit."""
    from olympic_hip.iq import DeviceReplayMemory
    c = ir.IAMCase(32, 32, 16, S.MAX_BATCH, 0, 0, True, S.IAM_SEEDS[3])
    k = ir.build(c, n_rows=5000, steps=S.UPDATES)
    ring = DeviceReplayMemory(eng, 5, 5000, c.d1, c.A)
    ring.add(dict(states=k["states"], actions=k["actions"], next_states=k["next_states"], absorbing=np.zeros(5000)))
    g = torch.Generator(device="cuda").manual_seed(3)
    idx = torch.stack([ring.sample_idx(c.batch, g) for _ in range(S.UPDATES)])
    assert idx.dtype == torch.int32 and idx.shape == (S.UPDATES, S.MAX_BATCH)
    assert int(idx.min()) >= 0 and 4000 < int(idx.max()) < 5000
    states, next_states, actions = ring.blocks["states"], ring.blocks["next_states"], ring.blocks["actions"]
    model, twin = _model(eng, c, k), _model(eng, c, k)
    out = model.fit(states, next_states, actions, idx)
    ref = eng.bc_fit_steps(torch.cat([states, next_states], dim=1), eng.bc_targets(actions, twin.central, twin.delta), idx,
                           twin._colstats(), twin.param, twin.exp_avg, twin.exp_avg_sq, twin.packed,
                           eng.bc_fit_ws(c.batch, c.d1 + c.d2, c.A), 0, 1e-3, log_std_min=br.LOG_STD_MIN,
                           log_std_max=br.LOG_STD_MAX)
    for a, r in ((out, ref), (model.param, twin.param), (model.exp_avg, twin.exp_avg), (model.exp_avg_sq, twin.exp_avg_sq),
                 (model.packed, twin.packed), (model.stand.colstats, twin.stand.colstats)):
        assert torch.equal(a, r)
    assert model.step == S.UPDATES and float(model.stand.colstats[0, 0]) == S.UPDATES * c.batch
    assert bool(torch.isfinite(out).all()) and not torch.equal(model.param, _model(eng, c, k).param)


def test_behavioral_cloning_at_4096_rows_equals_the_engine_call(eng):
    """One DeviceBehavioralCloning.fit_offline of two steps at (64, 16, 4096, 5000) against oly_bc_fit_steps on the trainer's
    own table and targets, bit for bit."""
    run = S.unpaired(3)
    c, k = run["c"], run["k"]
    assert (c.in_dim, c.A, c.batch, c.n_rows) == (64, 16, S.MAX_BATCH, 5000)
    demo = dict(states=k["states"], actions=k["actions"])
    tr, twin = make_trainer(eng, 31, demo, batch_size=c.batch), make_trainer(eng, 31, demo, batch_size=c.batch)
    assert tr.batch == S.MAX_BATCH and torch.equal(tr.policy.param, twin.policy.param)
    idx = d(k["idx"])
    out = tr.fit_offline(S.UPDATES, idx=idx)
    p = twin.policy
    ref = eng.bc_fit_steps(twin.states, twin.targets, idx, p._colstats(), p.param, twin.exp_avg, twin.exp_avg_sq, p.packed,
                           eng.bc_fit_ws(c.batch, c.in_dim, c.A), 0, 1e-3, log_std_min=p.log_std_min, log_std_max=p.log_std_max,
                           nll_eps=1e-6)
    assert torch.equal(out, ref) and bool(torch.isfinite(out).all()) and tr.step == S.UPDATES
    for a, r in zip(trainer_state(tr), trainer_state(twin)):
        assert torch.equal(a, r)
    assert float(p.stand.colstats[0, 0]) == S.UPDATES * c.batch
