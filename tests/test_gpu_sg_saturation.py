"""K25 (oly_sg_act) and K27 (oly_iq_pi_update, one critic and two) on the MI355X where the agents run them: the clamp
log_std in [-20, 2], a column clamped at sigma = exp(2), an unclamped one at sigma = 4.5, and |u| up to 30, where fp64 tanh
is exactly -+1 and only the 1e-6 guard is left of 1 - a^2 + 1e-6.  The tables, their seeds, the conditioning check that
accepts a case (the kernels' arithmetic on the CPU within TOL / 4 of float64) and the two wrong readings these cases tell
from the kernels are tests/sg_saturation.py's; tests/test_sg_saturation_cpu.py holds them without a GPU.  The older sweeps
(test_gpu_iq_pi.py, test_gpu_lsiq_h_actor.py, test_gpu_sg_act.py, iq_big_shapes.py) keep |u| < 4.

Tolerances: TOL = 2e-5 against float64 by test_gpu_iq_pi.py's rule (a parameter absolutely, m relative to its largest
entry, the scalars relative to max(1, |value|), the action absolutely, log_prob relative to max(1, |log_prob| max), the
statistics' counts exact), for K25 by test_gpu_sg_act.py's; everything the kernels' structure fixes is held bit for bit.
Every test prints its distances in units of TOL.

The lower clamp end stays out.  At log_sigma -> -20 the sample m + expf(ls) eps rounds to m in float32, d = a_raw - m is
0 or a few ulps of m against sigma = 2e-9, and the Gaussian term is quantisation noise in the reference's own float32 run
as in the kernels: holding d / sigma to 1e-5 needs log_sigma >~ -4.6.  test_gpu_sg_act.py's
test_log_sigma_past_both_clamp_bounds (finite, the clamp exact) is that end's test and stays as it is."""
import gc

import numpy as np
import pytest
import torch

import iq_pi_restate as P
import sg_saturation as S
from fences import Bufs
from test_gpu_iam import run_act
from test_gpu_iq_pi import Dev, split
from test_gpu_lsiq_h_actor import HPiDev
from test_gpu_sg_act import float64_of

pytestmark = pytest.mark.gpu
TOL = S.TOL
F32, F64 = torch.float32, torch.float64
ONE = [(k, j) for k in S.SAT_SHAPES for j in range(len(S.SAT_CONFIGS))]
TWO = [(k, j) for k in S.TWO_CRITICS for j in range(len(S.SAT_CONFIGS))]


def _engine(configure):
    from olympic_hip import specs
    from olympic_hip.engine import Engine
    e = Engine(0)
    if configure:
        e.il_configure(specs.unitree_h1("walk"))              # 11 actions: the controls of K25's second case
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine(False)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


@pytest.fixture(scope="module")
def eng_h1():
    e = _engine(True)
    yield e
    torch.cuda.synchronize()
    e.ctx.close()
    gc.collect()


def bounds_where_tanh_is_one(action, u64, central, delta):
    """Where |u| >= 19.1 in float64 (fp64 tanh is exactly -+1 there and the float32 sample is 1e-5 from u), the stored
    action has the bits of float32 central -+ delta.  Returns the number of such entries."""
    last = torch.as_tensor(np.abs(u64) >= S.EDGES[2], device="cuda")
    sign = torch.as_tensor(np.sign(u64), device="cuda").float()
    want = sign * delta[None, :] + central[None, :]
    assert torch.equal(action[last], want[last])
    return int(last.sum())


# ------------------------------------------------------------------------------ K27 against the float64 yardstick
def check_updates(eng, dev, k, j, two):
    in_dim, A, Bp = P.SHAPES[k]
    case, cfg, who = S.sat_inputs(k), S.SAT_CONFIGS[j], S.run_id(k, j, two)
    ref, ref_out, ref_acts, log = S.sat_yardstick(k, j, two)
    assert (cfg.ls_min, cfg.ls_max) == (-20.0, 2.0)
    outs, ratio = [], dict(action=0.0, log_prob=0.0)
    for s, (a_ref, lp_ref), e in zip(case["steps"], ref_acts, log):
        outs.append(dev.update(s).cpu().numpy())
        got = dev.snapshot()
        assert not S.facts_hold(S.facts_of(e["u"], e["raw"])), (who, "the float64 side's bands")
        ratio["action"] = max(ratio["action"], float(np.abs(got["action"].double().cpu().numpy() - a_ref).max()) / TOL)
        ratio["log_prob"] = max(ratio["log_prob"], float(np.abs(got["log_prob"].double().cpu().numpy() - lp_ref).max())
                                / max(1.0, np.abs(lp_ref).max()) / TOL)
        assert bounds_where_tanh_is_one(got["action"], e["u"], got["central"], got["delta"]) >= 4, who
    dev.check_fences(who)
    out = np.stack(outs)
    params = split(got["param"].double().cpu().numpy(), in_dim, 2 * A)
    for name, a, r in zip(P.NAMES, params, ref["policy"]["params"]):
        ratio[name] = float(np.abs(a - r).max()) / TOL
    r = P.cat(ref["policy"]["exp_avg"])
    ratio["m"] = float(np.abs(got["m"].double().cpu().numpy() - r).max()) / float(np.abs(r).max()) / TOL
    ratio["scalars"] = float((np.abs(out - ref_out) / np.maximum(1.0, np.abs(ref_out))).max()) / TOL
    stats = [("colstats", ref["policy"]["colstats"]), ("critic_colstats", ref["critic"]["colstats"])]
    if two:
        stats.append(("h_colstats", ref["h"]["colstats"]))
    if cfg.standardizer:
        for key, want in stats:
            a = got[key].cpu().numpy()
            assert np.array_equal(a[0], want[0]), (who, key, "counts")
            ratio[key] = float((np.abs(a - want) / np.maximum(1.0, np.abs(want))).max()) / TOL
    print(f"{who}: |kernel - f64| / TOL " + ", ".join(f"{key} {v:.4f}" for key, v in ratio.items()))
    assert np.isfinite(out).all() and all(bool(torch.isfinite(got[key]).all()) for key in ("param", "m", "v", "action", "log_prob"))
    assert all(v <= 1.0 for v in ratio.values()), (who, {key: v for key, v in ratio.items() if not v <= 1.0})
    assert torch.equal(got["packed"], eng.ilmlp_pack(*split(got["param"], in_dim, 2 * A)))


@pytest.mark.parametrize("k,j", ONE, ids=[S.run_id(k, j, False) for k, j in ONE])
def test_update_against_float64_at_saturated_tanh(eng, k, j):
    """Three updates of oly_iq_pi_update with one critic: the parameters, m, the four scalars, every update's action and
    log_prob, both Standardizers' statistics, packed == ilmlp_pack(param)."""
    check_updates(eng, Dev(eng, S.sat_inputs(k), S.SAT_CONFIGS[j], *P.SHAPES[k]), k, j, False)


@pytest.mark.parametrize("k,j", TWO, ids=[S.run_id(k, j, True) for k, j in TWO])
def test_actor_step_with_two_critics_at_saturated_tanh(eng, k, j):
    """The LSIQ-HC actor step (h_packed): the same, and H's statistics."""
    check_updates(eng, HPiDev(eng, S.sat_inputs(k), S.SAT_CONFIGS[j], *P.SHAPES[k]), k, j, True)


# ------------------------------------------------------------------------------ K25
def run_sg(eng, k, A, eps=True, ctrl=False, ctrl_f64=False):
    """One oly_sg_act on the case k, every operand fenced, every output poisoned.  Returns the Bufs, checked."""
    n, D = k["x"].shape
    b = Bufs()
    packed = b.inp("packed", eng.ilmlp_pack(*[torch.as_tensor(p).cuda() for p in k["params"]]))
    cs = b.inp("colstats", np.zeros((3, D))) if k["standardizer"] else None
    out = dict(action=b.out("action", (n, A), F32), log_prob=b.out("log_prob", (n,), F32), mu=b.out("mu", (n, A), F32),
               log_sigma=b.out("log_sigma", (n, A), F32))
    if ctrl:
        out["ctrl"] = b.out("ctrl", (n, int(eng.il_spec.nu)), F64 if ctrl_f64 else F32)
    eng.sg_act(b.inp("x", k["x"]), packed, b.inp("central", k["central"]), b.inp("delta", k["delta"]), colstats=cs,
               eps=b.inp("eps", k["eps"]) if eps else None, want=tuple(key for key in out if key != "action"),
               ctrl_f64=ctrl_f64, log_std_min=S.SAT_LS[0], log_std_max=S.SAT_LS[1], out=out)
    b.done(f"sg_act n={n} in={D} A={A}", written=tuple(out), finite=tuple(out) + ("colstats",) * bool(cs is not None))
    return b


@pytest.mark.parametrize("i", range(len(S.SG_CASES)), ids=[S.sg_id(i) for i in range(len(S.SG_CASES))])
def test_sg_act_at_saturated_tanh(eng_h1, i):
    eng = eng_h1
    n, D, A, _ = S.SG_CASES[i]
    k = S.sg_sat_case(i)
    ctrl = A == 11
    b = run_sg(eng, k, A, ctrl=ctrl)
    cs, x = b["colstats"].t, b["x"].t
    assert float(cs[0, 0]) == n and torch.equal(cs, eng.col_stats(x, None))
    # mu and log_sigma: the forward kernel's bits, split and clamped
    y = eng.ilmlp_forward(x, b["packed"].t, 2 * A, "identity", colstats=cs)
    assert torch.equal(b["mu"].t, y[:, :A]) and torch.equal(b["log_sigma"].t, torch.clamp(y[:, A:], -20.0, 2.0))
    assert bool((b["log_sigma"].t[:, 0] == 2.0).all()) and bool((y[:, A] > 2.0).all())
    # the float64 side: in place of |a_raw| < 4, the bands
    mu64, ls64, u64, a64, lp64 = float64_of(k, cs, A)
    u = u64.cpu().numpy()
    facts = S.facts_of(u, y[:, A:].double().cpu().numpy())
    print(f"{S.sg_id(i)}: bands {facts['bands']}, large-sigma saturated {facts['big_sigma_saturated']}, |u| max {np.abs(u).max():.2f}")
    assert not S.facts_hold(facts), S.facts_hold(facts)
    err_a = float((b["action"].t.double() - a64).abs().max())
    err_lp = float(((b["log_prob"].t.double() - lp64).abs() / lp64.abs().clamp(min=1.0)).max())
    print(f"{S.sg_id(i)}: |kernel - f64| / TOL action {err_a / TOL:.4f}, log_prob {err_lp / TOL:.4f}")
    assert err_a <= TOL and err_lp <= TOL
    assert bounds_where_tanh_is_one(b["action"].t, u, b["central"].t, b["delta"].t) >= 4
    if ctrl:
        assert torch.equal(b["ctrl"].t, eng.il_ctrl(b["action"].t))
        b64 = run_sg(eng, k, A, ctrl=True, ctrl_f64=True)
        assert b64["ctrl"].t.dtype == F64 and torch.equal(b64["ctrl"].t, eng.il_ctrl(b64["action"].t, ctrl_f64=True))
        assert torch.equal(b64["action"].bytes, b["action"].bytes)
    # deterministic: the squashed mean, nothing drawn; a second run of either has the same bits
    det = run_sg(eng, k, A, eps=False)
    assert torch.equal(det["mu"].bytes, b["mu"].bytes) and torch.equal(det["colstats"].bytes, b["colstats"].bytes)
    ref = torch.tanh(mu64) * b["delta"].t.double() + b["central"].t.double()
    assert float((det["action"].t.double() - ref).abs().max()) <= TOL
    assert not torch.equal(det["action"].t, b["action"].t)
    for first, again in ((b, run_sg(eng, k, A, ctrl=ctrl)), (det, run_sg(eng, k, A, eps=False))):
        for key in ("action", "log_prob", "mu", "log_sigma", "colstats") + (("ctrl",) if "ctrl" in again else ()):
            assert torch.equal(first[key].bytes, again[key].bytes), key


def test_paired_act_has_the_materialised_bits_at_saturated_tanh(eng):
    """K28's draw: oly_sg_act on two tables with idx (strides wider than the widths) against the same call on the rows
    torch materialises, on a saturated case: iam_restate's widest case with the table's biases and noise."""
    (c, k), n = S.paired_sat_case(), S.PAIRED_ROWS
    for use_idx in (True, False):
        one, rows = run_act(eng, c, k, n, True, use_idx)
        two, _ = run_act(eng, c, k, n, False, use_idx)
        for key in ("action", "log_prob", "mu", "log_sigma", "colstats"):
            assert torch.equal(one[key].bytes, two[key].bytes), (use_idx, key)
        assert float(one["colstats"].t[0, 0]) == n and bool((one["log_sigma"].t[:, 0] == 2.0).all())
        u = one.host("mu").astype(np.float64) + np.exp(one.host("log_sigma").astype(np.float64)) * k["eps"][:n]
        y = eng.ilmlp_forward(two["x"].t, two["packed"].t, 2 * c.A, "identity", colstats=two["colstats"].t)
        facts = S.facts_of(u, y[:, c.A:].double().cpu().numpy())
        print(f"paired, idx {use_idx}: bands {facts['bands']}, large-sigma saturated {facts['big_sigma_saturated']}")
        assert not S.facts_hold(facts), S.facts_hold(facts)
        assert bounds_where_tanh_is_one(one["action"].t, u, one["central"].t, one["delta"].t) >= 4


# ------------------------------------------------------------------------------ K25 and K27 agree
@pytest.mark.parametrize("k", S.TWO_CRITICS, ids=["-".join(map(str, P.SHAPES[k])) for k in S.TWO_CRITICS])
@pytest.mark.parametrize("standardizer", (False, True), ids=("nostd", "std"))
def test_the_updates_action_and_log_prob_are_sg_acts_at_saturated_tanh(eng, k, standardizer):
    """On the same weights, statistics and noise oly_iq_pi_update's stored action and log_prob of the first update have
    oly_sg_act's bits; test_gpu_iq_pi.py's test_the_calls_bits shows it with |u| < 4 only."""
    in_dim, A, Bp = P.SHAPES[k]
    case, cfg = S.sat_inputs(k), S.SAT_CONFIGS[0 if standardizer else 1]
    dev = Dev(eng, case, cfg, in_dim, A, Bp)
    start = None
    if standardizer:     # statistics that already hold rows: (count, sum, sumsq) of 7 earlier ones
        x0 = np.random.default_rng(3).standard_normal((7, in_dim)) * 2 + 1
        start = torch.as_tensor(np.stack([np.full(in_dim, 7.0), x0.sum(0), np.square(x0).sum(0)])).cuda()
        dev.t("colstats").copy_(start)
    before = dev.snapshot()
    dev.update(case["steps"][0])
    got = dev.snapshot()
    dev.check_fences("K25 and K27")
    b = Bufs()
    out = dict(action=b.out("action", (Bp, A), F32), log_prob=b.out("log_prob", (Bp,), F32), mu=b.out("mu", (Bp, A), F32),
               log_sigma=b.out("log_sigma", (Bp, A), F32))
    eng.sg_act(dev.inputs["x"].t, b.inp("packed", before["packed"]), dev.t("central"), dev.t("delta"),
               colstats=b.inp("colstats", start) if standardizer else None, eps=dev.inputs["eps"].t,
               update_stats=standardizer, log_std_min=cfg.ls_min, log_std_max=cfg.ls_max, want=("log_prob", "mu", "log_sigma"),
               out=out)
    b.done("sg_act", written=tuple(out))
    dev.check_fences("sg_act on the update's operands")
    assert torch.equal(got["action"], out["action"]) and torch.equal(got["log_prob"], out["log_prob"])
    if standardizer:
        assert torch.equal(got["colstats"], b["colstats"].t)
    u = b.host("mu").astype(np.float64) + np.exp(b.host("log_sigma").astype(np.float64)) * case["steps"][0]["eps"]
    assert (np.abs(u[:4, 0]) >= S.EDGES[2]).all() and bool((out["log_sigma"][:, 0] == 2.0).all())
    assert bounds_where_tanh_is_one(got["action"], u, dev.t("central"), dev.t("delta")) >= 4
