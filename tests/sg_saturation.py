"""K25 (oly_sg_act) and K27 (oly_iq_pi_update, one critic or two) where the agents run them and the older sweeps do not: the
reference's clamp log_std in [-20, 2], a column clamped at sigma = exp(2) = 7.39, an unclamped one at sigma = 4.5, and
tanh saturated up to the point where fp64 tanh is exactly -+1 and 1 - a^2 is 0.  No tests here: tables and builders.
tests/test_sg_saturation_cpu.py holds the tables to their purpose without a GPU, tests/test_gpu_sg_saturation.py runs the
kernels on them.

Why a table of its own.  iq_pi_restate's sweep narrows the clamp to [-3, -0.5] and test_gpu_sg_act.py keeps |a_raw| < 4,
because their conditioning check is torch's ALL-float32 run, and that run evaluates 1 - a^2 + 1e-6 in float32: once tanh
saturates it strays from float64 by 1e-3 on a parameter and can vouch for no case.  The kernels do not compute that term in
float32.  They form tanh, 1 - th^2, the guard, the logarithm, the Gaussian term and dL/du in fp64 from the float32 sample
(csrc/k25_sg_act.hip's and csrc/k27_iq_policy.hip's epilogues), and d/du log(1 - tanh(u)^2 + 1e-6) is bounded by 2, so
against float64 they are well conditioned at any |u|.  The conditioning check of these tables is therefore
kernel_model_act: the twin in float32 with that epilogue in float64, the kernels' arithmetic up to summation order.  It
guards a case against a relu that float32 takes on the other side exactly as the float32 run does, and never evaluates
the ill-conditioned float32 expression.  A case is accepted if the model lies within TOL / 4 of float64.

What the older sweeps cannot see (READINGS, both measured by tests/test_sg_saturation_cpu.py):
  "stable_identity_gradient"  the value of the guarded correction with the gradient of the stable SAC identity
                              log(1 - tanh(u)^2) = 2 (log 2 - u - softplus(-2u)), -2 tanh(u) instead of
                              2 a (1 - a^2) / (1 - a^2 + 1e-6);
  "no_guard"                  log(1 - a^2) without the 1e-6, value and gradient.
Both pass iq_pi_restate's sweep within TOL and miss these tables by far more than 10 TOL (or are not finite).

The lower clamp end stays out.  At log_sigma -> -20 the sample m + expf(ls) eps rounds to m in float32; d = a_raw - m is
then 0 or a few ulps of m against sigma = 2e-9, and the Gaussian term is quantisation noise in the reference's float32
run as well as in the kernels.  Holding d / sigma to 1e-5 needs sigma >~ 1e-2 |m|, log_sigma >~ -4.6; column 2's -6 is
held through log_prob's relative bound only because |m| is small there.  The finite-and-exact-clamp test of that end
(test_gpu_sg_act.py::test_log_sigma_past_both_clamp_bounds) stays as it is."""
import numpy as np
import torch

import bc_log_restate as blr
import iq_pi_restate as P
import lsiq_h_restate as H
from bc_restate import Standardizer
from il_shapes import linear_params

TOL = P.TOL
SAT_LS = (P.LOG_STD_MIN, P.LOG_STD_MAX)
assert SAT_LS == (-20.0, 2.0)
# iq_pi_restate's two configs (both Standardizers and a weight decay; neither) with the agents' clamp; Adam's eps, the
# learning rate and the weight decay stay the sweep's.
SAT_CONFIGS = tuple(c._replace(ls_min=SAT_LS[0], ls_max=SAT_LS[1]) for c in P.CONFIGS)
SAT_SHAPES = (1, 2, 3, 4)        # indices into iq_pi_restate.SHAPES: (12,5,18), (16,16,16), (32,11,48), (48,16,33); A = 1
TWO_CRITICS = (1, 4)             # has no second column and stays out.  The LSIQ-HC actor step runs on these two.
BIAS0 = 3.0                      # column 0's log_sigma bias: clamped at 2, sigma 7.39, no log_sigma gradient, mu's live
BIAS1 = 1.5                      # column 1's: unclamped, sigma ~ 4.5, du sigma eps - alpha / B with a large sigma
BIAS2 = -6.0                     # column 2's, as in iq_pi_restate.case_inputs: unclamped here, sigma 2.5e-3
PLACED = (3.2, -3.2, 4.0, -4.0)  # column 0's noise in rows 0 .. 3 of every update: |u| ~ 23.6 and 29.6
EDGES = (5.0, 9.0, 19.1)         # bands of |u|: [0, 5), [5, 9) (1 - a^2 < 2e-4), [9, 19.1) (1 - a^2 below the guard), and
#                                  [19.1, inf): fp64 tanh is exactly -+1 from |u| = 19.07 on, 1 - a^2 = 0, the guard alone
#                                  is left; 19.1 keeps the float32 sample's 1e-5 clear of that edge.
READINGS = ("stable_identity_gradient", "no_guard")
THREADS = (1, 4, 8, 16)          # torch's sums change their order with the thread count

# ---------------------------------------------------------------------------------------------- the seeds
# As bc_big_shapes.BC_SEEDS were, the seed of every shape was chosen on the CPU (python tests/sg_saturation.py prints this
# table again).  Tried: the first TRIED seeds from 20 upwards at which facts_hold's conditions hold on every (config,
# update), with one critic and, at TWO_CRITICS, with two; at 12 to 14 free rows in column 0 both signs in [9, 19.1) on all
# three updates is the rare one, so the small shapes walk further.  A candidate is a tried seed at which kernel_model_act
# lies within TOL / 4 of float64 on every tensor of the rule (distances()), in both configs, with torch on 1, 4, 8 and 16
# threads.  Chosen: the candidate whose worst distance is smallest, the lower seed on a tie.  Per shape: the seeds tried,
# the candidates among them, the chosen seed's worst model distance in units of TOL / 4 (one critic; two), and in
# brackets the worst among the seeds tried.
#   (12, 5, 18):  24 31 44 45 51 60 70 72 88 90 (of 20 .. 90);  10 of 10;  seed 44: 0.044; 0.044  (0.070)
#   (16, 16, 16): 37 42 49 50 55 56 61 70 78 80 (of 20 .. 80);  10 of 10;  seed 49: 0.044         (0.059)
#   (32, 11, 48): 20 21 23 24 25 26 27 28 29 30;                10 of 10;  seed 23: 0.044         (0.061)
#   (48, 16, 33): 20 21 24 25 26 27 28 29 30 31;                10 of 10;  seed 25: 0.044; 0.044  (0.068)
# 0.044 TOL / 4 = 2.2e-7 is the floor every good seed shares: b3 holds the biases 3 and -6, whose float32 neighbours lie
# 2.4e-7 and 4.8e-7 apart, and Adam's first steps land between them.  The check is not idle: of the seeds passed over because a
# band was one-signed, 25 at (16, 16, 16) puts the model 142 TOL / 4 from float64 and 22 at (48, 16, 33) 97 TOL / 4 (a
# relu taken on the other side); such a seed could not tell a kernel from a rounding.
TRIED = 10
SEEDS = {1: 44, 2: 49, 3: 23, 4: 25}


def saturate(b3, noises, A):
    """The three log_sigma biases and the hand-placed noise, in place."""
    assert A >= 3
    b3[A], b3[A + 1], b3[A + 2] = BIAS0, BIAS1, BIAS2
    for e in noises:
        assert len(e) >= len(PLACED)
        e[:len(PLACED), 0] = PLACED


_CACHE = {}


def sat_inputs(k, seed=None):
    """iq_pi_restate.case_inputs at shape k with the biases and noise above, and a second critic's parameters (hparams,
    as lsiq_h_restate.actor_case draws them) for the two-critic step.  Built once per (k, seed); callers leave it
    unchanged."""
    seed = SEEDS[k] if seed is None else seed
    if ("in", k, seed) not in _CACHE:
        in_dim, A, Bp = P.SHAPES[k]
        case = P.case_inputs(in_dim, A, Bp, seed)
        saturate(case["pparams"][5], [s["eps"] for s in case["steps"]], A)
        case["hparams"] = linear_params([(in_dim + A, 512), (512, 256), (256, 1)], H.H_SEED_OFFSET + seed)
        _CACHE[("in", k, seed)] = case
    return _CACHE[("in", k, seed)]


# ---------------------------------------------------------------------------------------------- the acts
def _sample(pi, x, eps):
    """Policy.act's first lines, the raw log_sigma kept: mu, raw, log_sigma, sigma, u = mu + sigma eps in the policy's
    dtype."""
    y = pi.heads(x)
    mu, raw = y[:, :pi.A], y[:, pi.A:]
    ls = torch.clamp(raw, pi.cfg.ls_min, pi.cfg.ls_max)
    sigma = ls.exp()
    return mu, raw, ls, sigma, mu + sigma * torch.as_tensor(np.asarray(eps, np.float32)).to(pi.dtype)


def recording_act(log):
    """Policy.act, expression for expression, that appends dict(raw, u) of every call to `log`."""
    def act(pi, x, eps):
        mu, raw, _, sigma, u = _sample(pi, x, eps)
        a = torch.tanh(u)
        logp = torch.distributions.Normal(mu, sigma).log_prob(u).sum(dim=1)
        logp = logp - torch.log(1.0 - a.pow(2) + 1e-6).sum(dim=1)
        log.append(dict(raw=raw.detach().double().numpy().copy(), u=u.detach().double().numpy().copy()))
        return a * pi.delta + pi.central, logp
    return act


def kernel_model_act(pi, x, eps):
    """K25's and K27's arithmetic on a float32 policy: the forward, the clamp and the sample u = mu + exp(ls) eps in
    float32; then from u.double(): tanh, the Gaussian term -(u - mu)^2 / (2 sigma^2) - ls - log sqrt(2 pi), log(1 - a^2 +
    1e-6) and the row sums in float64.  The action is float32(tanh) delta + central in float32.  The Gaussian term's
    quadratic is eps^2 / 2, a constant, and the kernel gives it no gradient (dL/dlog_sigma = du sigma eps - alpha / B):
    it is detached here.  The gradient dL/du is formed in float64 and rounded to float32 where it re-enters the network,
    as the kernel rounds du."""
    assert pi.dtype == torch.float32
    mu, _, ls, _, u = _sample(pi, x, eps)
    u64, ls64 = u.double(), ls.double()
    a = torch.tanh(u64)
    gauss = (-(u64 - mu.double()) ** 2 / (2.0 * torch.exp(ls64) ** 2)).detach() - ls64 - blr.HALF_LOG_2PI
    logp = gauss.sum(dim=1) - torch.log(1.0 - a * a + 1e-6).sum(dim=1)
    return a.float() * pi.delta + pi.central, logp


def reading_act(kind):
    """The two wrong readings of the tanh correction, in the policy's dtype."""
    assert kind in READINGS

    def act(pi, x, eps):
        mu, _, _, sigma, u = _sample(pi, x, eps)
        a = torch.tanh(u)
        # no_guard's first step leaves NaN parameters: the later ones run on, so that the run ends and is seen not finite
        logp = torch.distributions.Normal(mu, sigma, validate_args=False).log_prob(u).sum(dim=1)
        if kind == "no_guard":
            corr = torch.log(1.0 - a.pow(2))
        else:
            value = torch.log(1.0 - a.pow(2) + 1e-6)
            stable = 2.0 * (np.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))
            corr = stable + (value - stable).detach()            # the guarded value, the identity's gradient -2 tanh(u)
        return a * pi.delta + pi.central, logp - corr.sum(dim=1)
    return act


# ---------------------------------------------------------------------------------------------- the runs
def run_with(case, cfg, dtype=torch.float64, act=None, two=False):
    """iq_pi_restate.run, or with two critics lsiq_h_restate.run_actor (what
    test_gpu_lsiq_h_actor.py::test_actor_step_against_float64 restates), with `act` in Policy.act's place."""
    if two:
        return H.run_actor(case, cfg, dtype, act=act)
    return P.run(case, cfg, dtype, act=act)


def run_model(case, cfg, two=False):
    return run_with(case, cfg, torch.float32, kernel_model_act, two)


def run_reading(case, cfg, kind, two=False):
    return run_with(case, cfg, torch.float64, reading_act(kind), two)


def sat_yardstick(k, j, two=False, seed=None):
    """(float64 state, out, acts, log) of config j at shape k: the yardstick and, per update, the raw log_sigma and the
    sample it drew (recording_act).  Computed once and shared."""
    seed = SEEDS[k] if seed is None else seed
    if (k, j, two, seed) not in _CACHE:
        log = []
        _CACHE[(k, j, two, seed)] = run_with(sat_inputs(k, seed), SAT_CONFIGS[j], act=recording_act(log), two=two) + (log,)
    return _CACHE[(k, j, two, seed)]


def distances(got, ref):
    """How far the run `got` (state, out, acts) lies from `ref`, per tensor in units of TOL, by test_gpu_iq_pi.py's rule:
    each parameter tensor absolutely, m relative to its largest entry, the four scalars relative to max(1, |value|), the
    action absolutely and log_prob relative to max(1, |log_prob| max), the last two over every update."""
    (st, out, acts), (rst, rout, racts) = got[:3], ref[:3]
    with np.errstate(invalid="ignore"):
        d = {n: np.abs(a - r).max() for n, a, r in zip(P.NAMES, st["policy"]["params"], rst["policy"]["params"])}
        r = P.cat(rst["policy"]["exp_avg"])
        d["m"] = np.abs(P.cat(st["policy"]["exp_avg"]) - r).max() / np.abs(r).max()
        d["scalars"] = (np.abs(out - rout) / np.maximum(1.0, np.abs(rout))).max()
        d["action"] = max(np.abs(a - ra).max() for (a, _), (ra, _) in zip(acts, racts))
        d["log_prob"] = max(np.abs(lp - rlp).max() / max(1.0, np.abs(rlp).max()) for (_, lp), (_, rlp) in zip(acts, racts))
    return {k: float(v) / TOL for k, v in d.items()}


def worst(d):
    """The largest of distances(); inf if any is not finite."""
    v = np.array(list(d.values()))
    return float(v.max()) if np.isfinite(v).all() else float("inf")


# ---------------------------------------------------------------------------------------------- what the tables must hold
def facts_of(u, raw, lo=SAT_LS[0], hi=SAT_LS[1]):
    """Of one call's float64 sample u and raw log_sigma [n, A]: bands [4][2] the entries per band of |u| (EDGES) and sign
    (negative, positive); high / low / unclamped the log_sigma entries above, below and inside the clamp; high_columns
    the columns clamped high on all rows; big_sigma_saturated the unclamped entries with raw log_sigma > 1 and |u| >= 5;
    placed whether column 0's rows 0 .. 3 lie in the last band with PLACED's signs."""
    band = np.digitize(np.abs(u), EDGES)
    high, low = raw > hi, raw < lo
    free = ~(high | low)
    head = slice(0, len(PLACED))
    return dict(bands=[[int(((band == b) & (u < 0)).sum()), int(((band == b) & (u > 0)).sum())] for b in range(4)],
                high=int(high.sum()), low=int(low.sum()), unclamped=int(free.sum()),
                high_columns=int(high.all(axis=0).sum()),
                big_sigma_saturated=int((free & (raw > 1.0) & (np.abs(u) >= EDGES[0])).sum()),
                placed=bool((band[head, 0] == 3).all() and (np.sign(u[head, 0]) == np.sign(PLACED)).all()))


def sat_facts(case, cfg, two=False, log=None):
    """facts_of for every update of the float64 run of `case`."""
    if log is None:
        log = []
        run_with(case, cfg, act=recording_act(log), two=two)
    return [facts_of(e["u"], e["raw"], cfg.ls_min, cfg.ls_max) for e in log]


def facts_hold(f):
    """The table's purpose on one call: at least 2 entries in each band, both signs in each of the three upper bands, a
    column clamped high on all rows, at least 2 unclamped large-sigma saturated entries, the hand-placed entries in the
    last band.  Returns the list of what is missing (empty: holds)."""
    miss = [f"band {b}: {f['bands'][b]}" for b in range(4) if sum(f["bands"][b]) < 2]
    miss += [f"band {b} one-signed: {f['bands'][b]}" for b in (1, 2, 3) if min(f["bands"][b]) < 1]
    if f["high_columns"] < 1:
        miss.append("no column clamped high on all rows")
    if f["big_sigma_saturated"] < 2:
        miss.append(f"unclamped large-sigma saturated entries: {f['big_sigma_saturated']}")
    if not f["placed"]:
        miss.append("the hand-placed entries are not in the last band")
    return miss


def table():
    """Every K27 run of the tables: (k, j, two)."""
    return [(k, j, False) for k in SAT_SHAPES for j in range(len(SAT_CONFIGS))] + \
           [(k, j, True) for k in TWO_CRITICS for j in range(len(SAT_CONFIGS))]


def run_id(k, j, two):
    return "-".join(map(str, P.SHAPES[k])) + "-" + P.cfg_id(SAT_CONFIGS[j]) + ("-two" if two else "")


def required_present():
    """Holds the tables to their purpose: facts_hold on every (shape, config, update) of K27's table, with one critic
    and two, on K25's two cases and on the paired path's case.  Returns {run id: per-update facts} for the record."""
    assert [P.SHAPES[k] for k in SAT_SHAPES] == [(12, 5, 18), (16, 16, 16), (32, 11, 48), (48, 16, 33)]
    assert all(c.ls_min == -20.0 and c.ls_max == 2.0 and c.adam_eps == P.SWEEP_EPS for c in SAT_CONFIGS)
    assert [(c.standardizer, c.wd, c.lr) for c in SAT_CONFIGS] == [(c.standardizer, c.wd, c.lr) for c in P.CONFIGS]
    seen = {}
    for k, j, two in table():
        facts = sat_facts(sat_inputs(k), SAT_CONFIGS[j], two, log=sat_yardstick(k, j, two)[3])
        assert len(facts) == P.UPDATES
        for i, f in enumerate(facts):
            assert not facts_hold(f), (run_id(k, j, two), i, facts_hold(f), f)
        seen[run_id(k, j, two)] = facts
    for i in range(len(SG_CASES)):
        f = sg_facts(i)
        assert not facts_hold(f), (SG_CASES[i], facts_hold(f), f)
        seen[sg_id(i)] = [f]
    for use_idx in (True, False):
        f = paired_facts(use_idx)
        assert not facts_hold(f), ("paired", use_idx, facts_hold(f), f)
        seen["paired-idx" if use_idx else "paired-rows"] = [f]
    return seen


# ---------------------------------------------------------------------------------------------- K25's table
#            n, in, A, seed (test_gpu_sg_act.py's n % 97 + in + A); both with a Standardizer, the second with controls
SG_CASES = ((45, 19, 7, 71), (33, 32, 11, 76))


def sg_id(i):
    n, D, A, _ = SG_CASES[i]
    return f"n{n}-in{D}-A{A}"


def sg_sat_case(i):
    """test_gpu_sg_act.sg_case with the three biases, the hand-placed noise and the noise not clipped to -+2.  Built once;
    callers leave it unchanged."""
    if ("sg", i) not in _CACHE:
        from test_gpu_sg_act import sg_case
        n, D, A, seed = SG_CASES[i]
        k = sg_case(n, D, A, seed, standardizer=True, clip=None)
        saturate(k["params"][5], [k["eps"]], A)
        _CACHE[("sg", i)] = k
    return _CACHE[("sg", i)]


def sg_host(k, A, dtype=torch.float64, lo=SAT_LS[0], hi=SAT_LS[1]):
    """One oly_sg_act on the host: test_gpu_sg_act.float64_of with the Standardizer's statistics taken from the rows in
    numpy (dtype float64: the yardstick), or the kernel model (dtype float32: the forward, the clamp and the sample in
    float32, the epilogue in float64).  dict(mu, raw, log_sigma, u, action, log_prob) in float64."""
    z = Standardizer(k["x"].shape[1])(k["x"]) if k["standardizer"] else k["x"]
    w = [torch.as_tensor(p).to(dtype) for p in k["params"]]
    z = torch.as_tensor(z).to(dtype)
    y = torch.relu(torch.relu(z @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5]
    mu, raw = y[:, :A], y[:, A:]
    ls = torch.clamp(raw, lo, hi)
    u = mu + ls.exp() * torch.as_tensor(k["eps"]).to(dtype)
    a = torch.tanh(u.double())
    action = a.to(dtype) * torch.as_tensor(k["delta"]).to(dtype) + torch.as_tensor(k["central"]).to(dtype)
    out = dict(mu=mu, raw=raw, log_sigma=ls, u=u, action=action, log_prob=blr.log_prob(mu.double(), ls.double(), u.double()))
    return {key: t.double().numpy() for key, t in out.items()}


def sg_facts(i):
    h = sg_host(sg_sat_case(i), SG_CASES[i][2])
    return facts_of(h["u"], h["raw"])


def sg_distances(got, ref):
    """action absolutely, log_prob relative to max(1, |log_prob|) per row (test_gpu_sg_act.py's rule), in units of TOL."""
    return dict(action=float(np.abs(got["action"] - ref["action"]).max()) / TOL,
                log_prob=float((np.abs(got["log_prob"] - ref["log_prob"]) / np.maximum(1.0, np.abs(ref["log_prob"]))).max()) / TOL)


# ---------------------------------------------------------------------------------------------- the paired path's case
PAIRED_ROWS = 33          # 16 + 16 + 1 of the ring's 40
PAIRED_NOISE_SEED = 7100  # the first from 7100 upwards at which facts_hold holds on both row selections (7104 does not)


def paired_sat_case():
    """(c, k): iam_restate's widest case (32 + 32 columns, strides wider than the widths, A = 16, a Standardizer) with the
    three biases, noise drawn afresh and not clipped, and the hand-placed entries.  Built once; callers leave it
    unchanged."""
    import iam_restate as ir
    c = ir.CASES[3]
    assert (c.d1, c.d2, c.A, c.standardizer) == (32, 32, 16, True) and c.pad1 and c.pad2
    if "paired" not in _CACHE:
        k = dict(ir.build(c))
        k["params"] = [p.copy() for p in k["params"]]
        k["eps"] = np.random.default_rng(PAIRED_NOISE_SEED).standard_normal(k["eps"].shape).astype(np.float32)
        saturate(k["params"][5], [k["eps"]], c.A)
        _CACHE["paired"] = k
    return c, _CACHE["paired"]


def paired_facts(use_idx):
    """facts_of on the rows test_gpu_iam.run_act takes (use_idx: the ring's rows through idx; else rows 0 .. n - 1)."""
    c, k = paired_sat_case()
    n = PAIRED_ROWS
    rows = np.resize(k["idx"].reshape(-1), n) if use_idx else np.arange(n)
    if use_idx:
        rows[0], rows[-1] = len(k["states"]) - 1, 0
    h = sg_host(dict(k, x=k["table"][rows], eps=k["eps"][:n], standardizer=True), c.A)
    return facts_of(h["u"], h["raw"])


# ---------------------------------------------------------------------------------------------- the search
def model_worst(k, seed, threads=THREADS):
    """(missing facts, worst model distance over the configs and thread counts with one critic, with two or None)."""
    case, missing, one, two_ = sat_inputs(k, seed), [], 0.0, 0.0 if k in TWO_CRITICS else None
    keep = torch.get_num_threads()
    try:
        for j, cfg in enumerate(SAT_CONFIGS):
            for two in (False, True) if k in TWO_CRITICS else (False,):
                ref = sat_yardstick(k, j, two, seed)
                for f in sat_facts(case, cfg, two, log=ref[3]):
                    missing += facts_hold(f)
                for n in threads:
                    torch.set_num_threads(n)
                    w = worst(distances(run_model(case, cfg, two), ref))
                    one, two_ = (one, max(two_, w)) if two else (max(one, w), two_)
    finally:
        torch.set_num_threads(keep)
    return missing, one, two_


def search(first=20):
    for k in SAT_SHAPES:
        tried, seed = [], first
        while len(tried) < TRIED:          # the first TRIED seeds at which the table's conditions hold on every update
            runs = [(j, two) for j in range(len(SAT_CONFIGS)) for two in ((False, True) if k in TWO_CRITICS else (False,))]
            if not any(facts_hold(f) for j, two in runs
                       for f in sat_facts(None, SAT_CONFIGS[j], two, log=sat_yardstick(k, j, two, seed)[3])):
                tried.append(seed)
            seed += 1
        print(f"{P.SHAPES[k]}: seeds {first} .. {seed - 1} walked, the conditions hold at {tried}")
        rows = [(seed,) + model_worst(k, seed) for seed in tried]
        for seed, missing, one, two in rows:
            print(f"{P.SHAPES[k]} seed {seed}: model / (TOL / 4) one critic {4 * one:.3f}"
                  + (f", two {4 * two:.3f}" if two is not None else "") + (f"  MISSING {missing[:2]}" if missing else ""))
        ok = [(max(one, two or 0.0), seed) for seed, missing, one, two in rows if not missing and 4 * max(one, two or 0.0) <= 1.0]
        print(f"{P.SHAPES[k]}: {len(ok)} candidates of {TRIED}, best {min(ok) if ok else None}, "
              f"worst tried {4 * max(max(one, two or 0.0) for _, _, one, two in rows):.3f}")


if __name__ == "__main__":
    search()
