"""The large batches at which K26 (oly_iq_q_update: IQ, SQIL, LSIQ, LSIQ_H / LSIQ_HC) and K27 (oly_iq_pi_update with one
critic and with two, oly_iq_alpha_update) are compared with the float64 restatements of tests/iq_restate.py,
lsiq_restate.py, lsiq_h_restate.py and iq_pi_restate.py, and the builders of those cases.  No tests here:
tests/test_iq_big_shapes_cpu.py holds the tables to their conditions without a GPU, tests/test_gpu_iq_big_shapes.py runs
the kernels.

The small sweeps of those files stop at 48 rows, three 16-row tiles.  What only a larger batch runs: the second and later
trips of the weights kernel's unrolled loop over 16-row steps (dw_accumulate of csrc/ilmlp_fit.h, STEP_UNROLL steps at a
time, ceil(steps / 4) steps per wave) and wave shares that end inside a group; statistics slices of the prologue with
several rows per chain and a short last slice; the second trip of the loops that stride by the workgroup's 256 threads
(LSIQ_H's batch scalars, the alpha update); per-tile partials of more than three tiles, up to the 256 the folds are built
for; a policy / expert boundary inside a middle tile; workspaces of millions of floats.

Every case is rebuilt from its seed by the builders of the small sweeps (iq_restate.case_inputs, lsiq_h_restate.h_inputs,
iq_pi_restate.case_inputs) and runs UPDATES = 2 updates: the second steps from non-zero moments and, with Standardizers,
from non-empty statistics.  Adam's eps, the learning rates, the scaled output layer of the LSIQ sweeps and the log_std
clamp are the small sweeps', for the reasons written there."""
import numpy as np
import torch

import iq_pi_restate as P
import iq_restate as R
import lsiq_h_restate as H
import lsiq_restate as L
from il_shapes import linear_params

TOL, cat = R.TOL, R.cat
UPDATES = 2
TILE, STEP_UNROLL, WAVES, NSP, THREADS = 16, 4, 4, 16, 256     # csrc/ilmlp_fit.h, csrc/k26_iq_critic.hip
MAX_BATCH = 4096                                               # OLY_BC_MAX_BATCH

# ---------------------------------------------------------------------------------------------- the shapes
# K26 (in_dim, A, B, n_policy):
#   (17, 6, 257, 1)      17 tiles, the last of one row; one past 256, so the second trip of the strided loops has one row;
#                        one policy row; D = 23 takes the <2> instantiation; the last statistics slice has 2 rows
#   (32, 11, 300, 150)   19 tiles, the last of 12 rows; the subset boundary inside tile 9; D = 43 takes <4>
#   (48, 16, 1040, 520)  65 tiles, equal halves, the boundary mid-tile; three slots make 195 steps, 49 per wave
#   (48, 16, 4096, 2048) the limit: 256 tiles, D = 64
#   (1, 1, 4095, 4094)   the smallest widths, a last tile of 15 rows, one expert row, in the last tile
K26_SHAPES = ((17, 6, 257, 1), (32, 11, 300, 150), (48, 16, 1040, 520), (48, 16, 4096, 2048), (1, 1, 4095, 4094))
K27_SHAPES = tuple(s[:3] for s in K26_SHAPES)                  # (in_dim, A, Bp)
ALPHA_N = (256, 257, 4095, 4096)
EVERY = (0, 3)               # the 257-row and the 4096-row shape: every config runs there
OTHER = (1, 2, 4)            # the rest of the list rotates over these


def tiles(B):
    return (B + TILE - 1) // TILE


def last_tile(B):
    return B - (tiles(B) - 1) * TILE


def steps_of(B, slots=3):
    """The 16-row steps of the weights kernel with `slots` gradient passes, and a wave's share of them."""
    n = slots * tiles(B)
    return n, (n + WAVES - 1) // WAVES


def stat_slices(nb):
    """The rows of the prologue's NSP statistics slices for a pass of nb rows."""
    per = (nb + NSP - 1) // NSP
    return [max(0, min(nb, (s + 1) * per) - s * per) for s in range(NSP)]


def required_shapes_present():
    """The shapes the tables exist for, computed from the tables; raises AssertionError naming the first one missing."""
    k26, k27 = K26_SHAPES, K27_SHAPES
    assert len(set(k26)) == len(k26) and len(set(k27)) == len(k27), "a shape is listed twice"
    assert all(0 < i and 0 < a <= 16 and i + a <= 64 and 2 <= b <= 4096 and 1 <= n < b for i, a, b, n in k26)
    assert {s[:3] for s in k26} == set(k27), "K27 runs at K26's shapes"
    for table, name in (([s[2] for s in k26], "K26"), ([s[2] for s in k27], "K27")):
        for n in (17, 19, 65, 256):
            assert any(tiles(b) == n for b in table), f"{name}: {n} tiles"
        for n in (1, 12, 15):
            assert any(last_tile(b) == n for b in table), f"{name}: a last tile of {n} rows"
        assert any(b > THREADS and b % THREADS == 1 for b in table), f"{name}: a second strided trip of one row"
    inside = lambda b, n: n % TILE != 0 and 0 < n // TILE < tiles(b) - 1
    assert any(inside(b, n) for _, _, b, n in k26), "a policy / expert boundary inside a middle tile"
    assert any(n == 1 for *_, n in k26), "n_policy = 1"
    assert any(n == b - 1 for _, _, b, n in k26), "n_policy = B - 1"
    assert any(2 * n == b and n % TILE for _, _, b, n in k26), "equal halves with the boundary mid-tile"
    assert any(i + a <= 32 for i, a, _, _ in k26) and any(i + a > 32 for i, a, _, _ in k26), "both instantiations"
    assert any(i + a == 64 and b == MAX_BATCH for i, a, b, _ in k26), "the limit: the largest batch at the widest row"
    assert any(i == 1 and a == 1 for i, a, _, _ in k26), "the narrowest row"
    shares = [steps_of(b)[1] for _, _, b, _ in k26]
    assert any(q > STEP_UNROLL and q % STEP_UNROLL for q in shares), "a wave's share of steps that is no multiple of 4"
    assert any(steps_of(b)[0] % WAVES and steps_of(b)[1] > STEP_UNROLL for _, _, b, _ in k26), "a shorter last wave"
    assert any(0 < stat_slices(b)[-1] < stat_slices(b)[0] and stat_slices(b)[0] > 2 * WAVES for _, _, b, _ in k26), \
        "statistics slices of several rows per chain with a short last one"
    assert any(n > 2 * THREADS and n % THREADS for *_, n in k26), "the policy rows' cut in a later strided trip"
    assert set(ALPHA_N) >= {THREADS, THREADS + 1, 4095, 4096}, "the alpha update's n"


# ---------------------------------------------------------------------------------------------- the configs
# A short list per algorithm, not the cross product: the loss modes are swept at the small shapes, here the batch machinery
# is under test.  The hyperparameters are the small sweeps' (iq_restate.sweep_configs, lsiq_restate.sweep_configs,
# lsiq_h_restate.sweep_configs).
_IQ = dict(tau=0.05, adam_eps=R.SWEEP_EPS)
_LS = dict(tau=0.05, adam_eps=L.SWEEP_EPS, lr=L.SWEEP_LR, q_min=L.Q_MIN, q_max=L.Q_MAX)
Q_CONFIGS = (
    # IQ without a target: three gradient slots, both Standardizers' passes, a weight decay
    ("iq", R.Cfg(algo="iq", mode="value", reg="exp_and_plcy", use_target=False, standardizer=True, wd=1e-4, **_IQ)),
    ("iq", R.Cfg(algo="iq", mode="value_expert", reg="exp", treat=True, use_target=True, standardizer=False, **_IQ)),
    ("iq", R.Cfg(algo="sqil", mode="value_plcy", use_target=True, R_min=-0.25, R_max=1.5, **_IQ)),
    ("lsiq", L.LCfg(type="iq_like", exp_mode="fix", exp_loss="Huber", clip=True, use_target=True, mode="value", **_LS)),
    ("lsiq", L.LCfg(type="sqil_like", exp_mode="bootstrap", exp_loss="Huber", clip=True, use_target=False, mode="value_plcy",
                    treat=True, reg_mult=2.0, wd=1e-4, **_LS)),
    ("lsiq", L.LCfg(type="sqil_like", exp_mode="fix", exp_loss="MSE", clip=False, use_target=True, mode="value",
                    standardizer=False, reg_mult=2.0, **_LS)),
    ("h", H.CONFIGS[0]),          # LSIQ_H, MSE, clip_expert, Standardizers, a weight decay
    ("h", H.CONFIGS[12]),         # LSIQ_HC, Huber, clip_expert, Standardizers, a weight decay
)
PI_CONFIGS = tuple((cfg, two) for cfg in P.CONFIGS for two in (False, True))     # (config, with the second critic H)


def q_cfg_id(j):
    fam, c = Q_CONFIGS[j]
    return {"iq": R.cfg_id, "lsiq": L.cfg_id, "h": H.cfg_id}[fam](c)


def pi_cfg_id(j):
    c, two = PI_CONFIGS[j]
    return P.cfg_id(c) + ("-qh" if two else "-q")


def _needs_equal_halves(fam, c):
    return fam == "lsiq" and c.type == "sqil_like" and c.mode == "value"


def _everywhere(fam, c):
    """The two configs the sensitivity check takes at every shape: IQ without a target and SQIL."""
    return fam == "iq" and (c.algo == "sqil" or not c.use_target)


def q_shapes_of(j):
    """The shapes config j runs at: the 257-row and the 4096-row shape and one of the other three in rotation, as
    iq_restate.sweep rotates; sqil_like / value at the equal-halves shapes only (it is refused elsewhere); IQ without a
    target and SQIL at all five."""
    fam, c = Q_CONFIGS[j]
    if _needs_equal_halves(fam, c):
        return tuple(k for k, s in enumerate(K26_SHAPES) if 2 * s[3] == s[2])
    if _everywhere(fam, c):
        return tuple(range(len(K26_SHAPES)))
    rotating = [i for i, (f, d) in enumerate(Q_CONFIGS) if not _needs_equal_halves(f, d) and not _everywhere(f, d)]
    return tuple(sorted(EVERY + (OTHER[rotating.index(j) % len(OTHER)],)))


def pi_shapes_of(j):
    return tuple(sorted(EVERY + (OTHER[j % len(OTHER)],)))


Q_CASES = tuple((k, j) for k in range(len(K26_SHAPES)) for j in range(len(Q_CONFIGS)) if k in q_shapes_of(j))
PI_CASES = tuple((k, j) for k in range(len(K27_SHAPES)) for j in range(len(PI_CONFIGS)) if k in pi_shapes_of(j))


def q_case_id(case):
    return "-".join(map(str, K26_SHAPES[case[0]])) + "-" + q_cfg_id(case[1])


def pi_case_id(case):
    return "-".join(map(str, K27_SHAPES[case[0]])) + "-" + pi_cfg_id(case[1])


def required_configs_present():
    """What the config tables must hold, and that every config meets every shape it has to."""
    cfgs = lambda fam: [c for f, c in Q_CONFIGS if f == fam]
    iq, ls, h = cfgs("iq"), cfgs("lsiq"), cfgs("h")
    assert any(c.algo == "iq" and not c.use_target and c.mode == "value" and c.reg == "exp_and_plcy" and c.standardizer
               and c.wd > 0 for c in iq), "IQ without a target, value, exp_and_plcy, Standardizers, a weight decay"
    assert any(c.algo == "iq" and c.use_target and not c.standardizer for c in iq), "IQ with a target, no Standardizers"
    assert any(c.algo == "sqil" and c.mode == "value_plcy" and c.use_target for c in iq), "SQIL value_plcy with a target"
    assert any(c.type == "iq_like" and c.clip and c.use_target for c in ls), "LSIQ iq_like with target clipping"
    assert any(c.type == "sqil_like" and c.mode == "value_plcy" for c in ls), "LSIQ sqil_like / value_plcy"
    assert any(c.type == "sqil_like" and c.mode == "value" for c in ls), "LSIQ sqil_like / value"
    assert any(c.clip_expert and not c.cost for c in h) and any(c.clip_expert and c.cost for c in h), "LSIQ_H, LSIQ_HC"
    assert {(c, two) for c, two in PI_CONFIGS} == {(c, two) for c in P.CONFIGS for two in (False, True)}, "K27's configs"
    halves = {k for k, s in enumerate(K26_SHAPES) if 2 * s[3] == s[2]}
    for j, (fam, c) in enumerate(Q_CONFIGS):
        at = set(q_shapes_of(j))
        if _needs_equal_halves(fam, c):
            assert at == halves and len(at) >= 2 and 3 in at, (q_cfg_id(j), at)
        else:
            assert set(EVERY) <= at and at & set(OTHER), (q_cfg_id(j), at)
    for j in range(len(PI_CONFIGS)):
        assert set(EVERY) <= set(pi_shapes_of(j)) and set(pi_shapes_of(j)) & set(OTHER), pi_cfg_id(j)
    for k in range(len(K26_SHAPES)):
        here = [Q_CONFIGS[j] for kk, j in Q_CASES if kk == k]
        assert any(f == "iq" and c.algo == "iq" for f, c in here) and any(f == "iq" and c.algo == "sqil" for f, c in here), k
        assert any(kk == k for kk, _ in PI_CASES), k
    for k in OTHER:
        assert len({f for kk, j in Q_CASES if kk == k for f, _ in (Q_CONFIGS[j],)}) >= 2, k
    assert set(Q_CASES) == {(k, j) for j in range(len(Q_CONFIGS)) for k in q_shapes_of(j)}


# ---------------------------------------------------------------------------------------------- the seeds
# At 4096 rows x 768 hidden units x up to three passes some pre-activation lies within float32 rounding of zero; torch's
# own float32 run then takes the other side of a relu and strays from float64 by more than TOL, and such a case cannot tell
# a kernel from a rounding.  So, as il_shapes.py does for its two cases above 16 384 rows, the seed of every (family,
# shape) was chosen on the CPU: of the TRIED seeds from 10 upwards, the candidates are those at which the float32
# restatement stays within TOL / 4 of float64 on every parameter and target tensor for every config that runs at the shape
# (the condition tests/test_iq_cpu.py puts on the small table; tests/test_iq_big_shapes_cpu.py re-asserts it for the seeds
# below) and, for the LSIQ families, at which both runs take the same side of every clip, of Huber's kink and of the
# running maximum's branch on every row; among the candidates the seed whose smallest |pre-activation| relative to the sum
# of the absolute values of its terms, over every layer, pass, update and config of the shape, is largest.
# Measured on the CPU, seeds 10 .. 33 (TRIED = 24) for every family and shape.  Per entry below: candidates of the 24, the
# worst float32 spread on a parameter or target tensor at the chosen seed, its relative margin, and the worst spread among
# the seeds tried (what an unchosen seed can do).  No seed failed on the sides alone (one did on both, lsiq at 4096 rows,
# seed 16).  Above 1000 rows the relative margin is near 1e-8, below float32's rounding of a 64- to 512-term sum: with
# some 2e7 pre-activations per case none of the seeds keeps every one clear of zero, and what the TOL / 4 condition selects
# is that the units which do change side carry too little gradient to matter.  The order of torch's float32 sums changes
# with its thread count; the chosen seeds of every family hold TOL / 4 on 1, 4, 8 and 16 threads.
TRIED = 24
SEEDS = {
    #        257 rows: 23 of 24, 1.0e-6, 2.0e-7 (3.5e-4)     300: 22, 1.3e-6, 2.4e-7 (7.8e-4)    1040: 21, 1.1e-7, 6.0e-8 (5.8e-4)
    #        4096: 11, 8.2e-7, 1.1e-8 (4.1e-4)               4095: 20, 1.0e-7, 2.4e-8 (6.8e-5)
    # At 4096 rows seed 29 has a margin 2 % larger and held TOL / 4 with torch's sums on 2 threads, but strays by 4.4e-5 with
    # them on 8 (IQ without a target); the kernel, whose sums have an order of their own, strayed there by the same 4.4e-5.
    # So the float32 run of the IQ family was repeated on 1, 2, 4 and 8 threads and a candidate holds TOL / 4 on all.
    # At 4095 rows seed 13 has the largest margin (2.6e-8), but its row 4093 lies so near row 4094 that SQIL tells the
    # boundary row misread by 9.6 tolerances only; 17 is the next candidate (92 tolerances).
    "iq": (11, 23, 19, 26, 17),
    #        257: 23, 8.8e-8, 6.6e-7 (5.1e-6)   300: 23, 9.0e-8, 3.3e-7 (9.9e-6)   1040: 19, 6.9e-8, 7.4e-8 (5.9e-5)
    #        4096: 17, 6.7e-8, 2.4e-8 (3.8e-5)  4095: 22, 9.5e-8, 3.6e-8 (1.2e-5)
    "lsiq": (10, 32, 22, 10, 17),
    #        257: 23, 6.8e-8, 7.2e-7 (2.7e-5)   300: 24, 7.0e-8, 6.7e-7 (1.1e-7)   1040: 23, 7.1e-8, 3.2e-7 (1.1e-5)
    #        4096: 22, 7.1e-8, 2.6e-8 (4.6e-5)  4095: no H case runs there (the seed serves nothing)
    "h": (23, 14, 15, 16, 10),
    #        257: 22, 1.6e-7, 2.4e-7 (1.2e-4)   300: 23, 1.6e-7, 1.6e-7 (1.0e-4)   1040: 20, 1.6e-7, 1.3e-7 (4.2e-5)
    #        4096: 18, 1.6e-7, 2.2e-8 (4.0e-5)  4095: 24, 8.4e-8, 1.6e-7 (4.3e-6)
    "pi": (21, 10, 18, 22, 20),
}


# ---------------------------------------------------------------------------------------------- builders and yardsticks
def _scaled(params, scale):
    params = [np.asarray(p, np.float32).copy() for p in params]
    params[4] *= np.float32(scale)
    params[5] *= np.float32(scale)
    return params


def q_inputs(fam, k, seed=None):
    """(steps, params) of family fam at K26 shape k: the small sweeps' builders at the big shape (LSIQ's and H's with the
    critic's output layer scaled, H's with its own columns).  Not cached when a seed is given."""
    in_dim, A, B, n_policy = K26_SHAPES[k]
    seed = SEEDS[fam][k] if seed is None else seed
    if fam == "h":
        return H.h_inputs(in_dim, A, B, n_policy, seed, updates=UPDATES)
    steps, params = R.case_inputs(in_dim, A, B, seed=seed, updates=UPDATES)
    return steps, (_scaled(params, L.W3_SCALE) if fam == "lsiq" else params)


def q_steps(fam, cfg, steps, n_policy):
    """The steps as the config takes them (lsiq_restate.case_steps, lsiq_h_restate.case_steps)."""
    return L.case_steps(cfg, steps, n_policy) if fam == "lsiq" else H.case_steps(cfg, steps) if fam == "h" else steps


def q_run(fam, cfg, params, steps, n_policy, dtype=torch.float64):
    """(state, out [UPDATES, 16], the sides of every update or None) of one run."""
    if fam == "iq":
        return R.run(params, cfg, steps, n_policy, dtype) + (None,)
    mod = L if fam == "lsiq" else H
    state, out, margins = mod.run(params, cfg, q_steps(fam, cfg, steps, n_policy), n_policy, dtype, check=True)
    return state, out, [sides_of(m) for m in margins]


def sides_of(m):
    """What a float32 run must share with the float64 run, row by row: of lsiq_restate's and lsiq_h_restate's margins the
    side of every clip and of Huber's kink, and the branch of the running maximum's update."""
    out = {k: m[k] for k in ("clip_side", "exp_side", "target_side") if k in m and m.get("clip", True)}
    if m["huber"]:
        out["huber_side"] = m["huber_side"]
    if "cost_side" in m:
        out["reward_side"], out["reward_abs_side"] = m["cost_side"]
    if "branch" in m:
        out["branch"] = m["branch"]
    return out


def assert_same_sides(s64, s32, who=""):
    """The big table's replacement of the small tables' absolute margins (MARGIN, MAX_MARGIN), which cannot hold over
    4096 rows: the float32 and the float64 run take the same side at every update, on every row."""
    if s64 is None:
        return
    assert len(s64) == len(s32) == UPDATES
    for i, (a, b) in enumerate(zip(s64, s32)):
        assert set(a) == set(b), (who, i, set(a), set(b))
        for key in a:
            same = a[key] == b[key] if isinstance(a[key], str) else np.array_equal(a[key], b[key])
            assert same, (who, i, key, "the float32 run takes another side than float64")


_CACHE = {}


def q_case_inputs(fam, k):
    if ("qin", fam, k) not in _CACHE:
        _CACHE[("qin", fam, k)] = q_inputs(fam, k)
    return _CACHE[("qin", fam, k)]


def q_yardstick(case):
    """(float64 state, float64 out, float32 state, float32 out) of K26 case (k, j), computed once and shared; callers
    leave them unchanged.  For the LSIQ families both runs' sides are compared here."""
    if ("q", case) not in _CACHE:
        k, j = case
        fam, cfg = Q_CONFIGS[j]
        steps, params = q_case_inputs(fam, k)
        n_policy = K26_SHAPES[k][3]
        s64, o64, sd64 = q_run(fam, cfg, params, steps, n_policy)
        s32, o32, sd32 = q_run(fam, cfg, params, steps, n_policy, torch.float32)
        assert_same_sides(sd64, sd32, q_case_id(case))
        _CACHE[("q", case)] = (s64, o64, s32, o32)
    return _CACHE[("q", case)]


def pi_inputs(k, seed=None):
    """iq_pi_restate.case_inputs at K27 shape k with a second critic's parameters (lsiq_h_restate.actor_case's rule)."""
    in_dim, A, Bp = K27_SHAPES[k]
    seed = SEEDS["pi"][k] if seed is None else seed
    case = P.case_inputs(in_dim, A, Bp, seed=seed, updates=UPDATES)
    case["hparams"] = linear_params([(in_dim + A, 512), (512, 256), (256, 1)], H.H_SEED_OFFSET + seed)
    return case


def pi_run(cfg, two, case, dtype=torch.float64):
    """(state, out [UPDATES, 4], [(a_new, log_prob) per update]) with one critic or two."""
    return H.run_actor(case, cfg, dtype) if two else P.run(case, cfg, dtype)


def pi_case_inputs(k):
    if ("pin", k) not in _CACHE:
        _CACHE[("pin", k)] = pi_inputs(k)
    return _CACHE[("pin", k)]


def pi_yardstick(case):
    """(float64 state, out, acts, float32 state, out, acts) of K27 case (k, j), computed once and shared."""
    if ("pi", case) not in _CACHE:
        k, j = case
        cfg, two = PI_CONFIGS[j]
        inp = pi_case_inputs(k)
        _CACHE[("pi", case)] = pi_run(cfg, two, inp) + pi_run(cfg, two, inp, torch.float32)
    return _CACHE[("pi", case)]


def alpha_case(n):
    """The alpha update's inputs at n rows (tests/test_gpu_iq_pi.py's, two updates): (log-probabilities per update,
    target entropy, learning rate, initial alpha)."""
    rng = np.random.default_rng(50 + n)
    return [(rng.standard_normal(n) * 2 - 1).astype(np.float32) for _ in range(UPDATES)], -5.0, 3e-4, 0.2


# ---------------------------------------------------------------------------------------------- the comparison
def q_errors(got, out, yard):
    """The rule of tests/test_gpu_iq_q.py, test_gpu_lsiq_q.py and test_gpu_lsiq_h.py on one K26 case, as
    [(name, error, tolerance)]: got = dict(params, target, exp_avg, exp_avg_sq: flat float64 arrays; max: the running
    maximum or None) and out [UPDATES, 16] of the run under test, yard = q_yardstick's tuple.  Parameters and target
    |got - f64| <= max(TOL, 4 |f32 - f64|) per tensor group, the moments the same relative to the largest entry, the
    scalars TOL relative from 1 upwards or 4 x their spread (the worst ratio is returned, NaN where float64 has NaN on
    both sides), the running maximum relative to its size."""
    ref, ref_out, f32, f32_out = yard
    res = []
    for key in ("params", "target"):
        r = cat(ref[key])
        res.append((key, float(np.abs(got[key] - r).max()), max(TOL, 4 * float(np.abs(cat(f32[key]) - r).max()))))
    for key in ("exp_avg", "exp_avg_sq"):
        r = cat(ref[key])
        scale = max(float(np.abs(r).max()), 1e-300)
        res.append((key, float(np.abs(got[key] - r).max()) / scale, max(TOL, 4 * float(np.abs(cat(f32[key]) - r).max()) / scale)))
    spread = np.abs(f32_out - ref_out)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(ref_out)), 4 * np.where(np.isnan(spread), 0.0, spread))
    if not np.array_equal(np.isnan(out), np.isnan(ref_out)):
        res.append(("scalars", np.inf, 1.0))
    else:
        ratio = np.where(np.isnan(ref_out), 0.0, np.abs(out - ref_out) / tol)
        res.append(("scalars", float(ratio.max()), 1.0))
    if ref.get("max") is not None:
        size = abs(ref["max"])
        res.append(("max", abs(float(got["max"]) - ref["max"]) / size, max(TOL, 4 * abs(f32["max"] - ref["max"]) / size)))
    return res


def q_state_of(state):
    """q_errors' `got` from a restatement's state."""
    return dict({k: cat(state[k]) for k in ("params", "target", "exp_avg", "exp_avg_sq")}, max=state.get("max"))


def pi_errors(got, out, acts, yard):
    """The rule of tests/test_gpu_iq_pi.py and test_gpu_lsiq_h_actor.py on one K27 case, as [(name, error, tolerance)]:
    got = dict(params, exp_avg flat float64), out [UPDATES, 4], acts = (a_new, log_prob) of the last update."""
    ref, ref_out, ref_acts, f32 = yard[:4]
    r = cat(ref["policy"]["params"])
    res = [("params", float(np.abs(got["params"] - r).max()),
            max(TOL, 4 * float(np.abs(cat(f32["policy"]["params"]) - r).max())))]
    r = cat(ref["policy"]["exp_avg"])
    res.append(("exp_avg", float(np.abs(got["exp_avg"] - r).max()) / max(float(np.abs(r).max()), 1e-300), TOL))
    res.append(("scalars", float((np.abs(out - ref_out) / np.maximum(1.0, np.abs(ref_out))).max()), TOL))
    a_ref, lp_ref = ref_acts[-1]
    res.append(("a_new", float(np.abs(acts[0] - a_ref).max()), TOL))
    res.append(("log_prob", float(np.abs(acts[1] - lp_ref).max()), TOL * max(1.0, float(np.abs(lp_ref).max()))))
    return res


def pi_state_of(state):
    return dict(params=cat(state["policy"]["params"]), exp_avg=cat(state["policy"]["exp_avg"]))


def alpha_errors(got, want):
    """tests/test_gpu_iq_pi.py's rule on the [3] block: log_alpha absolutely, the two moments relative to their size."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return [("log_alpha", abs(got[0] - want[0]), TOL)] + \
        [(n, abs(got[i] - want[i]) / abs(want[i]), TOL) for i, n in ((1, "exp_avg"), (2, "exp_avg_sq"))]


def worst(errors):
    """The largest error / tolerance of a list of (name, error, tolerance)."""
    return max(e / t for _, e, t in errors)


# ---------------------------------------------------------------------------------------------- the wrong readings
def misread_row(steps, dst, src):
    """The steps with row dst overwritten by row src in every field that has one: one misread row."""
    out = []
    for s in steps:
        s = {k: np.array(v, copy=True) for k, v in s.items()}
        for v in s.values():
            if len(v) > max(dst, src):
                v[dst] = v[src]
        out.append(s)
    return out


def first_trip_only(lps, target_entropy):
    """The log-probabilities of an alpha update whose sum of log_prob + target_entropy takes the first THREADS rows only
    (and is still divided by n): the other rows' terms are zero."""
    rest = lambda lp: np.full(max(0, len(lp) - THREADS), -target_entropy, np.float32)
    return [np.concatenate([lp[:THREADS], rest(lp)]) for lp in lps]
