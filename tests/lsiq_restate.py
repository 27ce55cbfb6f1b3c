"""The yardstick of K26's third algorithm (oly_iq_q_update with OLY_IQ_ALGO_LSIQ, csrc/k26_iq_critic.hip): LSIQ._lossQ
(imitation_lib/imitation/lsiq.py:9-195) restated with torch autograd, torch's own clip / mse_loss / huber_loss and
torch.optim.Adam, in float64 (the yardstick) or float32 (what the reference runs).  Everything LSIQ inherits from IQ_SAC
(the network, the Standardizers pass by pass, Adam, the target update, the logged scalars) is tests/iq_restate.py's SoftQ,
by import.  No tests here: tests/test_lsiq_cpu.py holds this file against the fixtures of tests/golden/gen_lsiq_q_update.py
(which executes the reference's own lines), tests/test_gpu_lsiq_q.py runs the kernel against it.

The wrong readings (`wrong=`), each a plausible misreading the fixtures must tell from the reference:
  unclipped_target   y takes next_v itself although target_clipping is on
  clip_grad_through  without a target the gradient passes the clipped rows too (a straight-through clip)
  stats_all_rows     sqil_like / value_plcy: the critic's Standardizer takes B rows in the value pass, the policy's rows
                     and then the expert rows' observations beside the policy's actions, although getV ran on n_policy
  fix_grad_to_y      the fix loss's gradient reaches y as well (as if Q_max were compared with reward + y.detach())
  absorbing_rmin     sqil_like / value: the expert rows' r_min gets the absorbing treatment too
and iq_restate's one_stats / shared_target, which SoftQ.forward carries.

The margins: a float32 run may take another side of the clip or of Huber's kink than float64 where next_v or a residual
sits within rounding of it, and then no tolerance holds.  With check=True (float64 only) every update records how far each
row's next_v is from both bounds and each Huber residual from 1, and how many rows lie below, inside and above the clip
range and on each Huber branch; assert_margins holds them to MARGIN and, from B = 16, to two rows of every kind.

The same holds for a relu: measured on the CPU, config 23 at its shape had one layer-2 pre-activation of the first pass at
2.0e-8 in float64 (a sum of 512 products with partial sums near 1, whose float32 rounding is about 1e-7 per step), so its
side depends on the order of a float32 sum; that config's gradients nearly cancel (plcy_loss_mode off) and the flip moved
a parameter by two Adam steps.  Every update also records the smallest |pre-activation| of its passes and assert_margins
holds it to RELU_MARGIN = 1e-6, ten times that rounding."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import iq_restate as R
from iq_restate import SoftQ, update_target

IQ_LIKE_MODES = ("value", "value_expert", "value_policy", "q_old_policy", "value_q_old_policy", "off")
SQIL_LIKE_MODES = ("value", "value_plcy", "q_old_policy")
MARGIN, RELU_MARGIN = 1e-3, 1e-6

LCfg = namedtuple("LCfg", "type exp_mode exp_loss clip q_min q_max mode reg treat use_target standardizer gamma alpha "
                          "reg_mult lr tau wd update_target adam_eps",
                  defaults=("iq_like", "fix", "MSE", True, -1.0, 1.0, "value", "exp_and_plcy", False, True, True, 0.99,
                            float(np.exp(np.float32(np.log(1e-3)))), 0.5, 3e-4, 0.005, 0.0, True, 1e-8))


def has_v(cfg):
    """Whether the update runs the pass Q(obs | a_pi): always for iq_like (getV(obs) runs in every mode, lsiq.py:72), for
    sqil_like unless plcy_loss_mode is q_old_policy."""
    return cfg.type == "iq_like" or cfg.mode != "q_old_policy"


def value_rows(cfg, B, n_policy):
    """The rows of the pass on (obs | a_pi): the policy's alone for sqil_like / value_plcy (lsiq.py:167)."""
    return n_policy if (cfg.type == "sqil_like" and cfg.mode == "value_plcy") else B


def as_iq(cfg):
    """The IQ configuration an LSIQ one coincides with (iq_like, bootstrap, no clipping), or None."""
    if cfg.type != "iq_like" or cfg.exp_mode != "bootstrap" or cfg.clip or cfg.mode not in R.IQ_MODES:
        return None
    return R.Cfg(algo="iq", mode=cfg.mode, reg=cfg.reg, treat=cfg.treat, use_target=cfg.use_target,
                 standardizer=cfg.standardizer, gamma=cfg.gamma, alpha=cfg.alpha, reg_mult=cfg.reg_mult, lr=cfg.lr,
                 tau=cfg.tau, wd=cfg.wd, update_target=cfg.update_target, adam_eps=cfg.adam_eps)


class LSIQSoftQ(SoftQ):
    """SoftQ with LSIQ's update.  check: record the margins of every update (float64)."""

    def __init__(self, params, cfg, dtype=torch.float64, wrong=None, target=None, check=False):
        super().__init__(params, cfg, dtype, wrong, target)
        self.check, self.margins, self._relu = check, [], []

    def _net(self, ps, z):
        """SoftQ._net's lines; with check the smallest |pre-activation| of the pass is recorded."""
        if not self.check:
            return super()._net(ps, z)
        z1 = z @ ps[0].T + ps[1]
        z2 = torch.relu(z1) @ ps[2].T + ps[3]
        self._relu.append(min(float(z1.detach().abs().min()), float(z2.detach().abs().min())))
        return torch.relu(z2) @ ps[4].T + ps[5]

    def _point(self, value, target):
        """Q_exp_loss between two columns: F.mse_loss / torch.mean(torch.square(.)) or F.huber_loss (delta 1, mean)."""
        if self.cfg.exp_loss == "MSE":
            return F.mse_loss(value, target)
        if self.check:
            self._huber.append((value - target).detach().double().reshape(-1))
        return F.huber_loss(value, target)

    def update(self, obs, act, next_obs, absorbing, a_next, logp_next, a_pi, logp_pi, n_policy):
        """One update_Q_function and _update_all_targets; returns the 16 scalars of oly_iq_q_update as float64.  For
        sqil_like / value_plcy a_pi and logp_pi hold the policy's rows (more are ignored)."""
        c, dt, wrong = self.cfg, self.dtype, self.wrong
        B = len(obs)
        self._huber, self._relu = [], []
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        exp = torch.arange(B) >= n_policy
        nv_rows = value_rows(c, B, n_policy)
        x0, x1 = np.concatenate([obs, act], 1), np.concatenate([next_obs, a_next], 1)
        x2 = np.concatenate([obs[:nv_rows], np.asarray(a_pi)[:nv_rows]], 1) if has_v(c) else None
        ab = t(absorbing).reshape(B, 1)
        alpha, gamma = t(c.alpha), t(c.gamma)
        Q = self.forward(x0)
        if c.use_target:
            with torch.no_grad():
                nq = self.forward(x1, target=True)
        else:
            nq = self.forward(x1)
        next_v = nq - alpha * t(logp_next).reshape(B, 1)
        if c.clip and wrong != "unclipped_target":
            clipped = torch.clip(next_v, c.q_min, c.q_max)
            if wrong == "clip_grad_through":
                clipped = next_v + (clipped - next_v).detach()
            y = (1 - ab) * gamma * clipped
        else:
            y = (1 - ab) * gamma * next_v
        reward = Q - y
        V = None
        if x2 is not None:
            if wrong == "stats_all_rows" and nv_rows < B and self.stand is not None:
                extra = np.concatenate([obs[nv_rows:], np.asarray(a_pi)[:B - nv_rows]], 1)
                V = self.forward(np.concatenate([x2, extra]))[:nv_rows]
            else:
                V = self.forward(x2)
            V = V - alpha * t(logp_pi).reshape(-1, 1)[:nv_rows]
        q_max = torch.ones_like(Q[exp]) * c.q_max
        fix_in = Q[exp]
        out = np.zeros(16)
        if c.type == "iq_like":
            if c.exp_mode == "bootstrap":
                loss1 = -reward[exp].mean()
            else:
                loss1 = self._point(fix_in, q_max)
            value = V - y
            loss2 = {"value": lambda: value.mean(), "value_expert": lambda: value[exp].mean(),
                     "value_policy": lambda: value[~exp].mean(), "q_old_policy": lambda: reward[~exp].mean(),
                     "value_q_old_policy": lambda: reward[~exp].mean() + value.mean(),
                     "off": lambda: torch.zeros((), dtype=dt)}[c.mode]()
            ra = ab if c.treat else torch.zeros_like(ab)
            w = (1 - ra) * c.reg_mult + ra * (1.0 - gamma) * c.reg_mult
            chi = w * torch.square(reward)
            chi2 = {"exp_and_plcy": lambda: chi.mean(), "exp": lambda: chi[exp].mean(), "plcy": lambda: chi[~exp].mean(),
                    "off": lambda: torch.zeros((), dtype=dt)}[c.reg]()
            loss = loss1 + loss2 + chi2
            out[0], out[1], out[2] = (float(v.detach()) for v in (loss1, loss2, chi2))
            out[3] = float(V.detach().double().mean())
        else:
            if c.treat:
                r_max = (1 - ab) * (1 / c.reg_mult) + ab * (1 / (1 - gamma)) * (1 / c.reg_mult)
                r_min = (1 - ab) * (-(1 / c.reg_mult)) + ab * (1 / (1 - gamma)) * (-(1 / c.reg_mult))
            else:
                r_max = torch.ones_like(ab) * (1 / c.reg_mult)
                r_min = torch.ones_like(ab) * (-(1 / c.reg_mult))
            r_min_all = r_min
            r_max, r_min = r_max[exp], r_min[~exp]
            if c.exp_mode == "bootstrap":
                loss1 = self._point(Q[exp], r_max + y[exp])
            else:
                loss1 = self._point(fix_in, q_max)
            if c.mode == "value":
                assert 2 * n_policy == B, "sqil_like / value needs as many policy rows as expert rows (lsiq.py:165)"
                value, target = V, y
                rest = r_min_all[exp] if wrong == "absorbing_rmin" else torch.ones_like(r_min) * (-(1 / c.reg_mult))
                r_min = torch.concat([r_min, rest])
            elif c.mode == "value_plcy":
                value, target = V, y[~exp]
            else:
                value, target = Q[~exp], y[~exp]
            loss2 = self._point(value, r_min + target)
            loss = loss1 + loss2
            out[0], out[1] = float(loss1.detach()), float(loss2.detach())
        if wrong == "fix_grad_to_y" and c.exp_mode == "fix" and not c.use_target:
            # the misreading: d(loss1)/dy = -d(loss1)/dQ on the expert rows
            g = torch.autograd.grad(loss1, Q, retain_graph=True)[0].detach()
            loss = loss - (g * y).sum()
        self.opt.zero_grad()
        loss.backward()
        out[15] = float(torch.cat([p.grad.reshape(-1) for p in self.p]).double().norm())
        self.opt.step()
        with torch.no_grad():
            d = lambda v: v.detach().double()
            Qd, yd, rd, a_ = d(Q), d(y), d(reward), ab.reshape(-1) != 0
            out[4], out[5] = float(Qd[exp].mean()), float(torch.square(Qd[exp]).mean())
            out[6], out[7] = float(Qd[~exp].mean()), float(torch.square(Qd[~exp]).mean())
            out[8], out[9], out[10] = float(rd.mean()), float(rd[exp].mean()), float(rd[~exp].mean())
            out[11], out[12] = float(yd[exp].mean()), float(yd[~exp].mean())
            out[13] = float(Qd[exp][a_[exp]].mean()) if bool(a_[exp].any()) else np.nan
            out[14] = float(Qd[~exp][a_[~exp]].mean()) if bool(a_[~exp].any()) else np.nan
            if c.update_target:
                self.t = [update_target(c.tau, p.detach(), q) for p, q in zip(self.p, self.t)]
            if self.check:
                nv = d(next_v).reshape(-1).numpy()
                h = torch.cat(self._huber).numpy() if self._huber else np.zeros(0)
                self.margins.append(dict(
                    B=B, relu_margin=min(self._relu), clip=bool(c.clip), huber=c.exp_loss == "Huber" and len(h) > 0, next_v=np.sort(nv),
                    clip_margin=float(np.minimum(np.abs(nv - c.q_min), np.abs(nv - c.q_max)).min()),
                    below=int((nv < c.q_min).sum()), inside=int(((nv >= c.q_min) & (nv <= c.q_max)).sum()),
                    above=int((nv > c.q_max).sum()),
                    huber_margin=float(np.abs(np.abs(h) - 1.0).min()) if len(h) else np.inf,
                    quadratic=int((np.abs(h) < 1.0).sum()), linear=int((np.abs(h) >= 1.0).sum()),
                    # row by row, in the rows' order, for runs whose sides are compared between two precisions
                    # (tests/iq_big_shapes.py): -1 below, 0 inside, 1 above the clip range; Huber's quadratic branch
                    clip_side=(nv > c.q_max).astype(np.int8) - (nv < c.q_min).astype(np.int8), huber_side=np.abs(h) < 1.0))
        return out


def assert_margins(margins, who="", counts=True):
    """Every update of a case: no row within MARGIN of a clip bound or of Huber's kink; from B = 16 at least two rows
    below, inside and above the clip range and at least two residuals on each Huber branch (counts=False: a run whose
    batches are drawn at run time holds the distances only)."""
    for i, m in enumerate(margins):
        assert m["relu_margin"] >= RELU_MARGIN, (who, i, m["relu_margin"])
        if m["clip"]:
            assert m["clip_margin"] >= MARGIN, (who, i, m)
            if m["B"] >= 16 and counts:
                assert min(m["below"], m["inside"], m["above"]) >= 2, (who, i, m)
        if m["huber"]:
            assert m["huber_margin"] >= MARGIN, (who, i, m)
            if m["B"] >= 16 and counts:
                assert min(m["quadratic"], m["linear"]) >= 2, (who, i, m)


def run(params, cfg, steps, n_policy, dtype=torch.float64, wrong=None, check=False):
    """The updates of `steps` in order; returns (state after the last, out [updates, 16]) and, with check, the margins."""
    q = LSIQSoftQ(params, cfg, dtype, wrong, check=check)
    out = [q.update(n_policy=n_policy, **s) for s in steps]
    return (q.state(), np.asarray(out)) + ((q.margins,) if check else ())


# ---------------------------------------------------------------------------------------------- the GPU test's cases
# Measured on the CPU at (12,5,18,9) and (32,11,48,24): with nn.Linear's default initialisation Q and next_v span about
# +-0.15, so with the reference's default bounds +-1 no row would clip and Huber's |Q - Q_max| would sit on its kink at 1.
# The cases therefore scale the critic's output layer by W3_SCALE (Q spans about +-1.5) and take bounds near +-0.3, which
# are not symmetric so that a swapped pair shows.
#
# The learning rate is SWEEP_LR = 3e-5, a tenth of the fixtures' 3e-4.  Adam moves every weight by about lr per update, all
# of them downhill together, and with the scaled output layer that shifts every Q by about 1 per update at 3e-4 (measured:
# after one update all 18 rows of shape 1 lay below the range), so the later updates would run with no row inside the clip
# range.  At 3e-5 the rows stay spread over it for all three updates.  What pins the gradient does not depend on lr: the
# moments m and v (relative to their largest entry), the gradient's norm and the loss terms are held to TOL as before.
W3_SCALE, Q_MIN, Q_MAX, SWEEP_LR = 10.0, -0.25, 0.3, 3e-5
SHAPES, UPDATES, SWEEP_EPS, TOL, cat = R.SHAPES, R.UPDATES, R.SWEEP_EPS, R.TOL, R.cat
# the seed of each shape's inputs: the first from 10 upwards at which assert_margins holds for every config of the shape
SEEDS = {0: 10, 1: 26, 2: 101, 3: 137, 4: 16}


def sweep_configs():
    """Every expert loss (iq_like: bootstrap, fix/MSE, fix/Huber; sqil_like: bootstrap and fix x MSE and Huber) x clipping
    x target: 28 configs.  The iq_like ones walk through the six modes and the four regularizers, the sqil_like ones
    through the three modes; the Standardizers, treat_absorbing_states and a weight decay alternate over the list.
    sqil_like takes reg_mult 2 (rewards -+0.5, so that its residuals lie on both sides of Huber's kink)."""
    out = []
    experts = [("iq_like", "bootstrap", None), ("iq_like", "fix", "MSE"), ("iq_like", "fix", "Huber"),
               ("sqil_like", "bootstrap", "MSE"), ("sqil_like", "bootstrap", "Huber"), ("sqil_like", "fix", "MSE"),
               ("sqil_like", "fix", "Huber")]
    n_iq = n_sq = 0
    for clip in (True, False):
        for tgt in (True, False):
            for typ, em, el in experts:
                if typ == "iq_like":
                    mode, reg = IQ_LIKE_MODES[n_iq % 6], R.REG_MODES[(n_iq + n_iq // 6) % 4]
                    n_iq += 1
                    out.append(LCfg(type=typ, exp_mode=em, exp_loss=el, clip=clip, use_target=tgt, mode=mode, reg=reg))
                else:
                    mode = SQIL_LIKE_MODES[n_sq % 3]
                    n_sq += 1
                    out.append(LCfg(type=typ, exp_mode=em, exp_loss=el, clip=clip, use_target=tgt, mode=mode, reg_mult=2.0))
    return [c._replace(standardizer=(i // 3) % 2 == 0, treat=(i // 2) % 2 == 1, wd=1e-4 if i % 3 == 0 else 0.0, tau=0.05,
                       adam_eps=SWEEP_EPS, lr=SWEEP_LR, q_min=Q_MIN, q_max=Q_MAX) for i, c in enumerate(out)]


CONFIGS = sweep_configs()
UNBALANCED = 4            # (48,16,33,1): sqil_like / value is refused there and runs at shape 1 instead


def shape_of(j):
    k = j % len(SHAPES)
    c = CONFIGS[j]
    return 1 if (k == UNBALANCED and c.type == "sqil_like" and c.mode == "value") else k


def sweep(k):
    """[(number, config)] of the configs that run at shape k."""
    return [(j, c) for j, c in enumerate(CONFIGS) if shape_of(j) == k]


def cfg_id(c):
    return "-".join([c.type, c.exp_mode, str(c.exp_loss), "clip" if c.clip else "noclip", c.mode, c.reg,
                     "abs" if c.treat else "noabs", "tgt" if c.use_target else "notgt"]) + ("" if c.standardizer else "-nostd")


_CACHE = {}


def sweep_inputs(k):
    """(steps, params) of shape k: iq_restate.case_inputs from the shape's seed with the output layer scaled, rebuilt
    once; callers leave them unchanged.  At B = 2 the policy's row is absorbing and the expert's is not."""
    if ("in", k) not in _CACHE:
        in_dim, A, B, _ = SHAPES[k]
        steps, params = R.case_inputs(in_dim, A, B, seed=SEEDS[k], updates=UPDATES)
        if B == 2:
            for s in steps:
                s["absorbing"][:] = (1.0, 0.0)
        params = [np.asarray(p, np.float32).copy() for p in params]
        params[4] *= np.float32(W3_SCALE)
        params[5] *= np.float32(W3_SCALE)
        _CACHE[("in", k)] = (steps, params)
    return _CACHE[("in", k)]


def case_steps(cfg, steps, n_policy):
    """The steps as config cfg takes them: a_pi / logp_pi cut to the rows of its value pass."""
    n = value_rows(cfg, len(steps[0]["obs"]), n_policy)
    return [dict(s, a_pi=s["a_pi"][:n], logp_pi=s["logp_pi"][:n]) for s in steps]


def yardstick(k, j):
    """(float64 state, float64 out, float32 state, float32 out) of config j at shape k, computed once and shared; the
    float64 run's margins are asserted here, for every update."""
    if (k, j) not in _CACHE:
        steps, params = sweep_inputs(k)
        n_policy = SHAPES[k][3]
        st = case_steps(CONFIGS[j], steps, n_policy)
        s64, o64, margins = run(params, CONFIGS[j], st, n_policy, check=True)
        assert_margins(margins, (SHAPES[k], cfg_id(CONFIGS[j])))
        _CACHE[(k, j)] = (s64, o64) + run(params, CONFIGS[j], st, n_policy, torch.float32)
    return _CACHE[(k, j)]
