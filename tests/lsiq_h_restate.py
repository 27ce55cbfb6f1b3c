"""The yardstick of K26's fourth algorithm (oly_iq_q_update with OLY_IQ_ALGO_LSIQ_H, csrc/k26_iq_critic.hip):
update_H_function of LSIQ_H (imitation_lib/imitation/lsiq_h.py:57-102) and of LSIQ_HC
(imitation_lib/imitation/lsiq_hc.py:23-88) restated with torch autograd AS THE REFERENCE WRITES THEM: `absorbing` is the
[B] array update_H_function is handed (the unsqueeze in _lossQ_* rebinds a local), so every `(1 - absorbing) * ...`
against a [B, 1] term is a real [B, B] broadcast and mse_loss / huber_loss take H [B, 1] against a [B, B] target.  The
network, its Standardizers pass by pass, Adam and the target update are tests/iq_restate.py's SoftQ by import (through
lsiq_restate's LSIQSoftQ, whose _net records the relu margins), in float64 (the yardstick) or float32 (what the reference
runs).  The policy pass (a_next, logp_next) and, for LSIQ_HC, Q_target(obs | act) and Q_target(obs | a_pi) are inputs
here, as they are inputs of the kernel.  No tests here: tests/test_lsiq_h_cpu.py holds the closed form the kernel computes
against this file, tests/test_gpu_lsiq_h.py runs the kernel against it.

The wrong readings (`wrong=`), each a plausible misreading the cases must tell from the reference's lines:
  row_wise        absorbing taken as [B, 1]: target[i] = f(next_H[i], absorbing[i]), the plain row-wise TD target
  clip_old_max    the expert rows clipped with the running maximum from BEFORE this call's update of it
  h_step_clipped  H_step logged from the clipped -log pi
and, of CriticTwin (the whole update_Q_function of the two agents),
  target_after    LSIQ_HC reads the target Q critic AFTER this iteration's soft update of it
  h_before_q      update_H_function runs BEFORE the Q update.  H's update reads nothing the Q step writes, but its policy
                  passes then come first, and the policy's Standardizer (which every pass feeds) holds other rows at each
                  pass: the actions and log-probabilities of both updates change.  It shows only where the twin runs the
                  policy itself (not with `given` passes)

The margins: a float32 run may take another side of a clip, of Huber's kink, of a relu or of the running maximum's branch
than float64 where a value sits within rounding of it, and then no tolerance holds.  With check=True (float64 only) every
update records its distances and counts; assert_margins holds them (its docstring has the list)."""
import warnings
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import iq_restate as R
from iq_restate import update_target
from lsiq_restate import LSIQSoftQ

MARGIN, RELU_MARGIN, MAX_MARGIN = 1e-3, 1e-6, 1e-4

HCfg = namedtuple("HCfg", "cost loss clip_expert tau_up tau_down q_min q_max standardizer gamma alpha reg_mult lr tau wd "
                          "update_target adam_eps use_target",
                  defaults=(False, "MSE", True, 1e-2, 1e-4, -1.0, 1.0, True, 0.99, float(np.exp(np.float32(np.log(1e-3)))),
                            0.5, 3e-4, 0.005, 0.0, True, 1e-8, True))


def closed_form(H, t0, t1, n1, kind):
    """What the kernel computes in place of the [B, B] broadcast: with n0 = B - n1 the loss
    sum_i (n0 l(H_i - t0_i) + n1 l(H_i - t1_i)) / B^2 and its gradient with respect to H, l the square ("MSE") or Huber's
    delta-1 loss.  H, t0, t1 [B] float64 arrays; returns (loss, dL/dH [B])."""
    H, t0, t1 = (np.asarray(a, np.float64).reshape(-1) for a in (H, t0, t1))
    B = len(H)
    n0 = B - n1

    def point(d):
        if kind == "Huber":
            a = np.abs(d)
            return np.where(a < 1.0, 0.5 * d * d, a - 0.5), np.clip(d, -1.0, 1.0)
        return d * d, 2.0 * d
    l0, g0 = point(H - t0)
    l1, g1 = point(H - t1)
    return float((n0 * l0 + n1 * l1).sum() / B ** 2), (n0 * g0 + n1 * g1) / B ** 2


class HCritic(LSIQSoftQ):
    """The H critic, its target, Adam, the two Standardizers and the running maximum `M` (None until the first update
    with clip_expert).  check: record the margins of every update (float64)."""

    def __init__(self, params, cfg, dtype=torch.float64, wrong=None, target=None, check=False):
        super().__init__(params, cfg, dtype, wrong, target, check)
        self.M = None

    def update(self, obs, act, next_obs, absorbing, a_next, logp_next, n_policy, q_t=None, v_t=None, **unused):
        """One update_H_function and H's share of _update_all_targets; returns the 16 slots of oly_iq_q_update as float64
        (_abi.LSIQ_H_TAGS, then zeros)."""
        c, dt, wrong = self.cfg, self.dtype, self.wrong
        B = len(obs)
        self._huber, self._relu = [], []
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        is_expert = torch.arange(B) >= n_policy
        absorbing = t(absorbing)                                    # [B]
        if wrong == "row_wise":
            absorbing = absorbing.reshape(B, 1)
        alpha, gamma = t(c.alpha), t(c.gamma)
        m = dict(B=B, n_policy=n_policy)
        H = self.forward(np.concatenate([obs, act], 1))
        log_pi = t(logp_next)
        neg_log_pi = -log_pi
        if c.clip_expert:                                           # lsiq_h.py:64-75
            old = self.M
            curr = torch.max(neg_log_pi[~is_expert])
            if self.M is None:
                self.M = curr
            elif curr > self.M:
                m["branch"], m["max_margin"] = "up", float(abs(curr - self.M))
                self.M = (1 - c.tau_up) * self.M + c.tau_up * curr
            else:
                m["branch"], m["max_margin"] = "down", float(abs(curr - self.M))
                self.M = (1 - c.tau_down) * self.M + c.tau_down * curr
            bound = old if (wrong == "clip_old_max" and old is not None) else self.M
            e = neg_log_pi[is_expert].detach().double().numpy()
            m["exp_clipped"], m["exp_free"] = int((e < float(bound)).sum()), int((e > float(bound)).sum())
            m["exp_margin"] = float(np.abs(e - float(bound)).min())
            m["exp_side"] = e < float(bound)        # row by row, for runs compared between two precisions (iq_big_shapes)
            neg_log_pi[is_expert] = torch.clip(neg_log_pi[is_expert], bound, 100000)
        with torch.no_grad():
            next_H = self.forward(np.concatenate([next_obs, a_next], 1), target=True) + alpha * torch.unsqueeze(neg_log_pi, 1)
            if c.cost:                                              # lsiq_hc.py:29-38, 58-62
                Q_plcy, V_plcy = t(q_t).reshape(B, 1), t(v_t).reshape(B, 1)
                y = (1 - absorbing) * gamma * torch.clip(V_plcy, c.q_min, c.q_max)
                reward_non_abs = torch.square(torch.clip(Q_plcy - y, -1 / c.reg_mult, 1 / c.reg_mult))
                reward_abs = torch.square(torch.clip(Q_plcy - y, c.q_min, c.q_max))
                squared = (1 - absorbing) * c.reg_mult * reward_non_abs + absorbing * (1.0 - gamma) * c.reg_mult * reward_abs
                raw = squared + (1 - absorbing) * gamma * next_H
                Q2_max = (1.0 / c.reg_mult) ** 2 / (1 - gamma)
                lo, hi = -1000, float(Q2_max + 100)
                if self.check:
                    x, side = (Q_plcy - y).double().numpy(), lambda v, a, b: (v > b).astype(np.int8) - (v < a).astype(np.int8)
                    m["cost_side"] = (side(x, -1 / c.reg_mult, 1 / c.reg_mult), side(x, c.q_min, c.q_max))   # of this run's y
                    qd, vd, r = Q_plcy.double().reshape(-1).numpy(), V_plcy.double().reshape(-1).numpy(), 1 / c.reg_mult
                    d0 = qd - c.gamma * np.clip(vd, c.q_min, c.q_max)
                    side = lambda v, a, b: (int(((v < a) | (v > b)).sum()), int(((v >= a) & (v <= b)).sum()))
                    m["cost"] = dict(v=side(vd, c.q_min, c.q_max), non_abs=side(d0, -r, r), abs=side(qd, c.q_min, c.q_max))
                    m["cost_margin"] = float(min(np.abs(vd - c.q_min).min(), np.abs(vd - c.q_max).min(),
                                                 np.abs(np.abs(d0) - r).min(), np.abs(qd - c.q_min).min(),
                                                 np.abs(qd - c.q_max).min()))
            else:                                                   # lsiq_h.py:79-82
                raw = (1 - absorbing) * gamma * next_H
                lo, hi = -10000, 1000
            target_H = torch.clip(raw, lo, hi)
        with warnings.catch_warnings():                             # torch warns of the broadcast the reference relies on
            warnings.simplefilter("ignore")
            loss_H = F.huber_loss(H, target_H) if c.loss == "Huber" else F.mse_loss(H, target_H)
        self.opt.zero_grad()
        loss_H.backward()
        out = np.zeros(16)
        out[7] = float(torch.cat([p.grad.reshape(-1) for p in self.p]).double().norm())
        self.opt.step()
        with torch.no_grad():
            Hd = H.detach().double().reshape(-1)
            step = (neg_log_pi if wrong == "h_step_clipped" else -log_pi).double()     # np.mean(-log_pi), lsiq_h.py:98-100
            out[0] = float(loss_H.detach())
            out[1], out[2], out[3] = float(Hd.mean()), float(Hd[~is_expert].mean()), float(Hd[is_expert].mean())
            out[4], out[5], out[6] = float(step.mean()), float(step[~is_expert].mean()), float(step[is_expert].mean())
            out[8] = float(self.M) if c.clip_expert else 0.0
            if c.update_target:
                self.t = [update_target(c.tau, p.detach(), q) for p, q in zip(self.p, self.t)]
            if self.check:
                rw, td = raw.double().numpy(), target_H.double().numpy()
                res = (Hd.reshape(-1, 1).numpy() - td).reshape(-1)
                ab = np.asarray(absorbing.reshape(-1)) != 0
                m.update(relu_margin=min(self._relu), clip_margin=float(np.minimum(np.abs(rw - lo), np.abs(rw - hi)).min()),
                         above=int((rw.max(axis=-1) > hi).sum()), inside=int((rw.max(axis=-1) <= hi).sum()),
                         huber=c.loss == "Huber", huber_margin=float(np.abs(np.abs(res) - 1.0).min()),
                         quadratic=int((np.abs(res) < 1.0).sum()), linear=int((np.abs(res) >= 1.0).sum()),
                         abs_policy=int(ab[:n_policy].sum()), abs_expert=int(ab[n_policy:].sum()),
                         target_side=(rw > hi).astype(np.int8) - (rw < lo).astype(np.int8), huber_side=np.abs(res) < 1.0)
                self.margins.append(m)
        return out


def assert_margins(margins, who="", clipped_targets=False, counts=True):
    """Every update of a case (float64): no unclipped target within MARGIN of a clip bound, no Huber residual within MARGIN
    of its kink, no pre-activation within RELU_MARGIN of a relu's, no expert row's -log pi within MARGIN of the running
    maximum, |cur - M| > MAX_MARGIN at every update of the maximum, and for LSIQ_HC no V, Q or Q - y within MARGIN of the
    bound it is clipped to.  From B = 16: at least two absorbing and two non-absorbing rows in each half of the batch that
    has four rows or more (the shape with n_policy = 1 has no such policy half); at least two expert rows clipped by the
    maximum and two not; at least two residuals of the [B, B] matrix on each Huber branch; for LSIQ_HC at least two rows
    clipped and two unclipped at each of its three clips; both branches of the maximum's update within the case's
    updates.  clipped_targets: at least two rows' targets above the upper clip bound and two inside.  counts=False: a
    run whose policy passes are the policy's own holds the distances only."""
    branches = set()
    for i, m in enumerate(margins):
        big = m["B"] >= 16 and counts
        assert m["relu_margin"] >= RELU_MARGIN, (who, i, m["relu_margin"])
        assert m["clip_margin"] >= MARGIN, (who, i, m["clip_margin"])
        if clipped_targets:
            assert min(m["above"], m["inside"]) >= 2, (who, i, m["above"], m["inside"])
        if m["huber"]:
            assert m["huber_margin"] >= MARGIN, (who, i, m["huber_margin"])
            if big:
                assert min(m["quadratic"], m["linear"]) >= 2, (who, i, m["quadratic"], m["linear"])
        if big:
            for n, a in ((m["n_policy"], m["abs_policy"]), (m["B"] - m["n_policy"], m["abs_expert"])):
                if n >= 4:
                    assert a >= 2 and n - a >= 2, (who, i, n, a)
        if "exp_margin" in m:
            assert m["exp_margin"] >= MARGIN, (who, i, m["exp_margin"])
            if big:
                assert min(m["exp_clipped"], m["exp_free"]) >= 2, (who, i, m["exp_clipped"], m["exp_free"])
        if "branch" in m:
            branches.add(m["branch"])
            assert m["max_margin"] > MAX_MARGIN, (who, i, m["max_margin"])
        if "cost" in m:
            assert m["cost_margin"] >= MARGIN, (who, i, m["cost_margin"])
            if big:
                for k, (out, inside) in m["cost"].items():
                    assert min(out, inside) >= 2, (who, i, k, out, inside)
    if counts and margins and margins[0]["B"] >= 16 and any("exp_margin" in m for m in margins):
        assert branches == {"up", "down"}, (who, branches)


def run(params, cfg, steps, n_policy, dtype=torch.float64, wrong=None, check=False):
    """The updates of `steps` in order; returns (state after the last with "max" = the running maximum or None,
    out [updates, 16]) and, with check, the margins."""
    h = HCritic(params, cfg, dtype, wrong, check=check)
    out = [h.update(n_policy=n_policy, **s) for s in steps]
    state = dict(h.state(), max=None if h.M is None else float(h.M))
    return (state, np.asarray(out)) + ((h.margins,) if check else ())


# ---------------------------------------------------------------------------------------------- the GPU test's cases
# What the inputs are made for, each measured on the CPU with this file alone:
#  * H's output layer is scaled by W3_SCALE = 10 (live and target alike) as tests/lsiq_restate.py scales Q's: with
#    nn.Linear's default initialisation H and the targets span about +-0.15 and every Huber residual is quadratic; scaled,
#    the residuals of the [B, B] matrix lie on both sides of 1.  SWEEP_LR = 3e-5 keeps them there for three updates (that
#    file has the measurement: at 3e-4 Adam shifts every output by about 1 per update through the scaled layer).
#  * The expert rows' log-probabilities are drawn EXPERT_SHIFT = 3 lower than the policy's rows', so that about half of
#    the expert rows' -log pi exceed the maximum of the policy's rows (the maximum of nine draws lies about 1.5 deviations
#    = 3 above their mean) and half are clipped by it.  An expert's actions being less likely under the policy than the
#    policy's own is also the regime the clip exists for.
#  * The running maximum's rates are 0.3 (up) and 0.1 (down), not the reference's defaults 1e-2 and 1e-4: with those a
#    maximum read before its update differs from the updated one by less than the tolerance, and the wrong reading
#    clip_old_max could not be told from the right one.
#  * LSIQ_HC: reg_mult 2 (the reward's clip at +-0.5), bounds Q_MIN = -0.4, Q_MAX = 0.6 (not symmetric, so that a swapped
#    pair shows), and q_t, v_t drawn with deviation 0.6: Q - y, V and Q then lie on both sides of every bound.  At default
#    initialisation Q_target spans +-0.15 and none of the three clips would act.
#  * alpha is SWEEP_ALPHA = 0.2, not the 1e-3 of the other sweeps: the entropy enters the target as alpha (-log pi) with
#    -log pi near 5, which at 1e-3 is 0.005 against targets of order 1, and then neither the expert clip nor a maximum read
#    too early moves anything by more than a few tolerances (measured: clip_old_max missed by 3.4 tolerances at 1e-3).
#  * About 35 % of the rows are absorbing, so that both halves of a batch hold rows of both kinds.
#  * CLIPPED: alpha 300 (LSIQ_H) and 30 (LSIQ_HC) put gamma next_H = gamma (H' + alpha neg) on both sides of the upper
#    clip bound of the target (1000, and 0.25 / 0.01 + 100 = 125); at alpha = 1e-3 no target comes near either bound.  The
#    lower bounds (-10000, -1000) are not reached with -log pi mostly positive.
W3_SCALE, SWEEP_LR, EXPERT_SHIFT, TAU_UP, TAU_DOWN, SWEEP_ALPHA = 10.0, 3e-5, 3.0, 0.3, 0.1, 0.2
HC_REG_MULT, Q_MIN, Q_MAX, QT_DEV, ABSORBING_FRAC = 2.0, -0.4, 0.6, 0.6, 0.35
SHAPES, UPDATES, SWEEP_EPS, TOL, cat = R.SHAPES, R.UPDATES, R.SWEEP_EPS, R.TOL, R.cat
# the seed of each shape's inputs: the first from 10 upwards at which assert_margins holds for every config of the shape
SEEDS = {0: 10, 1: 58, 2: 14, 3: 79, 4: 75}
CLIPPED_SEED = 58


def sweep_configs():
    """Both classes x MSE / Huber x expert clip on / off x Standardizers on / off: 16 configs, a weight decay on every
    third."""
    out = []
    for cost in (False, True):
        for loss in ("MSE", "Huber"):
            for clip in (True, False):
                for stand in (True, False):
                    out.append(HCfg(cost=cost, loss=loss, clip_expert=clip, standardizer=stand))
    return [c._replace(tau_up=TAU_UP, tau_down=TAU_DOWN, q_min=Q_MIN, q_max=Q_MAX, reg_mult=HC_REG_MULT if c.cost else 0.5,
                       lr=SWEEP_LR, alpha=SWEEP_ALPHA, tau=0.05, adam_eps=SWEEP_EPS, wd=1e-4 if i % 3 == 0 else 0.0)
            for i, c in enumerate(out)]


CONFIGS = sweep_configs()
CLIPPED = (CONFIGS[0]._replace(alpha=300.0), CONFIGS[12]._replace(alpha=30.0))


def cfg_id(c):
    return "-".join(["hc" if c.cost else "h", c.loss, "clip" if c.clip_expert else "noclip",
                     "std" if c.standardizer else "nostd"])


_CACHE = {}


def h_inputs(in_dim, A, B, n_policy, seed, updates=UPDATES):
    """(steps, params): iq_restate.case_inputs from the seed, then the H update's own columns from a generator of their
    own: the absorbing flags, the expert rows' shifted log-probabilities, q_t and v_t; H's output layer scaled.  At
    B = 2 the policy's row is absorbing and the expert's is not."""
    steps, params = R.case_inputs(in_dim, A, B, seed=seed, updates=updates)
    rng = np.random.default_rng(7000 + seed)
    f = np.float32
    for s in steps:
        s["absorbing"] = np.array((1.0, 0.0), f) if B == 2 else (rng.uniform(0, 1, B) < ABSORBING_FRAC).astype(f)
        s["logp_next"][n_policy:] -= f(EXPERT_SHIFT)
        s["q_t"] = (rng.standard_normal(B) * QT_DEV).astype(f)
        s["v_t"] = (rng.standard_normal(B) * QT_DEV).astype(f)
        del s["a_pi"], s["logp_pi"]
    params = [np.asarray(p, np.float32).copy() for p in params]
    params[4] *= f(W3_SCALE)
    params[5] *= f(W3_SCALE)
    return steps, params


def sweep_inputs(k):
    """(steps, params) of shape k, rebuilt once; callers leave them unchanged."""
    if ("in", k) not in _CACHE:
        in_dim, A, B, n_policy = SHAPES[k]
        _CACHE[("in", k)] = h_inputs(in_dim, A, B, n_policy, SEEDS[k])
    return _CACHE[("in", k)]


def clipped_inputs():
    if "clipped" not in _CACHE:
        _CACHE["clipped"] = h_inputs(*SHAPES[1], CLIPPED_SEED)
    return _CACHE["clipped"]


def case_steps(cfg, steps):
    """The steps as config cfg takes them: q_t / v_t go with LSIQ_HC alone."""
    return steps if cfg.cost else [{k: v for k, v in s.items() if k not in ("q_t", "v_t")} for s in steps]


def yardstick(k, j):
    """(float64 state, float64 out, float32 state, float32 out) of config j at shape k (k = "clipped": of CLIPPED[j] at
    shape 1), computed once and shared; the float64 run's margins are asserted here, for every update."""
    if (k, j) not in _CACHE:
        clipped = k == "clipped"
        steps, params = clipped_inputs() if clipped else sweep_inputs(k)
        cfg = CLIPPED[j] if clipped else CONFIGS[j]
        n_policy = SHAPES[1 if clipped else k][3]
        st = case_steps(cfg, steps)
        s64, o64, margins = run(params, cfg, st, n_policy, check=True)
        assert_margins(margins, (k, cfg_id(cfg)), clipped_targets=clipped)
        _CACHE[(k, j)] = (s64, o64) + run(params, cfg, st, n_policy, torch.float32)
    return _CACHE[(k, j)]


# ---------------------------------------------------------------------------------------------- the agents' critic side
class CriticTwin:
    """update_Q_function of LSIQ_H / LSIQ_HC whole, as DeviceLSIQH / DeviceLSIQHC run it: iq_pi_restate's Policy (not
    trained here), lsiq_restate's LSIQSoftQ as the Q critic with alpha 0 (getV / get_targetV drop the entropy,
    lsiq_h.py:110-120) and HCritic as H.  The order is the reference's: the Q update's policy passes and its step
    (super()._lossQ_* ends in update_Q_parameters), then update_H_function: a NEW policy pass on next_obs, for LSIQ_HC
    Q_target(obs | act), a policy pass on obs and Q_target(obs | a_pi) (both feed the target critic's Standardizer), the
    H step; then _update_all_targets, of which the Q critic's part runs inside its update for LSIQ_H (the H update does
    not read it) and after the H update for LSIQ_HC."""

    def __init__(self, pparams, qparams, hparams, central, delta, pcfg, lcfg, hcfg, dtype=torch.float64, wrong=None,
                 check=False):
        import iq_pi_restate as P
        assert lcfg.type == "iq_like", "the twin issues iq_like's policy passes"
        self.pi = None if pparams is None else P.Policy(pparams, central, delta, pcfg, dtype)    # None: passes are given
        self.late = hcfg.cost and wrong != "target_after"
        self.h_first = wrong == "h_before_q"
        self.q = LSIQSoftQ(qparams, lcfg._replace(alpha=0.0, update_target=not self.late), dtype, check=check)
        self.h = HCritic(hparams, hcfg, dtype, None if wrong in ("target_after", "h_before_q") else wrong, check=check)

    def update_Q_function(self, s, n_policy, eps, logging=True, given=None):
        """eps: dict(next, expert, pi: the Q update's passes; h_next, h_pi: the H update's).  given: in place of the
        twin's own policy, the (action, log_prob) a run produced in each pass, dict(next, pi, h_next and, for LSIQ_HC,
        h_pi).  Returns (the Q critic's 16 scalars, the H update's)."""
        obs, act, nxt = s["obs"], s["act"], s["next_obs"]
        f = lambda t: t.detach().to(torch.float32).numpy()
        if self.h_first:
            assert given is None, "the order of the policy's passes shows only where the twin runs them"
            out_h = self._h_part(s, n_policy, eps, None)
            with torch.no_grad():
                a_next, lp_next = (f(t) for t in self.pi.act(nxt, eps["next"]))
                if logging:
                    self.pi.act(obs[n_policy:], eps["expert"])
                a_pi, lp_pi = (f(t) for t in self.pi.act(obs, eps["pi"]))
            out_q = self.q.update(obs, act, nxt, s["absorbing"], a_next, lp_next, a_pi, lp_pi, n_policy)
            return out_q, out_h
        if given is not None:
            (a_next, lp_next), (a_pi, lp_pi) = given["next"], given["pi"]
        else:
            with torch.no_grad():
                a_next, lp_next = (f(t) for t in self.pi.act(nxt, eps["next"]))
                if logging:
                    self.pi.act(obs[n_policy:], eps["expert"])
                a_pi, lp_pi = (f(t) for t in self.pi.act(obs, eps["pi"]))
        out_q = self.q.update(obs, act, nxt, s["absorbing"], a_next, lp_next, a_pi, lp_pi, n_policy)
        return out_q, self._h_part(s, n_policy, eps, given)

    def _h_part(self, s, n_policy, eps, given):
        obs, act, nxt = s["obs"], s["act"], s["next_obs"]
        f = lambda t: t.detach().to(torch.float32).numpy()
        with torch.no_grad():
            a_h, lp_h = given["h_next"] if given is not None else (f(t) for t in self.pi.act(nxt, eps["h_next"]))
            q_t = v_t = None
            if self.h.cfg.cost:
                q_t = f(self.q.forward(np.concatenate([obs, act], 1), target=True))
                a_v = given["h_pi"][0] if given is not None else f(self.pi.act(obs, eps["h_pi"])[0])
                v_t = f(self.q.forward(np.concatenate([obs, a_v], 1), target=True))
        out_h = self.h.update(obs, act, nxt, s["absorbing"], a_h, lp_h, n_policy, q_t=q_t, v_t=v_t)
        if self.late:
            c = self.q.cfg
            self.q.t = [update_target(c.tau, p.detach(), t) for p, t in zip(self.q.p, self.q.t)]
        return out_h

    def state(self):
        return dict(q=self.q.state(), h=dict(self.h.state(), max=None if self.h.M is None else float(self.h.M)),
                    policy_colstats=None if self.pi is None or self.pi.stand is None else self.pi.stand.colstats.copy())


AGENT_SEEDS = {False: 41, True: 42}     # the first from 41 upwards at which the float64 twin's margins hold


def agent_case(cost, seed=None):
    """One case of the agents' test at (12, 5, 18, 9): three batches, the noise of every policy pass, the three networks'
    initial parameters (both critics' output layers scaled, as the sweeps') and the configurations."""
    import iq_pi_restate as P
    import lsiq_restate as L
    seed = AGENT_SEEDS[cost] if seed is None else seed
    in_dim, A, B, n_policy = SHAPES[1]
    case = P.case_inputs(in_dim, A, B, seed=seed)
    steps, hparams = R.case_inputs(in_dim, A, B, seed=seed + 1, updates=UPDATES)
    rng = np.random.default_rng(9000 + seed)
    f = np.float32
    for s in steps:
        s["absorbing"] = (rng.uniform(0, 1, B) < ABSORBING_FRAC).astype(f)
    scale = lambda ps: [np.asarray(p, f) * (f(W3_SCALE) if i >= 4 else f(1)) for i, p in enumerate(ps)]
    noise = [{k: rng.standard_normal((B - n_policy if k == "expert" else B, A)).astype(f)
              for k in ("next", "expert", "pi", "h_next", "h_pi")} for _ in steps]
    pcfg = P.PiCfg(standardizer=True, adam_eps=P.SWEEP_EPS, ls_min=P.SWEEP_LS[0], ls_max=P.SWEEP_LS[1])
    lcfg = L.LCfg(type="iq_like", exp_mode="fix", exp_loss="Huber", mode="value", q_min=Q_MIN, q_max=Q_MAX,
                  reg_mult=HC_REG_MULT if cost else 0.5, lr=SWEEP_LR, adam_eps=SWEEP_EPS, tau=0.05)
    hcfg = HCfg(cost=cost, loss="Huber" if cost else "MSE", tau_up=TAU_UP, tau_down=TAU_DOWN, q_min=Q_MIN, q_max=Q_MAX,
                reg_mult=lcfg.reg_mult, lr=2 * SWEEP_LR, alpha=SWEEP_ALPHA, tau=0.2 if cost else lcfg.tau, adam_eps=SWEEP_EPS)
    return dict(in_dim=in_dim, A=A, B=B, n_policy=n_policy, steps=steps, noise=noise, pparams=case["pparams"],
                qparams=scale(case["cparams"]), hparams=scale(hparams), central=case["central"], delta=case["delta"],
                pcfg=pcfg, lcfg=lcfg, hcfg=hcfg)


def run_agent(case, dtype=torch.float64, wrong=None, check=False):
    """The case's updates through CriticTwin; returns (state, Q scalars [updates, 16], H scalars [updates, 16]) and, with
    check, the H critic's margins."""
    twin = CriticTwin(case["pparams"], case["qparams"], case["hparams"], case["central"], case["delta"], case["pcfg"],
                      case["lcfg"], case["hcfg"], dtype, wrong, check)
    outs = [twin.update_Q_function(s, case["n_policy"], e) for s, e in zip(case["steps"], case["noise"])]
    res = (twin.state(), np.asarray([o[0] for o in outs]), np.asarray([o[1] for o in outs]))
    return res + ((twin.h.margins,) if check else ())


# ---------------------------------------------------------------------------------------------- the reference-run fixtures
FIXTURES = ("h_iq", "hc_huber", "hc_mse")


def fixture_errors(g, gen, params, prefix):
    """The largest distance of six parameter arrays from a fixture's stored group (layers 1 and 2: their stored rows)."""
    heads = dict(w1=gen.W1_HEAD, w2=gen.W2_HEAD)
    return max(float(np.abs((a[:heads[n]] - g[f"{prefix}_{n}_head"]) if n in heads else (a - g[f"{prefix}_{n}"])).max())
               for n, a in zip(R.NAMES, params))


def fixture_whole(g, name, gen, wrong=None, dtype=torch.float64):
    """whole_twin over a fixture: the policy run by the twin itself on the recorded noise, trained by the two-critic
    actor loss; returns (the twin after the last iq_update, the H scalars [updates, 16])."""
    import iq_pi_restate as P
    spec = gen.FIXTURES[name]
    lcfg, hcfg = gen.twin_cfgs(spec, float(g["alpha"]))
    init = lambda prefix, seed: [gen.w2_init(seed) if n == "w2" else g[f"{prefix}_init_{n}"] for n in R.NAMES]
    f = np.float32
    case = dict(pparams=init("policy", 11), qparams=init("critic", 12), hparams=init("h", gen.H_W2_SEED),
                central=(0.5 * (g["max_a"] + g["min_a"])).astype(f), delta=(0.5 * (g["max_a"] - g["min_a"])).astype(f),
                lcfg=lcfg, hcfg=hcfg, pcfg=P.PiCfg(lr=float(g["lr_actor"]), ls_min=gen.G.LOG_STD_MIN, ls_max=gen.G.LOG_STD_MAX))
    order = [k for k in gen.PASSES + gen.PI_PASSES if spec["cost"] or k != "h_pi"]
    twin, outs = whole_twin(case, dtype, wrong=wrong), []
    for i in range(gen.N_ITER):
        s = {k: g[k][i] for k in ("obs", "act", "next_obs", "absorbing")}
        outs.append(twin.iq_update(s, int(g["n_policy"]), {k: g["eps_" + k][i] for k in order})[1])
    return twin, np.asarray(outs)


# ---------------------------------------------------------------------------------------------- the two-critic actor loss
def actor_twin(pparams, cparams, hparams, central, delta, cfg, dtype=torch.float64, wrong=None, qcfg=None):
    """iq_pi_restate's Twin with LSIQ_H's _actor_loss (lsiq_h.py:104-108): q = critic(state | a_new), then
    H = H_approximator(state | a_new), both live, each feeding its own Standardizer the Bp rows, soft_q = q + H (both
    [Bp, 1]) and loss = mean(alpha log_prob - soft_q) with the [Bp, Bp] broadcast Twin.policy_step keeps.  `hq` is H as a
    SoftQ.  wrong "no_h": the actor loss without H."""
    import iq_pi_restate as P

    class ActorTwin(P.Twin):
        def critic(self, x, a_new):
            q = super().critic(x, a_new)
            if wrong == "no_h":
                return q
            keep, self.q = self.q, self.hq        # Twin.critic's lines on the other network
            try:
                h = super().critic(x, a_new)
            finally:
                self.q = keep
            return q + h

        def policy_step(self, x, eps):
            for p in self.hq.p:
                p.grad = None
            return super().policy_step(x, eps)

        def state(self):
            return dict(super().state(), h=self.hq.state())
    t = ActorTwin(pparams, cparams, central, delta, cfg, qcfg=qcfg, dtype=dtype)
    t.hq = R.SoftQ(hparams, qcfg if qcfg is not None else R.Cfg(standardizer=cfg.standardizer), dtype)
    return t


H_SEED_OFFSET = 300      # H's initial parameters: il_shapes.linear_params from the case's seed + this


def actor_case(k):
    """iq_pi_restate's inputs of shape k with a second critic's parameters."""
    import iq_pi_restate as P
    from il_shapes import linear_params
    if ("actor", k) not in _CACHE:
        in_dim, A, Bp = P.SHAPES[k]
        case = dict(P.sweep_inputs(k))
        case["hparams"] = linear_params([(in_dim + A, 512), (512, 256), (256, 1)], H_SEED_OFFSET + 20 + k)
        _CACHE[("actor", k)] = case
    return _CACHE[("actor", k)]


def run_actor(case, cfg, dtype=torch.float64, wrong=None, act=None):
    """The policy steps of `case` in order: (state after the last, out [updates, 4], a_new and log_prob of every step).
    act: as iq_pi_restate.run's."""
    import iq_pi_restate as P
    t = actor_twin(case["pparams"], case["cparams"], case["hparams"], case["central"], case["delta"],
                   cfg._replace(init_alpha=P.ALPHA), dtype, wrong)
    if act is not None:
        t.pi.act = lambda x, eps: act(t.pi, x, eps)
    outs, acts = [], []
    for s in case["steps"]:
        o, a, lp = t.policy_step(s["x"], s["eps"])
        outs.append(o)
        acts.append((a.double().numpy(), lp.double().numpy()))
    return t.state(), np.asarray(outs), acts


def actor_yardstick(k, j):
    """(float64 state, out, acts, float32 state, out, acts) of iq_pi_restate's config j at shape k with two critics."""
    import iq_pi_restate as P
    if ("actor", k, j) not in _CACHE:
        case = actor_case(k)
        _CACHE[("actor", k, j)] = run_actor(case, P.CONFIGS[j]) + run_actor(case, P.CONFIGS[j], torch.float32)
    return _CACHE[("actor", k, j)]


# ---------------------------------------------------------------------------------------------- the whole agents
def whole_twin(case, dtype=torch.float64, check=False, wrong=None):
    """LSIQ_H / LSIQ_HC whole on agent_case's networks: CriticTwin's update_Q_function, then iq_pi_restate's
    update_policy with the two-critic actor loss on the SAME live critics and the same policy (iq_update,
    iq_sac.py:408-419).  Returns an object with iq_update(s, n_policy, eps, logging) and state()."""
    import iq_pi_restate as P
    crit = CriticTwin(case["pparams"], case["qparams"], case["hparams"], case["central"], case["delta"], case["pcfg"],
                      case["lcfg"], case["hcfg"], dtype, None if wrong == "no_h" else wrong, check)
    act = actor_twin(case["pparams"], case["qparams"], case["hparams"], case["central"], case["delta"],
                     case["pcfg"]._replace(init_alpha=case["hcfg"].alpha), dtype, wrong if wrong == "no_h" else None)
    act.q, act.hq, act.pi = crit.q, crit.h, crit.pi          # one set of networks
    act.pi.opt = torch.optim.Adam(act.pi.p, lr=case["pcfg"].lr, betas=(0.9, 0.999), eps=case["pcfg"].adam_eps,
                                  weight_decay=case["pcfg"].wd)

    class Whole:
        critic, actor = crit, act

        def iq_update(self, s, n_policy, eps, logging=True):
            out_q, out_h = crit.update_Q_function(s, n_policy, eps, logging)
            act.iter = getattr(self, "iter", 1)
            out_pi = act.update_policy(s["obs"], n_policy, dict(pi=eps["ppi"], log=eps.get("plog")), logging)
            self.iter = act.iter + 1
            act.pi.iter += 1
            return out_q, out_h, out_pi

        def state(self):
            return dict(crit.state(), policy=act.pi.state())
    return Whole()
