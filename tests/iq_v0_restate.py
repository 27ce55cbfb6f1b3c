"""The yardstick of K26's v0 pass and of all-expert batches (oly_iq_q_update with the block oly_iq_v0,
csrc/k26_iq_critic.hip): plcy_loss_mode "v0" of IQ_SAC._lossQ (imitation_lib/imitation/iq_sac.py:508-510) and of LSIQ's
iq_like loss (imitation_lib/imitation/lsiq.py:90-92), and LSIQ_Offline._lossQ (imitation_lib/imitation/offline/
lsiq_offline.py:50-159) under the neutral reading _Q_Q_multiplier = _abs_mult = 1.0, which is the iq_like loss with v0, an
all-expert batch, the clip always on and the absorbing-state weighting always on.  Everything else (the network, the
Standardizers pass by pass, Adam, the target update, the margins' record) is iq_restate's SoftQ and lsiq_restate's
LSIQSoftQ, by import.  IQ is the LSIQ configuration with bootstrap and no clipping (lsiq_restate.as_iq).

The fourth pass: after getV(obs) (which always runs and here carries no gradient), getV(obs[expert]) draws the policy's
action anew (a_v0, logp_v0: inputs here as they are inputs of the kernel), the live critic's Standardizer takes the n_v0
rows (obs[expert] | a_v0) and standardises them with what it then holds, and
loss_term2 = mean((1 - gamma) (Q_v0 - alpha logp_v0)) with 1 - gamma formed in the run's precision from the float32 gamma.

The wrong readings (`wrong=`), each a plausible misreading the fixtures must tell from the reference:
  v0_reuses_sample   v0 takes getV(obs)'s sample on the expert rows (a_pi[expert], logp_pi[expert]) instead of its own draw
  v0_no_stats        the fourth pass does not feed the Standardizer: it is standardised with what the third pass left
  v_pass_gradient    the pass on (obs | a_pi) carries the gradient: loss_term2 = mean(V - y), which is mode "value"
and the readings LSIQSoftQ carries.  No tests here: tests/test_iq_v0_cpu.py and tests/test_gpu_iq_v0.py use it."""
import numpy as np
import torch

import iq_restate as R
import lsiq_restate as L
from lsiq_restate import LCfg, LSIQSoftQ, update_target

TOL, cat = R.TOL, R.cat
ALL_EXPERT_REFUSED_MODES = ("value_policy", "q_old_policy", "value_q_old_policy")
V0_MODES = L.IQ_LIKE_MODES + ("v0",)


def iq_cfg(**kw):
    """algo "iq" as the LSIQ configuration it coincides with: bootstrap, no Q_exp_loss, no clipping."""
    return LCfg(type="iq_like", exp_mode="bootstrap", exp_loss=None, clip=False, **kw)


def offline_cfg(**kw):
    """LSIQ_Offline's loss: v0, the clip and the absorbing weighting always on; loss_mode_exp fix and regularizer off by
    default (lsiq_offline.py:11)."""
    base = dict(type="iq_like", exp_mode="fix", exp_loss="MSE", clip=True, mode="v0", reg="off", treat=True)
    base.update(kw)
    return LCfg(**base)


class V0SoftQ(LSIQSoftQ):
    """LSIQSoftQ with the iq_like loss's mode v0 and batches without policy rows."""

    def update(self, obs, act, next_obs, absorbing, a_next, logp_next, a_pi, logp_pi, n_policy, a_v0=None, logp_v0=None):
        """One update_Q_function and _update_all_targets; the 16 scalars of oly_iq_q_update as float64.  a_v0 [n_v0, A],
        logp_v0 [n_v0]: the policy's own draw on obs[n_policy:], read in mode v0."""
        c, dt, wrong = self.cfg, self.dtype, self.wrong
        assert c.type == "iq_like" and c.mode in V0_MODES
        B = len(obs)
        assert 0 <= n_policy < B
        if n_policy == 0:
            assert c.mode not in ALL_EXPERT_REFUSED_MODES and c.reg != "plcy", "an empty policy subset inside the loss"
        self._huber, self._relu = [], []
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        exp = torch.arange(B) >= n_policy
        x0, x1 = np.concatenate([obs, act], 1), np.concatenate([next_obs, a_next], 1)
        x2 = np.concatenate([obs, a_pi], 1)
        ab = t(absorbing).reshape(B, 1)
        alpha, gamma = t(c.alpha), t(c.gamma)
        Q = self.forward(x0)
        if c.use_target:
            with torch.no_grad():
                nq = self.forward(x1, target=True)
        else:
            nq = self.forward(x1)
        next_v = nq - alpha * t(logp_next).reshape(B, 1)
        y = (1 - ab) * gamma * (torch.clip(next_v, c.q_min, c.q_max) if c.clip else next_v)
        reward = Q - y
        V = self.forward(x2) - alpha * t(logp_pi).reshape(B, 1)
        value = V - y
        if c.exp_mode == "bootstrap":
            loss1 = -reward[exp].mean()
        else:
            loss1 = self._point(Q[exp], torch.ones_like(Q[exp]) * c.q_max)
        if c.mode == "v0" and wrong != "v_pass_gradient":
            if wrong == "v0_reuses_sample":
                a_v0, logp_v0 = np.asarray(a_pi)[n_policy:], np.asarray(logp_pi)[n_policy:]
            x3 = np.concatenate([np.asarray(obs)[n_policy:], a_v0], 1)
            frozen = None
            if wrong == "v0_no_stats" and self.stand is not None:
                cs = self.stand.colstats
                cnt = cs[0] + 1e-2
                mean = cs[1] / cnt
                std = np.sqrt(np.maximum((cs[2] + 1e-2) / cnt - np.square(mean), 1e-2))
                frozen = lambda x: ((np.asarray(x, np.float64) - mean) / std).astype(np.float32)
            V0 = self.forward(x3, frozen=frozen) - alpha * t(logp_v0).reshape(-1, 1)
            loss2 = ((1 - gamma) * V0).mean()
        elif c.mode == "v0":
            loss2 = value.mean()
        else:
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
        out = np.zeros(16)
        out[0], out[1], out[2] = (float(v.detach()) for v in (loss1, loss2, chi2))
        out[3] = float(V.detach().double().mean())
        self.opt.zero_grad()
        loss.backward()
        out[15] = float(torch.cat([p.grad.reshape(-1) for p in self.p]).double().norm())
        self.opt.step()
        with torch.no_grad():
            d = lambda v: v.detach().double()
            mean = lambda v: float(v.mean()) if v.numel() else np.nan       # torch's mean of nothing
            Qd, yd, rd, a_ = d(Q), d(y), d(reward), ab.reshape(-1) != 0
            out[4], out[5] = mean(Qd[exp]), mean(torch.square(Qd[exp]))
            out[6], out[7] = mean(Qd[~exp]), mean(torch.square(Qd[~exp]))
            out[8], out[9], out[10] = mean(rd), mean(rd[exp]), mean(rd[~exp])
            out[11], out[12] = mean(yd[exp]), mean(yd[~exp])
            out[13], out[14] = mean(Qd[exp][a_[exp]]), mean(Qd[~exp][a_[~exp]])
            if c.update_target:
                self.t = [update_target(c.tau, p.detach(), q) for p, q in zip(self.p, self.t)]
            if self.check:
                nv = d(next_v).reshape(-1).numpy()
                h = torch.cat(self._huber).numpy() if self._huber else np.zeros(0)
                self.margins.append(dict(
                    B=B, relu_margin=min(self._relu), clip=bool(c.clip), huber=c.exp_loss == "Huber" and len(h) > 0,
                    clip_margin=float(np.minimum(np.abs(nv - c.q_min), np.abs(nv - c.q_max)).min()),
                    below=int((nv < c.q_min).sum()), inside=int(((nv >= c.q_min) & (nv <= c.q_max)).sum()),
                    above=int((nv > c.q_max).sum()),
                    huber_margin=float(np.abs(np.abs(h) - 1.0).min()) if len(h) else np.inf,
                    quadratic=int((np.abs(h) < 1.0).sum()), linear=int((np.abs(h) >= 1.0).sum())))
        return out


def run(params, cfg, steps, n_policy, dtype=torch.float64, wrong=None, check=False, target=None):
    """The updates of `steps` in order; (state after the last, out [updates, 16]) and, with check, the margins."""
    q = V0SoftQ(params, cfg, dtype, wrong, target=target, check=check)
    out = [q.update(n_policy=n_policy, **s) for s in steps]
    return (q.state(), np.asarray(out)) + ((q.margins,) if check else ())


class OfflineTwin:
    """LSIQ_Offline whole (lsiq_offline.py:9-210): iq_pi_restate's Twin (the policy, its Adam, the temperature,
    update_policy, whose lines with no policy rows are the reference's override's: get_mu_log_sigma on zero rows feeds the
    Standardizer nothing and the two policy-states means are NaN) around V0SoftQ with offline_cfg, on batches of expert
    rows.  wrong: one of V0SoftQ's readings."""

    def __new__(cls, pparams, cparams, central, delta, cfg, qcfg, dtype=torch.float64, wrong=None):
        import iq_pi_restate as P

        class _Twin(P.Twin):
            def iq_update(self, s, eps, logging=True):
                """One LSIQ_Offline.iq_update (:161-173) and fit_offline's counters on s = dict(obs, act, next_obs,
                absorbing).  eps: dict(next, expert (logging), pi, v0: update_Q_function's passes in their order; ppi,
                plog: update_policy's).  Returns (the critic's 16 scalars, the policy's 4)."""
                self.q.cfg = self.q.cfg._replace(alpha=float(self.alpha))
                obs = s["obs"]
                f = lambda t: t.detach().to(torch.float32).numpy()
                with torch.no_grad():
                    a_next, lp_next = (f(t) for t in self.pi.act(s["next_obs"], eps["next"]))
                    if logging:
                        self.pi.act(obs, eps["expert"])                 # logging_loss's draw_action(obs[is_expert])
                    a_pi, lp_pi = (f(t) for t in self.pi.act(obs, eps["pi"]))      # getV(obs)
                    a_v0, lp_v0 = (f(t) for t in self.pi.act(obs, eps["v0"]))      # getV(obs[is_expert])
                out_q = self.q.update(obs, s["act"], s["next_obs"], s["absorbing"], a_next, lp_next, a_pi, lp_pi, 0,
                                      a_v0=a_v0, logp_v0=lp_v0)
                out_pi = self.update_policy(obs, 0, dict(pi=eps["ppi"], log=eps.get("plog")), logging)
                self.iter += 1
                self.pi.iter += 1
                return out_q, out_pi
        assert qcfg.mode == "v0" and qcfg.clip and qcfg.treat and not cfg.own_states
        t = _Twin(pparams, cparams, central, delta, cfg, dtype=dtype)
        t.q = V0SoftQ(cparams, qcfg, dtype, wrong)
        return t


# ---------------------------------------------------------------------------------------------- the GPU test's cases
# (in_dim, A, B, n_policy).  B and n_policy are the smallest that can go wrong: one full tile plus two rows with the halves
# split inside the first tile (18, 9); no policy rows at all with one row in the second tile (17, 0); a single expert row,
# alone in the second tile, so the first tile's v0 pass takes no row (17, 16); the smallest batch (2, 0); three tiles with
# one row in the last (33, 0); many tiles, with no policy rows (300, 0) and with the boundary inside a tile (300, 137).
# in_dim + A is 17 (two k-groups in layer 1, the <2> instantiation) or 64 (the <4> instantiation, every column used).
SHAPES = ((12, 5, 18, 9), (12, 5, 17, 0), (48, 16, 17, 16), (12, 5, 2, 0), (48, 16, 33, 0), (12, 5, 300, 0), (48, 16, 300, 137))
UPDATES = 2
# the output layer's scale, the clip bounds, the learning rate and Adam's eps are lsiq_restate's, for its reasons
W3_SCALE, Q_MIN, Q_MAX, SWEEP_LR, SWEEP_EPS = L.W3_SCALE, L.Q_MIN, L.Q_MAX, L.SWEEP_LR, L.SWEEP_EPS


def sweep_configs():
    """(algo, config): IQ and LSIQ fix/MSE, fix/Huber and bootstrap, each with v0; the regularizers off, exp and
    exp_and_plcy, the target, the Standardizers, treat_absorbing_states and a weight decay alternate over the list.  The
    last entries are all-expert batches in the modes that need no v0 draw (value, value_expert, off): they run in the
    kernel's existing instantiations with n_policy = 0."""
    kinds = [("iq", iq_cfg()), ("lsiq", LCfg(exp_mode="fix", exp_loss="MSE")), ("lsiq", LCfg(exp_mode="fix", exp_loss="Huber")),
             ("lsiq", LCfg(exp_mode="bootstrap", exp_loss=None))]
    regs = ("off", "exp", "exp_and_plcy")
    out = []
    for i in range(12):
        algo, c = kinds[i % 4]
        out.append((algo, c._replace(mode="v0", reg=regs[(i + i // 4) % 3], use_target=(i // 2) % 2 == 0)))
    out.append(("lsiq", offline_cfg()))
    out.append(("lsiq", offline_cfg(exp_loss="Huber", reg="exp", use_target=False)))
    full = [(a, c._replace(standardizer=(i // 3) % 2 == 0, treat=c.treat or (i // 2) % 2 == 1, wd=1e-4 if i % 3 == 0 else 0.0,
                           tau=0.05, adam_eps=SWEEP_EPS, lr=SWEEP_LR,
                           **({} if a == "iq" else dict(q_min=Q_MIN, q_max=Q_MAX)))) for i, (a, c) in enumerate(out)]
    return full


CONFIGS = sweep_configs()
# all-expert batches without v0: config, run at the shapes with n_policy = 0
PLAIN_ALL_EXPERT = [("iq", iq_cfg(mode="value", reg="exp", tau=0.05, adam_eps=SWEEP_EPS, lr=SWEEP_LR)),
                    ("lsiq", LCfg(mode="value_expert", reg="exp_and_plcy", exp_loss="MSE", use_target=False, tau=0.05,
                                  adam_eps=SWEEP_EPS, lr=SWEEP_LR, q_min=Q_MIN, q_max=Q_MAX)),
                    ("lsiq", LCfg(mode="off", reg="off", exp_loss="Huber", tau=0.05, adam_eps=SWEEP_EPS, lr=SWEEP_LR,
                                  q_min=Q_MIN, q_max=Q_MAX))]


def sweep(k):
    """[(number, algo, config)] of shape k: every shape runs four consecutive configs of the list (with 7 shapes and 14
    configs each config runs at two shapes), so the seven shapes together run every one at both widths."""
    n = len(CONFIGS)
    return [((2 * k + i) % n,) + CONFIGS[(2 * k + i) % n] for i in range(4)]


def cfg_id(algo, c):
    return algo + "-" + L.cfg_id(c)


_CACHE = {}


def sweep_inputs(k, seed=None):
    """(steps, params) of shape k: iq_restate.case_inputs with a_v0 / logp_v0 [n_v0] added and the output layer scaled,
    rebuilt once; callers leave them unchanged."""
    key = ("in", k, seed)
    if key not in _CACHE:
        in_dim, A, B, n_policy = SHAPES[k]
        steps, params = R.case_inputs(in_dim, A, B, seed=(40 + k) if seed is None else seed, updates=UPDATES)
        rng = np.random.default_rng(900 + k)
        for s in steps:
            s["a_v0"] = np.tanh(rng.standard_normal((B - n_policy, A))).astype(np.float32)
            s["logp_v0"] = (rng.standard_normal(B - n_policy) * 2 - A).astype(np.float32)
        params = [np.asarray(p, np.float32).copy() for p in params]
        params[4] *= np.float32(W3_SCALE)
        params[5] *= np.float32(W3_SCALE)
        _CACHE[key] = (steps, params)
    return _CACHE[key]


def case_steps(cfg, steps):
    """The steps as config cfg takes them: a_v0 / logp_v0 only in mode v0."""
    if cfg.mode == "v0":
        return steps
    return [{k: v for k, v in s.items() if k not in ("a_v0", "logp_v0")} for s in steps]


def yardstick(k, algo, cfg):
    """(float64 state, float64 out, float32 state, float32 out, margins) of a config at shape k, computed once and shared.
    The margins are returned, not asserted: a case whose float64 run has a row within rounding of a kink is told by its
    float32 spread, which widens its own tolerance (4 x the spread) as the project's rule has it."""
    key = (k, algo, cfg)
    if key not in _CACHE:
        steps, params = sweep_inputs(k)
        n_policy = SHAPES[k][3]
        st = case_steps(cfg, steps)
        s64, o64, margins = run(params, cfg, st, n_policy, check=True)
        _CACHE[key] = (s64, o64) + run(params, cfg, st, n_policy, torch.float32) + (margins,)
    return _CACHE[key]
