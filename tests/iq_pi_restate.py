"""The yardstick of K27 (oly_iq_pi_update and oly_iq_alpha_update, csrc/k27_iq_policy.hip): IQ_SAC.update_policy with
_actor_loss and _update_alpha (imitation_lib/imitation/iq_sac.py:431-465, 587-595) and the whole of iq_update (:408-419;
SQIL's, imitation_lib/imitation/sqil_sac.py:16-62) restated with torch autograd and torch.optim.Adam, both Standardizers
in numpy float64 as tests/iq_restate.py keeps them, in float64 (the yardstick) or float32 (what the reference runs).  No
tests here: tests/test_iq_pi_cpu.py holds this file against the fixtures of tests/golden/gen_iq_pi_update.py (which
executes the reference's own lines) and holds the sweep's table to its purpose, tests/test_gpu_iq_pi.py runs the kernel
against it.

The loss is formed as the reference forms it: the critic is built with squeeze_out=False, so q is [Bp, 1] against log_prob
[Bp] and alpha log_prob - q broadcasts to [Bp, Bp] before the mean.  The kernel computes the row-wise mean; the two agree
to rounding, which is what holding the kernel to this file shows.

_optimize_actor_parameters is mushroom-rl's DeepAC's RESTATED from its published definition (mushroom-rl is not
installed): zero_grad, backward, (clipping: not built), optimizer.step() over the policy's parameters.  The gradient this
leaves on the critic's parameters is discarded by the critic optimiser's zero_grad (iq_sac.py:567), as SoftQ.update does."""
from collections import namedtuple

import numpy as np
import torch

import iq_restate as Q
from bc_restate import Standardizer
from il_shapes import TOL, _columns, linear_params  # noqa: F401  (TOL is re-exported to the tests)

NAMES = Q.NAMES
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
INIT_ALPHA = 1e-3
PI_TAGS = ("Actor/Loss", "Gradients/Norm2 Gradient Q wrt. Pi-parameters")
LOG_TAGS = ("Actor/Entropy Expert States", "Actor/Entropy Policy States", "Actor/Entropy from Gaussian Policy States",
            "Actor/Entropy Lower Bound", "Actor/Entropy from Gaussian Expert States")

PiCfg = namedtuple("PiCfg", "standardizer lr wd adam_eps ls_min ls_max own_states learnable lr_alpha target_entropy "
                            "init_alpha e_thres e_reduc",
                   defaults=(True, 3e-4, 0.0, 1e-8, LOG_STD_MIN, LOG_STD_MAX, False, False, 3e-4, None, INIT_ALPHA, 2.0,
                             1e-5))


def _moments(st):
    cnt = st.colstats[0] + 1e-2
    mean = st.colstats[1] / cnt
    return mean, np.sqrt(np.maximum((st.colstats[2] + 1e-2) / cnt - np.square(mean), 1e-2))


class Policy:
    """IQ_Learn_Policy (iq_sac.py:18-167) over FullyConnectedNetwork(in -> [512, 256] -> 2A) with its Standardizer and the
    actor's Adam."""

    def __init__(self, params, central, delta, cfg, dtype):
        self.cfg, self.dtype = cfg, dtype
        self.p = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in params]
        self.A = int(self.p[4].shape[0]) // 2
        self.central = torch.as_tensor(np.asarray(central, np.float32)).to(dtype)
        self.delta = torch.as_tensor(np.asarray(delta, np.float32)).to(dtype)
        self.stand = Standardizer(int(self.p[0].shape[1])) if cfg.standardizer else None
        self.opt = torch.optim.Adam(self.p, lr=cfg.lr, betas=(0.9, 0.999), eps=cfg.adam_eps, weight_decay=cfg.wd)
        self.iter = 0

    def heads(self, x):
        """The network's forward (its Standardizer takes the rows): [n, 2A], mu | log_sigma before the clamp."""
        z = self.stand(x) if self.stand is not None else np.asarray(x, np.float32)
        z = torch.as_tensor(z).to(self.dtype)
        z = torch.relu(z @ self.p[0].T + self.p[1])
        z = torch.relu(z @ self.p[2].T + self.p[3])
        return z @ self.p[4].T + self.p[5]

    def mu_log_sigma(self, x):
        """get_mu_log_sigma (:132-151): the forward, the split, the clamp."""
        y = self.heads(x)
        return y[:, :self.A], torch.clamp(y[:, self.A:], self.cfg.ls_min, self.cfg.ls_max)

    def act(self, x, eps):
        """compute_action_and_log_prob_t (:102-130) with the noise given: (a_new [n,A], log_prob [n]), with gradients."""
        mu, ls = self.mu_log_sigma(x)
        sigma = ls.exp()
        u = mu + sigma * torch.as_tensor(np.asarray(eps, np.float32)).to(self.dtype)
        a = torch.tanh(u)
        logp = torch.distributions.Normal(mu, sigma).log_prob(u).sum(dim=1)
        logp = logp - torch.log(1.0 - a.pow(2) + 1e-6).sum(dim=1)
        return a * self.delta + self.central, logp

    def entropy_from_logsigma(self, ls):
        return self.A * (0.5 + 0.5 * np.log(2 * np.pi)) + torch.sum(ls, dim=-1)

    def state(self):
        z = lambda p: np.zeros(tuple(p.shape))
        g = lambda k: [self.opt.state[p][k].double().numpy().copy() if p in self.opt.state else z(p) for p in self.p]
        return dict(params=[p.detach().double().numpy().copy() for p in self.p], exp_avg=g("exp_avg"),
                    exp_avg_sq=g("exp_avg_sq"), colstats=None if self.stand is None else self.stand.colstats.copy())


class Twin:
    """The whole agent: tests/iq_restate.py's SoftQ (the critic, its target, its Adam, its two Standardizers), a Policy and
    the temperature.  wrong: None, "critic_stats_untouched" (the policy update leaves the critic's Standardizer alone) or
    "alpha_from_first_pass" (on a logging iteration _update_alpha takes update_policy's FIRST log-probabilities): the two
    readings the fixtures must tell from the reference."""

    def __init__(self, pparams, cparams, central, delta, cfg, qcfg=None, dtype=torch.float64, wrong=None):
        self.cfg, self.dtype, self.wrong = cfg, dtype, wrong
        qcfg = qcfg if qcfg is not None else Q.Cfg(standardizer=cfg.standardizer)
        self.q = Q.SoftQ(cparams, qcfg, dtype)
        self.pi = Policy(pparams, central, delta, cfg, dtype)
        self.log_alpha = torch.tensor(float(np.float32(np.log(cfg.init_alpha))), dtype=dtype, requires_grad=True)
        self.aopt = torch.optim.Adam([self.log_alpha], lr=cfg.lr_alpha)
        self.target_entropy = -float(self.pi.A) if cfg.target_entropy is None else float(cfg.target_entropy)
        self.iter = 1
        self.scalars = {}

    @property
    def alpha(self):
        return self.log_alpha.detach().exp()

    def critic(self, x, a_new):
        """The live critic on (x | a_new): FullyConnectedNetwork.forward adds the concatenated float32 rows to the critic's
        Standardizer and standardises with statistics that include them; the row itself carries the gradient."""
        dt, st = self.dtype, self.q.stand
        xa = torch.cat([torch.as_tensor(np.asarray(x, np.float32)).to(dt), a_new], dim=1)
        if st is not None:
            if self.wrong != "critic_stats_untouched":
                st(xa.detach().to(torch.float32).numpy())
            mean, std = _moments(st)
            xa = ((xa.double() - torch.as_tensor(mean)) / torch.as_tensor(std)).to(dt)
        return self.q._net(self.q.p, xa)

    def policy_step(self, x, eps):
        """Steps 1 to 4: returns ([Actor/Loss, the gradient's norm, mean(log_prob), mean(q)] f64, a_new, log_prob)."""
        a_new, logp = self.pi.act(x, eps)
        q = self.critic(x, a_new)                               # [Bp, 1]
        loss = (self.alpha * logp - q).mean()                   # [Bp] - [Bp, 1]: the reference's broadcast (:589)
        self.pi.opt.zero_grad()                                 # RESTATEMENT of DeepAC._optimize_actor_parameters
        for p in self.q.p:
            p.grad = None
        loss.backward()
        self.pi.opt.step()
        norm = torch.cat([p.grad.reshape(-1) for p in self.pi.p]).double().norm()
        out = np.array([float(loss.detach().double()), float(norm), float(logp.detach().double().mean()),
                        float(q.detach().double().mean())])
        return out, a_new.detach(), logp.detach()

    def alpha_step(self, logp):
        """_update_alpha (:591-595)."""
        loss = -(self.log_alpha.exp() * (torch.as_tensor(logp).to(self.dtype) + self.target_entropy)).mean()
        self.aopt.zero_grad()
        loss.backward()
        self.aopt.step()

    def update_policy(self, obs, n_policy, eps, logging):
        """update_policy (:431-465).  eps: dict(pi [Bp,A], log [B,A] on a logging iteration)."""
        x = obs[:n_policy] if self.cfg.own_states else obs
        out, _, logp = self.policy_step(x, eps["pi"])
        first = logp
        if logging:
            row = self.scalars.setdefault(self.iter, {})
            row[PI_TAGS[1]], row[PI_TAGS[0]] = out[1], out[0]
            with torch.no_grad():
                _, logp = self.pi.act(obs, eps["log"])
                row[LOG_TAGS[0]] = float((-logp[n_policy:]).double().mean())
                row[LOG_TAGS[1]] = float((-logp[:n_policy]).double().mean())
                _, ls = self.pi.mu_log_sigma(obs[:n_policy])
                row[LOG_TAGS[2]] = float(self.pi.entropy_from_logsigma(ls).double().mean())
                row[LOG_TAGS[3]] = self.cfg.e_thres - self.pi.iter * self.cfg.e_reduc
                _, ls = self.pi.mu_log_sigma(obs[n_policy:])
                row[LOG_TAGS[4]] = float(self.pi.entropy_from_logsigma(ls).double().mean())
        if self.cfg.learnable:
            self.alpha_step(first if self.wrong == "alpha_from_first_pass" else logp)
        return out

    def iq_update(self, s, n_policy, eps, logging=True):
        """One iq_update (:408-419) and fit's counters (:405-406) on a batch s = dict(obs, act, next_obs, absorbing).  eps:
        dict(next, pi, expert: update_Q_function's passes; ppi, plog: update_policy's).  The policy passes of the critic
        update are the policy's own, in the reference's order (as DeviceIQLearn.update_Q_function issues them).  Returns
        (the critic's 16 scalars, the policy's 4)."""
        c = self.q.cfg
        self.q.cfg = c = c._replace(alpha=float(self.alpha))
        obs = s["obs"]
        f = lambda t: t.detach().to(torch.float32).numpy()
        with torch.no_grad():
            a_next, lp_next = (f(t) for t in self.pi.act(s["next_obs"], eps["next"]))
            a_pi = lp_pi = None
            if logging and c.algo == "iq":
                self.pi.act(obs[n_policy:], eps["expert"])
            if Q.has_v(c):
                a_pi, lp_pi = (f(t) for t in self.pi.act(obs, eps["pi"]))
            if logging and c.algo != "iq":
                self.pi.act(obs[n_policy:], eps["expert"])
        out_q = self.q.update(obs, s["act"], s["next_obs"], s["absorbing"], a_next, lp_next, a_pi, lp_pi, n_policy)
        out_pi = self.update_policy(obs, n_policy, dict(pi=eps["ppi"], log=eps.get("plog")), logging)
        self.iter += 1
        self.pi.iter += 1
        return out_q, out_pi

    def alpha_block(self):
        st = self.aopt.state.get(self.log_alpha, {})
        g = lambda k: float(st[k].double()) if k in st else 0.0
        return np.array([float(self.log_alpha.detach().double()), g("exp_avg"), g("exp_avg_sq")])

    def state(self):
        return dict(policy=self.pi.state(), critic=self.q.state(), alpha=self.alpha_block())


def alpha_adam(log_prob_steps, target_entropy, lr, init=INIT_ALPHA, dtype=torch.float64):
    """The [3] block (log_alpha, exp_avg, exp_avg_sq) after one _update_alpha per entry of log_prob_steps."""
    la = torch.tensor(float(np.float32(np.log(init))), dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([la], lr=lr)
    for lp in log_prob_steps:
        loss = -(la.exp() * (torch.as_tensor(np.asarray(lp, np.float32)).to(dtype) + target_entropy)).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    st = opt.state[la]
    return np.array([float(la.detach()), float(st["exp_avg"]), float(st["exp_avg_sq"])], np.float64)


def alpha_err(got, want):
    """How far the [3] block `got` lies from `want`: log_alpha absolutely, the two moments relative to their own size
    (exp_avg_sq is of the order alpha^2: an absolute bound would not see it)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rel = [abs(g - w) / abs(w) if w != 0.0 else abs(g) for g, w in zip(got[1:], want[1:])]
    return float(max([abs(got[0] - want[0])] + rel))


# ---------------------------------------------------------------------------------------------- the GPU test's cases
# (in, A, Bp): one row; the obs | act seam inside a 16-wide tile; full tiles; two output column tiles; a ragged last tile.
SHAPES = ((1, 1, 1), (12, 5, 18), (16, 16, 16), (32, 11, 48), (48, 16, 33))
UPDATES, SWEEP_EPS = 3, 1e-5
# Two configs per shape: both Standardizers and a weight decay; neither.  Adam's eps is 1e-5 here, as in
# tests/iq_restate.py's sweep and for its reason (an entry whose gradient nearly cancels moves by lr / eps times a rounding
# of the gradient; at 1e-8 torch's own float32 run cannot be held to TOL / 4); the fixtures keep torch's default 1e-8.
# The clamp is [-3, -0.5] here (the fixtures keep [-20, 2]), for the sake of this sweep's conditioning check, which is
# torch's own all-float32 run (tests/test_iq_pi_cpu.py holds it within TOL / 4): a column clamped at log_std_max = 2 has
# sigma = 7.4, its tanh saturates and 1 - a^2 + 1e-6 evaluated IN FLOAT32 strays from float64 by 1e-3 on a parameter, so
# that run could not vouch for such a case.  With sigma <= 0.61 no entry saturates.  The kernels form that term in fp64
# and are held at the agents' clamp [-20, 2] with saturated entries by the tables of tests/sg_saturation.py
# (tests/test_sg_saturation_cpu.py, tests/test_gpu_sg_saturation.py), whose conditioning check is a float32 run with
# the kernels' fp64 epilogue.
SWEEP_LS = (-3.0, -0.5)
CONFIGS = (PiCfg(standardizer=True, wd=1e-4, adam_eps=SWEEP_EPS, ls_min=SWEEP_LS[0], ls_max=SWEEP_LS[1]),
           PiCfg(standardizer=False, adam_eps=SWEEP_EPS, ls_min=SWEEP_LS[0], ls_max=SWEEP_LS[1]))
ALPHA = 0.2          # the sweep's temperature: both terms of the loss weigh in the gradient


def cfg_id(c):
    return ("std" if c.standardizer else "nostd") + ("-wd" if c.wd else "")


def case_inputs(in_dim, A, Bp, seed, updates=UPDATES):
    """dict(steps: per update dict(x [Bp,in] f32 with a scale and a shift per column, eps [Bp,A] f32), pparams, cparams
    (nn.Linear's default initialisation; the policy's output weights scaled by 0.3 and its log_sigma bias moved to -1.5,
    column 0's to 1 (above the sweep's log_std_max) and, with A > 2, column 2's to -6 (below its log_std_min): clamped
    columns beside unclamped ones), central, delta f32 of unequal
    widths), rebuilt from the seed."""
    rng = np.random.default_rng(7000 + seed)
    scale, shift = _columns(rng, in_dim)
    steps = [dict(x=(rng.standard_normal((Bp, in_dim)) * scale + shift).astype(np.float32),
                  eps=rng.standard_normal((Bp, A)).astype(np.float32)) for _ in range(updates)]
    min_a, max_a = -rng.uniform(0.5, 2.0, A), rng.uniform(0.5, 3.0, A)
    pparams = linear_params([(in_dim, 512), (512, 256), (256, 2 * A)], seed)
    cparams = linear_params([(in_dim + A, 512), (512, 256), (256, 1)], 100 + seed)
    pparams[4] *= np.float32(0.3)
    pparams[5][A:] -= np.float32(1.5)
    if A > 1:
        pparams[5][A + 0] = 1.0
    if A > 2:
        pparams[5][A + 2] = -6.0
    return dict(steps=steps, pparams=pparams, cparams=cparams, central=(0.5 * (max_a + min_a)).astype(np.float32),
                delta=(0.5 * (max_a - min_a)).astype(np.float32))


def run(case, cfg, dtype=torch.float64, alpha=ALPHA, act=None):
    """The policy steps of `case` in order: (state after the last, out [updates, 4], a_new and log_prob of every step).
    act(policy, x, eps), if given, stands in for Policy.act (tests/sg_saturation.py's mixed-precision model and its wrong
    readings)."""
    t = Twin(case["pparams"], case["cparams"], case["central"], case["delta"], cfg._replace(init_alpha=alpha), dtype=dtype)
    if act is not None:
        t.pi.act = lambda x, eps: act(t.pi, x, eps)
    outs, acts = [], []
    for s in case["steps"]:
        o, a, lp = t.policy_step(s["x"], s["eps"])
        outs.append(o)
        acts.append((a.double().numpy(), lp.double().numpy()))
    return t.state(), np.asarray(outs), acts


_CACHE = {}


def sweep_inputs(k):
    if ("in", k) not in _CACHE:
        in_dim, A, Bp = SHAPES[k]
        _CACHE[("in", k)] = case_inputs(in_dim, A, Bp, seed=20 + k)
    return _CACHE[("in", k)]


def yardstick(k, j):
    """(float64 state, out, acts, float32 state, out, acts) of config j at shape k, computed once and shared."""
    if (k, j) not in _CACHE:
        case = sweep_inputs(k)
        _CACHE[(k, j)] = run(case, CONFIGS[j]) + run(case, CONFIGS[j], torch.float32)
    return _CACHE[(k, j)]


def sweep_facts(k, j):
    """What the table must hold at (shape k, config j), measured on the float64 run's first step: the number of clamped
    and unclamped log_sigma entries, of dead relu units (no row activates them) in the policy's and the critic's layers."""
    case, cfg = sweep_inputs(k), CONFIGS[j]
    t = Twin(case["pparams"], case["cparams"], case["central"], case["delta"], cfg._replace(init_alpha=ALPHA))
    s = case["steps"][0]
    A = SHAPES[k][1]
    with torch.no_grad():
        z = t.pi.stand(s["x"]) if t.pi.stand is not None else s["x"]
        z = torch.as_tensor(z).double()
        h1 = torch.relu(z @ t.pi.p[0].T + t.pi.p[1])
        h2 = torch.relu(h1 @ t.pi.p[2].T + t.pi.p[3])
        y = h2 @ t.pi.p[4].T + t.pi.p[5]
        mu, raw = y[:, :A], y[:, A:]
        cut = (raw < cfg.ls_min) | (raw > cfg.ls_max)
        sigma = torch.clamp(raw, cfg.ls_min, cfg.ls_max).exp()
        a_new = torch.tanh(mu + sigma * torch.as_tensor(s["eps"]).double()) * t.pi.delta + t.pi.central
        xa = torch.cat([torch.as_tensor(s["x"]).double(), a_new], 1)
        if t.q.stand is not None:
            t.q.stand(xa.float().numpy())
            mean, std = _moments(t.q.stand)
            xa = (xa - torch.as_tensor(mean)) / torch.as_tensor(std)
        c1 = torch.relu(xa @ t.q.p[0].T + t.q.p[1])
        c2 = torch.relu(c1 @ t.q.p[2].T + t.q.p[3])
    dead = lambda h: int((h <= 0).all(dim=0).sum())
    return dict(clamped=int(cut.sum()), unclamped=int((~cut).sum()), dead_policy=dead(h1) + dead(h2),
                dead_critic=dead(c1) + dead(c2))


def cat(xs):
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])
