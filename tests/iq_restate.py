"""The yardstick of K26 (oly_iq_q_update, csrc/k26_iq_critic.hip): IQ_SAC.update_Q_function with _update_all_targets
(imitation_lib/imitation/iq_sac.py:421-429, 467-595, 674-676) and SQIL's loss (imitation_lib/imitation/sqil_sac.py:64-136)
restated with torch autograd and torch.optim.Adam, the Standardizers in numpy float64 pass by pass as networks.py:68-81
feeds them, in float64 (the yardstick) or float32 (what the reference runs).  The policy's actions and log-probabilities
are inputs here, as they are inputs of the kernel.  No tests here: tests/test_iq_cpu.py holds this file against the
fixtures of tests/golden/gen_iq_q_update.py (which executes the reference's own lines), tests/test_gpu_iq_q.py runs the
kernel against it.

_update_target is mushroom-rl's DeepAC._update_target RESTATED from its published definition (mushroom-rl is not
installed): per weight array, float32 arrays times a Python float, tau * online + (1 - tau) * target, i.e.
f32(tau) * w + f32(1 - tau) * t with two float32 products and one add."""
from collections import namedtuple

import numpy as np
import torch

from bc_restate import Standardizer
from il_shapes import TOL, _columns, linear_params  # noqa: F401  (TOL is re-exported to the tests)

IQ_MODES = ("value", "value_expert", "value_policy", "q_old_policy")
REG_MODES = ("exp_and_plcy", "exp", "plcy", "off")
SQIL_MODES = ("plcy", "value", "value_plcy")
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")

Cfg = namedtuple("Cfg", "algo mode reg treat use_target standardizer gamma alpha reg_mult R_min R_max lr tau wd "
                        "update_target adam_eps", defaults=("iq", "value", "exp_and_plcy", False, True, True, 0.99,
                                                            float(np.exp(np.float32(np.log(1e-3)))), 0.5, 0.0, 1.0, 3e-4,
                                                            0.005, 0.0, True, 1e-8))


def has_v(cfg):
    """Whether the update runs the pass Q(obs | a_pi): always for IQ, for SQIL unless plcy_loss_mode is plcy."""
    return cfg.algo == "iq" or cfg.mode != "plcy"


class SoftQ:
    """The live critic, its target, Adam and the two Standardizers.  wrong: None, "one_stats" (the statistics take every
    pass's rows first and all passes are standardised alike) or "shared_target" (the target goes through the live
    Standardizer): the two readings the fixtures must tell from the reference."""

    def __init__(self, params, cfg, dtype=torch.float64, wrong=None, target=None):
        self.cfg, self.dtype, self.wrong = cfg, dtype, wrong
        self.p = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in params]
        self.t = [torch.tensor(np.asarray(a), dtype=dtype) for a in (params if target is None else target)]
        D = int(self.p[0].shape[1])
        self.stand = Standardizer(D) if cfg.standardizer else None
        self.tstand = Standardizer(D) if cfg.standardizer else None
        self.opt = torch.optim.Adam(self.p, lr=cfg.lr, betas=(0.9, 0.999), eps=cfg.adam_eps, weight_decay=cfg.wd)
        self.grad_passes = []

    def _net(self, ps, z):
        z = torch.relu(z @ ps[0].T + ps[1])
        z = torch.relu(z @ ps[2].T + ps[3])
        return z @ ps[4].T + ps[5]

    def forward(self, x, target=False, frozen=None):
        """FullyConnectedNetwork.forward on the concatenated float32 rows x: the network's Standardizer takes them, then
        f32((f64(x) - mean) / std) goes through the layers."""
        ps = self.t if target else self.p
        st = self.tstand if (target and self.wrong != "shared_target") else self.stand
        if frozen is not None:
            z = frozen(x)
        elif st is not None:
            z = st(x)
        else:
            z = np.asarray(x, np.float32)
        return self._net(ps, torch.as_tensor(z).to(self.dtype))

    def update(self, obs, act, next_obs, absorbing, a_next, logp_next, a_pi, logp_pi, n_policy):
        """One update_Q_function and _update_all_targets; returns the 16 scalars of oly_iq_q_update as float64."""
        c, dt = self.cfg, self.dtype
        B = len(obs)
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        x0, x1 = np.concatenate([obs, act], 1), np.concatenate([next_obs, a_next], 1)
        x2 = np.concatenate([obs, a_pi], 1) if has_v(c) else None
        frozen = None
        if self.wrong == "one_stats" and self.stand is not None:
            for x in (x0, x1, x2) if not c.use_target else (x0, x2):
                if x is not None:
                    self.stand(x)
            cnt = self.stand.colstats[0] + 1e-2
            mean = self.stand.colstats[1] / cnt
            std = np.sqrt(np.maximum((self.stand.colstats[2] + 1e-2) / cnt - np.square(mean), 1e-2))
            frozen = lambda x: ((np.asarray(x, np.float64) - mean) / std).astype(np.float32)
        exp = torch.arange(B) >= n_policy
        ab = t(absorbing).reshape(B, 1)
        alpha, gamma = t(c.alpha), t(c.gamma)
        Q = self.forward(x0, frozen=frozen)
        if c.use_target:
            with torch.no_grad():
                nq = self.forward(x1, target=True)
        else:
            nq = self.forward(x1, frozen=frozen)
        next_v = nq - alpha * t(logp_next).reshape(B, 1)
        y = (1 - ab) * gamma * next_v
        reward = Q - y
        V = None
        if x2 is not None:
            V = self.forward(x2, frozen=frozen) - alpha * t(logp_pi).reshape(B, 1)
        out = np.zeros(16)
        if c.algo == "iq":
            loss1 = -reward[exp].mean()
            value = V - y
            loss2 = {"value": lambda: value.mean(), "value_expert": lambda: value[exp].mean(),
                     "value_policy": lambda: value[~exp].mean(), "q_old_policy": lambda: reward[~exp].mean()}[c.mode]()
            ra = ab if c.treat else torch.zeros_like(ab)
            w = (1 - ra) * c.reg_mult + ra * (1.0 - gamma) * c.reg_mult
            chi = w * torch.square(reward)
            chi2 = {"exp_and_plcy": lambda: chi.mean(), "exp": lambda: chi[exp].mean(), "plcy": lambda: chi[~exp].mean(),
                    "off": lambda: torch.zeros((), dtype=dt)}[c.reg]()
            loss = loss1 + loss2 + chi2
            out[0], out[1], out[2] = (float(v.detach()) for v in (loss1, loss2, chi2))
        else:
            loss = 0.5 * torch.mean(torch.square(Q[exp] - (c.R_max + y[exp])))
            if c.mode == "value":
                loss = loss + 0.5 * torch.mean(torch.square(V - (c.R_min + y)))
            elif c.mode == "value_plcy":
                loss = loss + 0.5 * torch.mean(torch.square(V[~exp] - (c.R_min + y[~exp])))
            else:
                loss = loss + 0.5 * torch.mean(torch.square(Q[~exp] - (c.R_min + y[~exp])))
            loss = loss * c.reg_mult
            out[0] = float(loss.detach())
        self.opt.zero_grad()
        loss.backward()
        out[15] = float(torch.cat([p.grad.reshape(-1) for p in self.p]).double().norm())
        self.opt.step()
        with torch.no_grad():
            d = lambda v: v.detach().double()
            Qd, yd, rd, a_ = d(Q), d(y), d(reward), ab.reshape(-1) != 0
            out[3] = float(d(V).mean()) if V is not None else 0.0
            out[4], out[5] = float(Qd[exp].mean()), float(torch.square(Qd[exp]).mean())
            out[6], out[7] = float(Qd[~exp].mean()), float(torch.square(Qd[~exp]).mean())
            out[8], out[9], out[10] = float(rd.mean()), float(rd[exp].mean()), float(rd[~exp].mean())
            out[11], out[12] = float(yd[exp].mean()), float(yd[~exp].mean())
            out[13] = float(Qd[exp][a_[exp]].mean()) if bool(a_[exp].any()) else np.nan
            out[14] = float(Qd[~exp][a_[~exp]].mean()) if bool(a_[~exp].any()) else np.nan
            if c.update_target:
                self.t = [update_target(c.tau, p.detach(), q) for p, q in zip(self.p, self.t)]
        return out

    def state(self):
        """dict(params, target, exp_avg, exp_avg_sq: six float64 arrays each; colstats, tcolstats [3,D] or None)."""
        z = lambda p: np.zeros(tuple(p.shape))
        g = lambda k: [self.opt.state[p][k].double().numpy().copy() if p in self.opt.state else z(p) for p in self.p]
        return dict(params=[p.detach().double().numpy().copy() for p in self.p],
                    target=[q.double().numpy().copy() for q in self.t], exp_avg=g("exp_avg"), exp_avg_sq=g("exp_avg_sq"),
                    colstats=None if self.stand is None else self.stand.colstats.copy(),
                    tcolstats=None if self.tstand is None else self.tstand.colstats.copy())


def update_target(tau, w, t):
    """RESTATEMENT of mushroom-rl's DeepAC._update_target for one weight array (see the module docstring)."""
    if w.dtype == torch.float32:
        r = np.float32(tau) * w.numpy() + np.float32(1 - tau) * t.numpy()
        assert r.dtype == np.float32
        return torch.from_numpy(r)
    return tau * w + (1 - tau) * t


# ---------------------------------------------------------------------------------------------- the GPU test's cases
def case_inputs(in_dim, A, B, seed, updates=3, absorbing_frac=0.2):
    """Per update dict(obs, act, next_obs [B,.] f32 with a scale and a shift per column, absorbing [B] f32 (about a fifth
    of the rows), a_next, a_pi [B,A] f32 in (-1, 1), logp_next, logp_pi [B] f32), rebuilt from the seed; and the critic's
    initial parameters (nn.Linear's default initialisation, the output layer as drawn)."""
    rng = np.random.default_rng(5000 + seed)
    scale, shift = _columns(rng, in_dim)
    f = np.float32
    steps = []
    for _ in range(updates):
        obs = (rng.standard_normal((B, in_dim)) * scale + shift).astype(f)
        nxt = (obs + 0.1 * rng.standard_normal((B, in_dim)) * scale).astype(f)
        steps.append(dict(obs=obs, next_obs=nxt, act=np.tanh(rng.standard_normal((B, A))).astype(f),
                          absorbing=(rng.uniform(0, 1, B) < absorbing_frac).astype(f),
                          a_next=np.tanh(rng.standard_normal((B, A))).astype(f),
                          a_pi=np.tanh(rng.standard_normal((B, A))).astype(f),
                          logp_next=(rng.standard_normal(B) * 2 - A).astype(f),
                          logp_pi=(rng.standard_normal(B) * 2 - A).astype(f)))
    return steps, linear_params([(in_dim + A, 512), (512, 256), (256, 1)], seed)


def run(params, cfg, steps, n_policy, dtype=torch.float64, wrong=None):
    """The updates of `steps` in order; returns (state after the last, out [updates, 16])."""
    q = SoftQ(params, cfg, dtype, wrong)
    out = [q.update(n_policy=n_policy, **s) for s in steps]
    return q.state(), np.asarray(out)


# ---------------------------------------------------------------------------------------------- the sweep's table
# (obs, A, B, n_policy): the shapes of the issue.  Every IQ loss mode x regularizer mode x treat_absorbing x use_target and
# the three SQIL modes x use_target make 70 configs; config j runs at shape j % 5 for UPDATES updates, so the five shapes
# together run every one.  The Standardizers and a weight decay alternate over the list.
#
# Adam's eps is 1e-5 here (the fixtures keep torch's default 1e-8).  The step of an entry is lr m / (sqrt(v) + eps): where
# the entry's gradient nearly cancels, its derivative with respect to the gradient is lr / eps = 3e4 at eps = 1e-8, and a
# float32 rounding of the gradient (1e-9) moves the parameter by more than TOL.  Measured on the CPU, without any kernel:
# at eps = 1e-8 torch's own float32 run of this table strays from float64 by up to 2.4e-4 on a parameter (the regularizer
# "off" configs, whose coefficients are constants and whose gradients cancel most), at eps = 1e-5 by less than 1e-6 on
# every config but one.  A case that float32 itself cannot hold to TOL / 4 cannot tell a kernel from a rounding;
# tests/test_iq_cpu.py asserts that no case of the table is one.  Config 63 (q_old_policy, off, treat_absorbing, no
# target) strays by 4.8e-4 at its own shape 3 (a relu changes side between float32 and float64) and by 2.5e-7 at shape 4,
# so it runs there.
SHAPES = ((1, 1, 2, 1), (12, 5, 18, 9), (16, 16, 16, 8), (32, 11, 48, 24), (48, 16, 33, 1))
UPDATES, SWEEP_EPS = 3, 1e-5
MOVED = {63: 4}


def sweep_configs():
    out = []
    for mode in IQ_MODES:
        for reg in REG_MODES:
            for treat in (False, True):
                for tgt in (True, False):
                    out.append(Cfg(algo="iq", mode=mode, reg=reg, treat=treat, use_target=tgt))
    for mode in SQIL_MODES:
        for tgt in (True, False):
            out.append(Cfg(algo="sqil", mode=mode, use_target=tgt, R_min=-0.25, R_max=1.5))
    return [c._replace(standardizer=(i // 5) % 2 == 0, wd=1e-4 if i % 3 == 0 else 0.0, tau=0.05, adam_eps=SWEEP_EPS)
            for i, c in enumerate(out)]


CONFIGS = sweep_configs()


def sweep(k):
    """[(number, config)] of the configs that run at shape k."""
    return [(j, c) for j, c in enumerate(CONFIGS) if MOVED.get(j, j % len(SHAPES)) == k]


def cfg_id(c):
    return f"{c.algo}-{c.mode}-{c.reg}-{'abs' if c.treat else 'noabs'}-{'tgt' if c.use_target else 'notgt'}" + \
        ("" if c.standardizer else "-nostd")


_CACHE = {}


def sweep_inputs(k):
    """(steps, params) of shape k, rebuilt from its seed once; callers leave them unchanged.  At B = 2 the policy's row
    is absorbing and the expert's is not: an empty absorbing subset, NaN in the reference as in the kernel."""
    if ("in", k) not in _CACHE:
        in_dim, A, B, _ = SHAPES[k]
        steps, params = case_inputs(in_dim, A, B, seed=10 + k, updates=UPDATES)
        if B == 2:
            for s in steps:
                s["absorbing"][:] = (1.0, 0.0)
        _CACHE[("in", k)] = (steps, params)
    return _CACHE[("in", k)]


def yardstick(k, j):
    """(float64 state, float64 out, float32 state, float32 out) of config j at shape k, computed once and shared."""
    if (k, j) not in _CACHE:
        steps, params = sweep_inputs(k)
        n_policy = SHAPES[k][3]
        _CACHE[(k, j)] = run(params, CONFIGS[j], steps, n_policy) + run(params, CONFIGS[j], steps, n_policy, torch.float32)
    return _CACHE[(k, j)]


def cat(xs):
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])
