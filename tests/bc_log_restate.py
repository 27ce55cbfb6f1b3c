"""The yardstick of the logged fit (oly_bc_fit_steps_log, K24 + K25): tests/bc_restate.py's restatement of
BehavioralCloning.fit_offline with the WHOLE of logging() (imitation_lib/imitation/offline/behavioral_cloning.py:82-94).
On an iteration that logs, after the optimiser's step, compute_action_and_log_prob runs the minibatch through the network
a second time (imitation_lib/imitation/iq_sac.py:102-151): the Standardizer takes the rows again, the weights are the
stepped ones, and -mean(log_prob) of the sample mu + exp(log_sigma) eps is the step's fourth scalar.  No tests here:
tests/test_bc_log_cpu.py holds it to the reference-run fixture without a GPU, tests/test_gpu_sg_act.py runs the kernels.

Two deliberately wrong readings, which the fixture tells apart (tests/golden/gen_bc_log.py asserts the margins):
once=True feeds the Standardizer the logged rows once, prestep=True forwards them with the weights before the step."""
import numpy as np
import torch

import bc_restate as br
from il_shapes import TOL  # noqa: F401  (re-exported to the tests)

EPS_LOG_PROB = 1e-6
HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)


def ent_tol(value, ent_spread):
    """The entropy tolerance: max(TOL max(1, |value|), 4 ent_spread), ent_spread the fixture's (the reference run's own
    float32 rounding, measured by the generator against its float64 twin)."""
    return max(TOL * max(1.0, abs(float(value))), 4.0 * float(ent_spread))


def logged_steps(steps, logging_iter, iter0=0):
    return [s for s in range(steps) if (iter0 + s) % logging_iter == 0]


def log_prob(mu, log_sigma, a_raw):
    """iq_sac.py:117-128 on tensors of any dtype: Normal(mu, sigma).log_prob(a_raw) summed over the actions, minus the
    tanh correction."""
    lp = (-(a_raw - mu) ** 2 / (2 * torch.exp(log_sigma) ** 2) - log_sigma - HALF_LOG_2PI).sum(dim=1)
    return lp - torch.log(1.0 - torch.tanh(a_raw) ** 2 + EPS_LOG_PROB).sum(dim=1)


def restate(in_dim, A, k, steps, lr, standardizer, eps, logging_iter, iter0=0, dtype=torch.float64, once=False,
            prestep=False, lo=br.LOG_STD_MIN, hi=br.LOG_STD_MAX):
    """`steps` iterations on the case k = dict(params, states, targets, idx) (bc_restate.build's keys), eps
    [n_logged, batch, A] the noise of the logging steps in order.  Returns dict(params: per step the six tensors,
    colstats [3,in] or None, out [steps,4]: loss, mean entropy_from_logsigma, mse, the sampled entropy or NaN)."""
    with torch.random.fork_rng(devices=[]):
        lins = [torch.nn.Linear(i, o) for i, o in ((in_dim, 512), (512, 256), (256, 2 * A))]
    ps = [p for lin in lins for p in (lin.weight, lin.bias)]
    with torch.no_grad():
        for p, v in zip(ps, k["params"]):
            p.data = torch.as_tensor(v).to(dtype).clone()
    opt = torch.optim.Adam(ps, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    loss_fn = torch.nn.GaussianNLLLoss()
    stand = br.Standardizer(in_dim) if standardizer else None
    t_all = torch.as_tensor(k["targets"]).to(dtype)

    def forward(z):
        y = lins[2](torch.relu(lins[1](torch.relu(lins[0](z)))))
        return y[:, :A], torch.clamp(y[:, A:], lo, hi)                                  # iq_sac.py:132-151

    snaps, out, n_logged = [], [], 0
    for s in range(steps):
        rows = k["idx"][s].astype(np.int64)
        x = k["states"][rows]
        z = torch.as_tensor(stand(x) if stand is not None else x).to(dtype)
        mu, log_sigma = forward(z)
        target = t_all[rows]
        loss = loss_fn(input=mu, target=target, var=torch.square(log_sigma.exp()))
        opt.zero_grad()
        loss.backward()
        before = [p.detach().clone() for p in ps]
        opt.step()
        ent = A * (0.5 + HALF_LOG_2PI) + torch.sum(log_sigma, dim=-1)                   # entropy_from_logsigma
        mse = torch.nn.functional.mse_loss(mu, target)
        row = [float(loss.detach().double()), float(ent.detach().double().mean()), float(mse.detach().double()), np.nan]
        if (iter0 + s) % logging_iter == 0:
            with torch.no_grad():
                after = [p.detach().clone() for p in ps]
                if prestep:
                    for p, b in zip(ps, before):
                        p.copy_(b)
                if stand is not None and not once:
                    z = torch.as_tensor(stand(x)).to(dtype)      # the rows go in a second time (networks.py:68-81)
                mu2, ls2 = forward(z)
                a_raw = mu2 + ls2.exp() * torch.as_tensor(eps[n_logged]).to(dtype)
                row[3] = float(-log_prob(mu2, ls2, a_raw).double().mean())
                if prestep:
                    for p, b in zip(ps, after):
                        p.copy_(b)
            n_logged += 1
        out.append(row)
        snaps.append([p.detach().double().numpy().copy() for p in ps])
    return dict(params=snaps, exp_avg=[opt.state[p]["exp_avg"].double().numpy().copy() for p in ps],
                exp_avg_sq=[opt.state[p]["exp_avg_sq"].double().numpy().copy() for p in ps],
                colstats=None if stand is None else stand.colstats.copy(), out=np.asarray(out, np.float64))


def noise(c, logging_iter, iter0=0, seed=0):
    """eps [n_logged, batch, A] f32 for case c of bc_restate.CASES, clipped to -+2.5 as
    test_policy_log_prob_against_float64 clips it (|a_raw| stays small), rebuilt from the seed."""
    n = len(logged_steps(c.steps, logging_iter, iter0))
    rng = np.random.default_rng(7000 + 10 * c.seed + seed)
    return np.clip(rng.standard_normal((n, min(c.batch, c.n_rows), c.A)), -2.5, 2.5).astype(np.float32)


# The cases the logged fit is held to the restatement on: (1, 1, 1), (33, 11, 33) and (64, 16, 256) of bc_restate.CASES.
# The last two are tabled saturated (log_sigma columns at -9 and at the clamp's -20): there the sample
# mu + exp(log_sigma) eps formed in float32 rounds to mu and the float32 log-probability is no function of its float64
# value: torch's own float32 restatement misses the float64 entropy by 0.03 .. 0.49 on them, against a tolerance of
# 7e-4.  The entropy is therefore held on their twins without the saturation.  The twins' seed: with the tabled seeds
# the float32 restatement lay 5.6e-5 (seed 4; 11 and 12: 8.0e-6, 6.4e-6) and 4.97e-6 (seed 6) from float64 on a weight
# (an Adam step on a gradient close to zero, as bc_restate.CASES notes for its last case), above or too close to the
# TOL / 4 that tests/test_bc_log_cpu.py asks; seed 13 gives 9.0e-7 and 1.6e-6.
TABLED = (br.CASES[0], br.CASES[3], br.CASES[5])
PLAIN = (br.CASES[0], br.CASES[3]._replace(saturated=False, seed=13), br.CASES[5]._replace(saturated=False, seed=13))
RUNS = PLAIN + tuple(c for c in TABLED if c.saturated)       # the entropy tolerance on PLAIN, the rest on all of them


def logging_iter_of(c):
    return 2 if c.steps >= 3 else 1


def fixture_case(g):
    """The reference-run fixture's case in bc_restate.build's keys (tests/golden/gen_bc_log.py's setup)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_bc_log as gen
    states, actions, min_a, max_a = gen.fit.inputs()
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)
    return dict(params=gen.initial_params(g), states=states, actions=actions, central=central, delta=delta,
                targets=br.targets_of(actions, central, delta), idx=g["idx"].astype(np.int32), batch=gen.BATCH), gen
