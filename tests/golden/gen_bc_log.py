#!/usr/bin/env python3
"""Generate tests/golden/bc_log/bc_log.npz: gen_bc_fit.py's fit (the reference's own FullyConnectedNetwork and
Standardizer from imitation_lib/utils/networks.py under the inert stubs of _ref_stubs.py, 32 -> [512, 256] -> 22, 200
rows, batch 32, 6 steps, Adam(lr=1e-3) over GaussianNLLLoss) with the WHOLE of BehavioralCloning.logging()
(imitation_lib/imitation/offline/behavioral_cloning.py:82-94).  Run in the build container only:

    python tests/golden/gen_bc_log.py [--out DIR]

Every logging_iter iterations logging() calls policy.compute_action_and_log_prob(states): a second forward of the
minibatch through the reference network, AFTER the optimiser's step.  The Standardizer takes the rows a second time
(networks.py:68-81), the weights are the stepped ones, and -mean(log_prob) of a sample is "Squashed Gaussian Entropy
(Empirical)".  Two runs are stored: logging_iter = 1 (every minibatch enters the statistics twice) and logging_iter = 2
(iterations 0, 2, 4 do).

mushroom-rl is absent, so what goes through it is RESTATED and marked, as in gen_bc_fit.py; in addition
compute_action_and_log_prob_t (imitation_lib/imitation/iq_sac.py:117-128): distribution() is torch's Normal on
get_mu_log_sigma's output, the lines after it are copied in meaning.  The forward, the Standardizer, the loss, backward,
Adam and the sample are the reference network's and torch's own.

The noise: torch's generator state is saved before dist.rsample() and the same standard normal is drawn again from the
restored state (Normal.rsample is loc + eps * scale with eps = torch.empty(shape).normal_()); the generator asserts that
mu + sigma * eps reproduces the sample bit for bit, and stores eps.

Asserted here, on the CPU, for both runs:
  * |a_raw| < 4 and log_std_min < log_sigma < log_std_max strictly at every logged step (the log-probability is then
    well conditioned, tests/test_gpu_bc_fit.py::test_policy_log_prob_against_float64's docstring);
  * a reading that forwards the logged minibatch with the PRE-step weights misses a logged entropy by at least 10 of the
    entropy tolerance max(TOL max(1, |value|), 4 ent_spread), TOL = 2e-5;
  * a reading that adds the logged rows to the Standardizer ONCE misses the final parameters by at least 10 TOL.
Both held at the first setting tried (lr = 1e-3, 6 steps): neither was raised.

The float64 twin: every logged entropy is also evaluated in float64 from the same float32 parameters, standardised rows
and eps; ent_spread is the largest |float32 - float64| over both runs (the reference run's own rounding, measured
without any kernel).

One departure from gen_bc_fit.py's setup, needed for the first assertion: the output layer's initial weight is scaled by
W3_SCALE and the log_sigma half of its bias shifted by LOG_SIGMA_SHIFT (see there).

Layer 2's weight is handled as in gen_bc_fit.py (a seeded numpy draw, not stored); the archive has fixed member dates:
running the generator again reproduces the file byte for byte.  The fixture holds data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "bc_log")
if __name__ == "__main__" and "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]
sys.path.insert(0, HERE)
import gen_bc_fit as fit  # noqa: E402  (the setup: constants, inputs(), w2_init(), write_npz())

N_ROWS, IN_DIM, ACT_DIM, BATCH, N_STEPS, LR = fit.N_ROWS, fit.IN_DIM, fit.ACT_DIM, fit.BATCH, fit.N_STEPS, fit.LR
LOG_STD_MIN, LOG_STD_MAX = fit.LOG_STD_MIN, fit.LOG_STD_MAX
NAMES = fit.NAMES
LOGGING_ITERS = (1, 2)
TOL = 2e-5
# The one departure from gen_bc_fit.py's setup.  At the class's default initialisation (xavier with relu's gain on the
# output layer too) log_sigma reaches 1.77 and |a_raw| 11 on these rows: 1 - tanh(a_raw)^2 + 1e-6 then loses its digits in
# float32, in torch as anywhere.  The output layer starts ten times smaller, with log_sigma about -0.5.
W3_SCALE, LOG_SIGMA_SHIFT = 0.1, -0.5
EPS_LOG_PROB = 1e-6          # IQ_Learn_Policy._eps_log_prob (iq_sac.py:48)


def initial_params(g):
    """The six initial tensors from the fixture `g` and gen_bc_fit.w2_init()."""
    return [fit.w2_init() if n == "w2" else g[f"init_{n}"] for n in NAMES]


def ent_tol(value, ent_spread):
    return max(TOL * max(1.0, abs(float(value))), 4.0 * float(ent_spread))


def run(ns, logging_iter, idx, reading="true", eps_given=None):
    """One fit.  reading: "true" (the reference), "prestep" (the logged forward with the weights before the step) or
    "once" (the logged forward does not feed the Standardizer).  Returns dict(init, params, scalars [6,4] (loss, entropy, mse, sampled entropy or NaN), eps
    [n_logged,32,11], st_sum / st_sumsq / st_count, ent64 [n_logged]: the float64 twins, worst_raw, ls: the extremes)."""
    import torch
    from torch.nn import GaussianNLLLoss
    nw = ns.networks
    torch.manual_seed(5)
    stand = nw.Standardizer()
    net = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(2 * ACT_DIM,), n_features=[512, 256],
                                   activations=["relu", "relu", "identity"], standardizer=stand, squeeze_out=False)
    with torch.no_grad():
        net._linears[1].weight.copy_(torch.from_numpy(fit.w2_init()))
        net._linears[2].weight.mul_(W3_SCALE)
        net._linears[2].bias[ACT_DIM:].add_(LOG_SIGMA_SHIFT)
    states, actions, min_a, max_a = fit.inputs()

    def params():
        return {n: t.detach().numpy().copy() for n, t in zip(NAMES, [p for lin in net._linears for p in (lin.weight, lin.bias)])}
    init = params()
    # ---- RESTATEMENT (mushroom-rl pieces): to_float_tensor(.5 * (max_a -+ min_a)), iq_sac.py:43-44
    delta_a = torch.as_tensor(0.5 * (max_a - min_a), dtype=torch.float32)
    central_a = torch.as_tensor(0.5 * (max_a + min_a), dtype=torch.float32)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    actor_loss = GaussianNLLLoss()
    torch.manual_seed(31 + logging_iter)       # the sampling generator of this run
    scalars, eps_all, ent64, worst_raw, ls_lo, ls_hi = [], [], [], 0.0, np.inf, -np.inf

    def get_mu_log_sigma(s):
        # RESTATEMENT of get_mu_log_sigma (iq_sac.py:132-151): the Regressor's predict is the network's forward
        y = net(s)
        return y[:, 0:ACT_DIM], torch.clamp(y[:, ACT_DIM:2 * ACT_DIM], LOG_STD_MIN, LOG_STD_MAX)

    for i in range(N_STEPS):
        # RESTATEMENT: next(minibatch_generator(batch_size, states, actions, ...)), to_float_tensor
        s = torch.as_tensor(states[idx[i]], dtype=torch.float32)
        target_actions = torch.as_tensor(actions[idx[i]], dtype=torch.float32)
        # behavioral_cloning.py:63-66
        target_actions = torch.clip((target_actions - central_a) / delta_a, -1.0 + 1e-7, 1.0 - 1e-7)
        target_actions = torch.arctanh(target_actions)
        mu, log_sigma = get_mu_log_sigma(s)
        # behavioral_cloning.py:71-75
        loss = actor_loss(input=mu, target=target_actions, var=torch.square(log_sigma.exp()))
        opt.zero_grad()
        loss.backward()
        before = [p.detach().clone() for p in net.parameters()]
        opt.step()
        # logging(), :82-94
        gauss_ent = ACT_DIM * (0.5 + 0.5 * np.log(2 * np.pi)) + torch.sum(log_sigma, axis=-1)     # entropy_from_logsigma
        mse = torch.nn.functional.mse_loss(mu, target_actions)
        row = [np.mean(loss.detach().numpy()), np.mean(gauss_ent.detach().numpy()), np.nan, np.mean(mse.detach().numpy())]
        if i % logging_iter == 0:
            # ---- RESTATEMENT of compute_action_and_log_prob_t (iq_sac.py:117-128) under no_grad, as
            # compute_action_and_log_prob's detach() leaves it
            with torch.no_grad():
                after = [p.detach().clone() for p in net.parameters()]
                if reading == "prestep":
                    for p, b in zip(net.parameters(), before):
                        p.copy_(b)
                if reading == "once":
                    keep = stand.update_mean_std
                    stand.update_mean_std = lambda x: None
                mu2, ls2 = get_mu_log_sigma(s)             # the second forward: the Standardizer takes the rows again
                if reading == "once":
                    stand.update_mean_std = keep
                dist = torch.distributions.Normal(mu2, ls2.exp())
                state = torch.get_rng_state()
                a_raw = dist.rsample()
                torch.set_rng_state(state)
                eps = torch.empty(a_raw.shape, dtype=torch.float32).normal_()
                if eps_given is not None:                  # the variant readings take the true run's noise
                    eps = torch.as_tensor(eps_given[len(eps_all)])
                    a_raw = mu2 + ls2.exp() * eps
                assert torch.equal(a_raw, mu2 + ls2.exp() * eps), "eps does not reproduce rsample()"
                a = torch.tanh(a_raw)
                log_prob = dist.log_prob(a_raw).sum(dim=1)
                log_prob -= torch.log(1. - a.pow(2) + EPS_LOG_PROB).sum(dim=1)
                row[2] = -np.mean(log_prob.numpy())
                # ---- end of that restatement; the float64 twin from the same float32 mu's inputs
                x64 = torch.as_tensor(((s.numpy().astype(np.float64) - stand.mean) / stand.std).astype(np.float32)).double()
                w = [p.detach().double() for p in net.parameters()]
                y64 = torch.relu(torch.relu(x64 @ w[0].T + w[1]) @ w[2].T + w[3]) @ w[4].T + w[5]
                mu64, ls64 = y64[:, :ACT_DIM], torch.clamp(y64[:, ACT_DIM:], LOG_STD_MIN, LOG_STD_MAX)
                raw64 = mu64 + ls64.exp() * eps.double()
                lp64 = torch.distributions.Normal(mu64, ls64.exp()).log_prob(raw64).sum(1)
                lp64 = lp64 - torch.log(1.0 - torch.tanh(raw64) ** 2 + EPS_LOG_PROB).sum(1)
                ent64.append(float(-lp64.mean()))
                eps_all.append(eps.numpy().copy())
                worst_raw = max(worst_raw, float(a_raw.abs().max()))
                ls_lo, ls_hi = min(ls_lo, float(ls2.min())), max(ls_hi, float(ls2.max()))
                if reading == "prestep":
                    for p, b in zip(net.parameters(), after):
                        p.copy_(b)
        # the order of the reference's add_scalar calls is loss, entropy, empirical entropy, mse; stored as
        # loss, entropy, mse, empirical entropy: oly_bc_fit_steps' three columns, then the new one
        scalars.append([row[0], row[1], row[3], row[2]])
    # ---- end of the restatement
    return dict(init=init, params=params(), scalars=np.asarray(scalars, np.float64), eps=np.asarray(eps_all, np.float32),
                st_sum=np.asarray(stand._sum, np.float64), st_sumsq=np.asarray(stand._sumsq, np.float64),
                st_count=np.asarray(stand._count, np.float64), ent64=np.asarray(ent64), worst_raw=worst_raw, ls=(ls_lo, ls_hi))


def main():
    import _ref_stubs as stubs
    ns = stubs.load_reference()
    rng = np.random.default_rng(23)
    idx = np.stack([rng.permutation(N_ROWS)[:BATCH] for _ in range(N_STEPS)]).astype(np.int32)
    runs = {li: run(ns, li, idx) for li in LOGGING_ITERS}
    ent_spread = 0.0
    for li, r in runs.items():
        logged = [s for s in range(N_STEPS) if s % li == 0]
        assert r["worst_raw"] < 4.0, r["worst_raw"]
        assert LOG_STD_MIN < r["ls"][0] and r["ls"][1] < LOG_STD_MAX, r["ls"]
        ent_spread = max(ent_spread, float(np.abs(r["scalars"][logged, 3] - r["ent64"]).max()))
        print(f"logging_iter {li}: |a_raw| max {r['worst_raw']:.3f}, log_sigma in [{r['ls'][0]:.3f}, {r['ls'][1]:.3f}], "
              f"entropy {r['scalars'][logged, 3]}")
    print(f"ent_spread {ent_spread:.3e}")
    arrays = {f"init_{n}": v for n, v in runs[1]["init"].items() if n != "w2"}
    for li, r in runs.items():
        assert all(np.array_equal(r["init"][n], runs[1]["init"][n]) for n in NAMES)
        logged = [s for s in range(N_STEPS) if s % li == 0]
        pre = run(ns, li, idx, "prestep", eps_given=r["eps"])
        once = run(ns, li, idx, "once", eps_given=r["eps"])
        sep_e = np.abs(pre["scalars"][logged, 3] - r["scalars"][logged, 3])
        tol_e = np.array([ent_tol(v, ent_spread) for v in r["scalars"][logged, 3]])
        sep_p = max(float(np.abs(once["params"][n] - r["params"][n]).max()) for n in NAMES if n != "w2")
        print(f"logging_iter {li}: pre-step reading misses the entropy by {sep_e / tol_e} tolerances; once-only reading "
              f"misses the parameters by {sep_p / TOL:.1f} TOL")
        assert (sep_e / tol_e).max() >= 10.0, "raise lr or the step count"
        assert sep_p >= 10 * TOL, "raise lr or the step count"
        arrays.update({f"{n}_li{li}": v for n, v in r["params"].items() if n != "w2"})
        arrays.update({f"scalars_li{li}": r["scalars"], f"eps_li{li}": r["eps"], f"st_sum_li{li}": r["st_sum"],
                       f"st_sumsq_li{li}": r["st_sumsq"], f"st_count_li{li}": r["st_count"],
                       f"sep_params_li{li}": np.float64(sep_p)})
    arrays.update(idx=idx, ent_spread=np.float64(ent_spread), lr=np.float64(LR), batch=np.int64(BATCH),
                  logging_iters=np.asarray(LOGGING_ITERS, np.int64))
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, "bc_log.npz")
    fit.write_npz(path, arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
