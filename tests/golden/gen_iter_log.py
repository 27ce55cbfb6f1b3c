#!/usr/bin/env python3
"""Generate tests/golden/iter_log/{a,b}.npz by EXECUTING the reference's own _logging_sw
(imitation_lib/imitation/gail_TRPO.py:251-272) on the reference's FullyConnectedNetwork, Standardizer and NormcInitializer
(imitation_lib/utils/networks.py), imported from the reference tree under the inert stubs of _ref_stubs.py.  Run in the
build container only:

    python tests/golden/gen_iter_log.py [--out DIR]

The method is called on an instance of the reference's GAIL class made without its constructor (which needs mushroom-rl),
carrying the attributes it reads: _sw (a recording stand-in for the SummaryWriter), _iter, _train_D_n_th_epoch, _V and
policy.  mushroom-rl is absent, so these of its pieces are RESTATED (marked below), each a READING of mushroom-rl >= 1.10:
compute_J and compute_episodes_length (mushroom_rl.utils.dataset), arrays_as_dataset, Regressor.__call__ as `_V` (the
network's forward over the whole batch, [n, 1] out), and GaussianTorchPolicy with distribution / distribution_t / entropy /
entropy_t (as tests/golden/gen_trpo_step.py restates it).  Everything else is the reference's code.

Both networks are the reference's FullyConnectedNetwork(32 -> [512, 256] -> out, relu / relu / identity,
NormcInitializer(1, 1, 0.001)) sharing one Standardizer, as examples/imitation_learning/utils.py:123-149 builds them;
their weights are then replaced by a seeded draw at a trained network's scale (net_params), because the initialiser's
(unit Frobenius norm per layer) make V(x) and mu(x) all but independent of x and so of the statistics the call is about.

Cases (obs 32, act 11, std_0 0.5):
    a   T = 250, N = 4, float32 environment reward, env_reward_frac 0; `last` sprinkled from a seed and every column's
        final step closes its episode; 3000 prior rows of another distribution
    b   T = 1000, N = 1, float64 environment reward, env_reward_frac 0.3, a trailing open episode; 50 000 prior rows
The old distribution is taken as gail_TRPO.py:132-133 takes it (a deep copy of the policy, Standardizer included, whose
forward adds the batch to the COPY's statistics); then the live Standardizer takes the batch three more times (the critic
fit's updates, :152-154), the policy gets a seeded perturbation of theta and log_sigma (what a TRPO step leaves, sized so
that kl is of max_kl's order), and _logging_sw runs.  The dataset lists are passed column by column, x in the agent's
T-major row order.

Neither inputs nor weights are stored: case_args() rebuilds them from the seeds the fixture names, and the old means by
the float64 restatement narrowed to float32.  The generator checks that the mean episode length is not within 0.01 of a
half-integer and that each case holds at least three completed episodes.  One file per case, a few KiB each.
"""
import copy
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

OBS, ACT, STD_0, ITER = 32, 11, 0.5, 9
CASES = {
    "a": dict(T=250, N=4, prior_rows=3000, frac=0.0, r64=False, p_last=1 / 40, close=True, seed=71, prior_seed=81,
              net_seed=91, step_seed=101, step_scale=4e-4, ls_scale=2e-3, prior_dev=0.05),
    "b": dict(T=1000, N=1, prior_rows=50000, frac=0.3, r64=True, p_last=1 / 130, close=False, seed=72, prior_seed=82,
              net_seed=92, step_seed=102, step_scale=4e-4, ls_scale=2e-3, prior_dev=0.3),
}
SHAPES = ((512, OBS), (512,), (256, 512), (256,))


def net_params(out_dim, seed):
    """A seeded relu MLP 32 -> 512 -> 256 -> out at a trained network's scale (torch order W1, b1, W2, b2, W3, b3)."""
    rng = np.random.default_rng(seed)
    gains = (1.4, 1.4, 0.5)
    out = []
    for i, shape in enumerate(SHAPES + ((out_dim, 256), (out_dim,))):
        if i % 2 == 0:
            out.append((rng.standard_normal(shape) * gains[i // 2] / np.sqrt(shape[1])).astype(np.float32))
        else:
            out.append((rng.uniform(-1, 1, shape) * 0.1).astype(np.float32))
    return out


def stepped(case, params, log_sigma):
    """The policy after the step: the old parameters plus a seeded perturbation."""
    c = CASES[case]
    rng = np.random.default_rng(c["step_seed"])
    new = [(p + c["step_scale"] * rng.standard_normal(p.shape)).astype(np.float32) for p in params]
    return new, (log_sigma + c["ls_scale"] * rng.standard_normal(log_sigma.shape)).astype(np.float32)


def columns(case):
    """The batch's per-column (scale, shift)."""
    rng = np.random.default_rng(CASES[case]["seed"] + 1000)
    return rng.uniform(0.3, 3.0, OBS), rng.normal(0, 2, OBS)


def prior(case):
    """The rows the Standardizer has seen before the iteration: another shift and scale than the batch's, by prior_dev
    (the means of the two distributions differ by about that many batch standard deviations: beyond a few hundredths
    the drift of the statistics between the old distribution's forward and the logging's alone is a KL far above max_kl)."""
    c = CASES[case]
    scale, shift = columns(case)
    rng = np.random.default_rng(c["prior_seed"])
    dev = c["prior_dev"]
    return (rng.normal(0, 1, (c["prior_rows"], OBS)) * scale * rng.uniform(1 - dev, 1 + dev, OBS)
            + shift + dev * scale * rng.normal(0, 1, OBS)).astype(np.float32)


def inputs(case):
    """dict(x [T N, 32] in T-major row order, v_target [T N], r_env [T,N] (f32, or f64 for b), r [T,N] f32 the reward
    trained on, last [T,N] bool)."""
    c = CASES[case]
    T, N = c["T"], c["N"]
    rng = np.random.default_rng(c["seed"])
    scale, shift = columns(case)
    x = (rng.normal(0, 1, (T * N, OBS)) * scale + shift).astype(np.float32)
    v_target = (rng.normal(0, 1, T * N) + 0.5 * x[:, 0]).astype(np.float32)
    r_env = rng.uniform(0.2, 1.2, (T, N))
    r_env = r_env if c["r64"] else r_env.astype(np.float32)
    r_disc = rng.uniform(0.05, 2.0, (T, N)).astype(np.float32)
    # gail_TRPO.py:109, 124: r = reward.astype(np.float32); r = r * frac + r_disc * (1 - frac), float32 throughout
    r = r_disc if c["frac"] == 0.0 else (r_env.astype(np.float32) * np.float32(c["frac"])
                                         + r_disc * np.float32(1 - c["frac"])).astype(np.float32)
    last = rng.random((T, N)) < c["p_last"]
    last[-1] = c["close"]
    return dict(x=x, v_target=v_target, r_env=r_env, r=r, last=last)


def raw(count, s, sq):
    """Standardizer (_count, _sum, _sumsq) as raw (count, sum, sumsq) rows: the 1e-2 starting values removed."""
    cnt = np.round(float(np.asarray(count).reshape(-1)[0]) - 1e-2)
    return np.stack([np.full(OBS, cnt), np.asarray(s, dtype=np.float64), np.asarray(sq, dtype=np.float64) - 1e-2])


def case_args(case, g, device="cpu"):
    """restate_iter_log's arguments for a fixture: everything rebuilt from the seeds it names, the statistics from it."""
    import iter_log_restate as rs
    c = CASES[case]
    assert int(g["seed"]) == c["seed"] and int(g["net_seed"]) == c["net_seed"] and int(g["step_seed"]) == c["step_seed"]
    d = inputs(case)
    old = net_params(ACT, c["net_seed"] + 1)
    ls_old = np.full(ACT, np.log(STD_0), dtype=np.float32)
    policy, log_sigma = stepped(case, old, ls_old)
    mu_old = rs.old_means(old, raw(g["st_old_count"], g["st_old_sum"], g["st_old_sumsq"]), d["x"], device)
    return dict(critic=net_params(1, c["net_seed"]), policy=policy, log_sigma=log_sigma, mu_old=mu_old, ls_old=ls_old,
                colstats=raw(g["st0_count"], g["st0_sum"], g["st0_sumsq"]), **d)


class Recorder:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


def run_case(ns, case):
    import torch
    c = CASES[case]
    T, N = c["T"], c["N"]
    nw = ns.networks
    d = inputs(case)
    x, r_env, r, last = d["x"], d["r_env"], d["r"], d["last"]

    # ---- RESTATEMENT (a reading of mushroom-rl >= 1.10) of mushroom_rl.utils.dataset
    def compute_J(dataset, gamma=1.):
        js = list()
        j = 0.
        episode_steps = 0
        for i in range(len(dataset)):
            j += gamma ** episode_steps * dataset[i][2]
            episode_steps += 1
            if dataset[i][-1] or i == len(dataset) - 1:
                js.append(j)
                j = 0.
                episode_steps = 0
        if len(js) == 0:
            return [0.]
        return js

    def compute_episodes_length(dataset):
        lengths = list()
        l = 0
        for sample in dataset:
            l += 1
            if sample[-1] == 1:
                lengths.append(l)
                l = 0
        return lengths

    def arrays_as_dataset(states, actions, rewards, next_states, absorbings, lasts):
        dataset = list()
        for s, a, rr, ss, ab, la in zip(states, actions, rewards.astype('float'), next_states, absorbings.astype('bool'),
                                        lasts.astype('bool')):
            dataset.append((s, a, rr.item(0), ss, ab.item(0), la.item(0)))
        return dataset

    # ---- RESTATEMENT of mushroom-rl's GaussianTorchPolicy (>= 1.10, this project's reading; as gen_trpo_step.py)
    class GaussianTorchPolicy(torch.nn.Module):
        def __init__(self, network, action_dim, std_0):
            super().__init__()
            self._mu = network
            self._action_dim = action_dim
            self._log_sigma = torch.nn.Parameter(torch.ones(action_dim) * np.log(std_0))

        def distribution(self, state):
            return self.distribution_t(torch.as_tensor(state).float())

        def distribution_t(self, state):
            mu = self._mu(state)
            return torch.distributions.MultivariateNormal(loc=mu, scale_tril=torch.diag(torch.exp(self._log_sigma)))

        def entropy(self, state=None):
            return self.entropy_t(state).detach().cpu().numpy().item()

        def entropy_t(self, state=None):
            return self._action_dim / 2 * np.log(2 * np.pi * np.e) + torch.sum(self._log_sigma)

        def parameters(self):
            return itertools.chain(self._mu.parameters(), [self._log_sigma])
    # ---- end of the restatements

    def network(out_dim, params, stand):
        net = nw.FullyConnectedNetwork(input_shape=(OBS,), output_shape=(out_dim,), n_features=[512, 256],
                                       activations=["relu", "relu", "identity"],
                                       initializers=[nw.NormcInitializer(1.0), nw.NormcInitializer(1.0),
                                                     nw.NormcInitializer(0.001)],
                                       standardizer=stand, squeeze_out=False)
        load(net, params)
        return net

    def load(net, params):
        with torch.no_grad():
            for i, p in enumerate(params):
                (net._linears[i // 2].weight if i % 2 == 0 else net._linears[i // 2].bias).copy_(torch.from_numpy(p))

    def stats(st):
        return (np.asarray(st._count, dtype=np.float64).copy(), np.asarray(st._sum).copy(), np.asarray(st._sumsq).copy())

    stand = nw.Standardizer()                          # trpo_standardizer: one object for the policy and the critic
    stand.update_mean_std(prior(case))
    critic = network(1, net_params(1, c["net_seed"]), stand)
    old = net_params(ACT, c["net_seed"] + 1)
    policy = GaussianTorchPolicy(network(ACT, old, stand), ACT, STD_0)
    obs = torch.from_numpy(x)
    # ---- gail_TRPO.py:132-133: the old distribution through a deep copy, whose Standardizer is a copy too
    st_old = stats(stand)
    with torch.no_grad():
        old_policy = copy.deepcopy(policy)
        old_pol_dist = old_policy.distribution_t(obs)
    assert stats(stand)[0] == st_old[0]                # the live Standardizer did not move
    for _ in range(3):                                 # :152-154, the critic fit's updates
        stand.update_mean_std(x)
    new, log_sigma = stepped(case, old, np.full(ACT, np.log(STD_0), dtype=np.float32))
    load(policy._mu, new)
    with torch.no_grad():
        policy._log_sigma.copy_(torch.from_numpy(log_sigma))
    st0 = stats(stand)

    def regressor_call(arr):
        # ---- RESTATEMENT (a reading) of mushroom-rl's Regressor.__call__ / TorchApproximator.predict: the network's
        # forward over the whole batch, numpy in, numpy [n, 1] out
        with torch.no_grad():
            return critic(torch.from_numpy(np.asarray(arr))).detach().numpy()
        # ---- end of the restatement

    # the datasets, column by column: the environment's reward as Core collects it (Python floats), the trained-on reward
    # through arrays_as_dataset as gail_TRPO.py:162 builds it
    xc = x.reshape(T, N, OBS).transpose(1, 0, 2).reshape(T * N, OBS)
    lc = last.T.reshape(-1)
    zeros = np.zeros((T * N, 1), dtype=np.float32)
    dataset = [(xc[i], zeros[i], float(r_env.T.reshape(-1)[i]), xc[i], False, bool(lc[i])) for i in range(T * N)]
    new_dataset = arrays_as_dataset(xc, zeros, r.T.reshape(-1, 1), xc, np.zeros((T * N, 1)), lc.reshape(-1, 1))
    lengths = compute_episodes_length(dataset)
    assert len(lengths) >= 3, (case, lengths)
    frac = np.mean(lengths) % 1.0
    assert abs(frac - 0.5) > 0.01, (case, np.mean(lengths))

    g = ns.gail
    g.compute_J, g.compute_episodes_length = compute_J, compute_episodes_length
    agent = g.GAIL.__new__(g.GAIL)
    sw = Recorder()
    agent._sw, agent._iter, agent._train_D_n_th_epoch, agent._V, agent.policy = sw, ITER, 3, regressor_call, policy
    agent._logging_sw(dataset, new_dataset, x, d["v_target"][:, None], old_pol_dist)
    kl = dict((t, v) for t, v, _ in sw.rows)["kl"]
    assert 1e-3 <= kl <= 1e-2, (case, kl)
    st = stats(stand)
    return {"tags": np.array([r_[0] for r_ in sw.rows]), "values": np.array([r_[1] for r_ in sw.rows], dtype=np.float64),
            "steps": np.array([r_[2] for r_ in sw.rows], dtype=np.int64), "iter": np.int64(ITER),
            "st_old_count": st_old[0], "st_old_sum": st_old[1], "st_old_sumsq": st_old[2],
            "st0_count": st0[0], "st0_sum": st0[1], "st0_sumsq": st0[2],
            "st_count": st[0], "st_sum": st[1], "st_sumsq": st[2],
            "seed": np.int64(c["seed"]), "prior_seed": np.int64(c["prior_seed"]), "net_seed": np.int64(c["net_seed"]),
            "step_seed": np.int64(c["step_seed"]), "episodes": np.int64(len(lengths)),
            "mean_length": np.float64(np.mean(lengths)), "mu_old_head": old_pol_dist.loc[0].numpy().copy(),
            "mu_old_sum": np.float64(old_pol_dist.loc.double().sum().item())}


def main():
    out_dir = os.path.join(HERE, "iter_log")
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
    import _ref_stubs as stubs
    ns = stubs.load_reference()
    import torch
    torch.manual_seed(5)
    torch.set_num_threads(1)          # one summation order, whatever the machine
    os.makedirs(out_dir, exist_ok=True)
    for case in CASES:
        path = os.path.join(out_dir, f"{case}.npz")
        arrays = run_case(ns, case)
        np.savez_compressed(path, **arrays)
        print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB; {int(arrays['episodes'])} episodes, mean length "
              f"{float(arrays['mean_length']):.4f}; " + ", ".join(f"{t}={v:.9g}" for t, v in zip(arrays["tags"], arrays["values"])))


if __name__ == "__main__":
    main()
