#!/usr/bin/env python3
"""Generate tests/golden/trpo_step/trpo_step.npz by EXECUTING the reference's own policy network
(imitation_lib/utils/networks.py: FullyConnectedNetwork, Standardizer, NormcInitializer) imported from the reference
tree under the inert stubs of _ref_stubs.py.  Run in the build container only:

    python tests/golden/gen_trpo_step.py [--out DIR]

The network is the policy mean of examples/imitation_learning/utils.py:126-134 for a 32-wide observation and 11
actions: FullyConnectedNetwork(32 -> [512, 256] -> 11, relu / relu / identity, NormcInitializer(1, 1, 0.001),
standardizer=Standardizer()), std_0 = 0.5, UnitreeH1's confs.yaml values max_kl 5e-3 and ent_coeff 1e-3, and GAIL's
defaults cg_damping 1e-1, cg_residual_tol 1e-10, n_epochs_line_search 10 and n_epochs_cg 10 (gail_TRPO.py:29-32).
With confs.yaml's n_epochs_cg 25 the residual crosses 1e-10 at iteration 11 to 13 depending on the precision and the
summation order, so the fixture keeps GAIL's default of 10, which every precision runs to the end.

mushroom-rl is absent, so GaussianTorchPolicy and TRPO's _compute_loss, _compute_kl, _fisher_vector_product(_t),
_conjugate_gradient and _line_search are RESTATED here (marked below) as this project reads mushroom-rl >= 1.10;
the step itself is gail_TRPO.py:131-149 (deepcopy of the policy, old_pol_dist, old_log_prob, loss, backward, CG,
line search), run in float32 as the reference runs it.  The float64 restatement of tests/trpo_restate.py runs the
same inputs; the spread between the two is recorded as each case's tolerance.

Two cases share the policy and the batch (n = 1000): (a) the first fit, the Standardizer fresh before VAILAgent's
own three updates (fit start, V(x), V(x')); (b) the same after 50 000 earlier rows.  Layer 2's initial weight is
rebuilt from a seed by w2_init(); the stepped W2 and W2's part of the CG solution are stored as 16 seeded
projections, so the file stays under the size limit for a committed file.
"""
import copy
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "trpo_step")
if "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]

N_ROWS, IN_DIM, ACT_DIM, STD_0 = 1000, 32, 11, 0.5
CONF = dict(max_kl=5e-3, ent_coeff=1e-3, n_epochs_cg=10, cg_damping=1e-1, cg_residual_tol=1e-10,
            n_epochs_line_search=10)


def w2_init():
    """NormcInitializer(1.0) (networks.py:37-46) on a PCG64(11) standard-normal draw: w / ||w||_F."""
    g = np.random.default_rng(11).standard_normal((256, 512))
    return (g / np.sqrt(np.sum(np.square(g)))).astype(np.float32)


def w2_proj():
    """16 seeded directions W2's stepped values and CG part are projected on (rebuilt by the tests, not stored)."""
    return np.random.default_rng(12).standard_normal((16, 256 * 512)).astype(np.float32)


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import _ref_stubs as stubs
    ns = stubs.load_reference()
    import torch
    import trpo_restate as tr
    nw = ns.networks

    # ---- RESTATEMENT of mushroom-rl's GaussianTorchPolicy (>= 1.10, this project's reading)
    class GaussianTorchPolicy(torch.nn.Module):
        def __init__(self, network, action_dim, std_0):
            super().__init__()
            self._mu = network
            self._action_dim = action_dim
            self._log_sigma = torch.nn.Parameter(torch.ones(action_dim) * np.log(std_0))

        def distribution_t(self, state):
            mu = self._mu(state)
            return torch.distributions.MultivariateNormal(loc=mu, scale_tril=torch.diag(torch.exp(self._log_sigma)))

        def log_prob_t(self, state, action):
            return self.distribution_t(state).log_prob(action)[:, None]

        def entropy_t(self, state=None):
            return self._action_dim / 2 * np.log(2 * np.pi * np.e) + torch.sum(self._log_sigma)

        def parameters(self):
            return itertools.chain(self._mu.parameters(), [self._log_sigma])

        def get_weights(self):
            return np.concatenate([p.data.detach().cpu().numpy().flatten() for p in self.parameters()])

        def set_weights(self, w):
            i = 0
            for p in self.parameters():
                k = p.numel()
                p.data = torch.from_numpy(w[i:i + k]).reshape(p.shape)
                i += k

    # ---- RESTATEMENT of mushroom-rl's TRPO methods (>= 1.10, this project's reading; numpy float32 CG)
    def compute_loss(policy, obs, act, adv, old_log_prob):
        ratio = torch.exp(policy.log_prob_t(obs, act) - old_log_prob)
        J = torch.mean(ratio * adv)
        return J + CONF["ent_coeff"] * policy.entropy_t(obs)

    def compute_kl(policy, obs, old_pol_dist):
        new_pol_dist = policy.distribution_t(obs)
        return torch.mean(torch.distributions.kl.kl_divergence(old_pol_dist, new_pol_dist))

    def fvp(policy, p, obs, old_pol_dist):
        p_t = torch.from_numpy(p)
        kl = compute_kl(policy, obs, old_pol_dist)
        grads = torch.autograd.grad(kl, list(policy.parameters()), create_graph=True)
        flat_grad_kl = torch.cat([g.view(-1) for g in grads])
        kl_v = torch.sum(flat_grad_kl * p_t)
        grads_v = torch.autograd.grad(kl_v, list(policy.parameters()), create_graph=False)
        flat_grad_grad_kl = torch.cat([g.contiguous().view(-1) for g in grads_v]).data
        return (flat_grad_grad_kl + p_t * CONF["cg_damping"]).detach().cpu().numpy()

    def conjugate_gradient(policy, b, obs, old_pol_dist):
        p = b.detach().cpu().numpy()
        r = b.detach().cpu().numpy()
        x = np.zeros_like(p)
        r2 = r.dot(r)
        k_run = 0
        for _ in range(CONF["n_epochs_cg"]):
            z = fvp(policy, p, obs, old_pol_dist)
            v = r2 / p.dot(z)
            x += v * p
            r -= v * z
            r2_new = r.dot(r)
            mu = r2_new / r2
            p = r + mu * p
            r2 = r2_new
            k_run += 1
            if r2 < CONF["cg_residual_tol"]:
                break
        return x, k_run

    def line_search(policy, obs, act, adv, old_log_prob, old_pol_dist, prev_loss, stepdir):
        direction = fvp(policy, stepdir, obs, old_pol_dist)
        shs = .5 * stepdir.dot(direction)
        lm = np.sqrt(shs / CONF["max_kl"])
        full_step = stepdir / lm
        stepsize = 1.
        theta_old = policy.get_weights()
        violation = True
        j_acc, j_run, kl, new_loss = -1, 0, None, None
        for j in range(CONF["n_epochs_line_search"]):
            theta_new = theta_old + full_step * stepsize
            policy.set_weights(theta_new)
            new_loss = compute_loss(policy, obs, act, adv, old_log_prob)
            kl = compute_kl(policy, obs, old_pol_dist)
            improve = new_loss - prev_loss
            j_run = j + 1
            if kl <= CONF["max_kl"] * 1.5 or improve >= 0:
                violation = False
                j_acc = j
                break
            stepsize *= .5
        if violation:
            policy.set_weights(theta_old)
        return dict(shs=float(shs), j=j_acc, j_run=j_run, kl=float(kl), J=float(new_loss))
    # ---- end of the restatement

    torch.manual_seed(13)
    stand = nw.Standardizer()
    net = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(ACT_DIM,), n_features=[512, 256],
                                   activations=["relu", "relu", "identity"],
                                   initializers=[nw.NormcInitializer(1.0), nw.NormcInitializer(1.0),
                                                 nw.NormcInitializer(0.001)],
                                   standardizer=stand)
    with torch.no_grad():
        net._linears[1].weight.copy_(torch.from_numpy(w2_init()))
    policy0 = GaussianTorchPolicy(net, ACT_DIM, STD_0)
    rng = np.random.default_rng(17)
    scale, shift = rng.uniform(0.3, 3.0, IN_DIM), rng.normal(0, 2, IN_DIM)
    x = (rng.normal(0, 1, (N_ROWS, IN_DIM)) * scale + shift).astype(np.float32)
    xn = (rng.normal(0, 1, (N_ROWS, IN_DIM)) * scale + shift).astype(np.float32)
    act = rng.normal(0, STD_0, (N_ROWS, ACT_DIM)).astype(np.float32)
    # advantages that favour a direction of the action space (a gradient well above the CG tolerance)
    adv = rng.normal(0, 1, (N_ROWS, 1)) + 2.0 * act[:, :1] / STD_0
    adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).astype(np.float32)
    prior = (rng.normal(0, 1, (50 * N_ROWS, IN_DIM)) * scale * 1.3 + shift * 0.8).astype(np.float32)
    names = ["w1", "b1", "w2", "b2", "w3", "b3"]
    init = {n: t.detach().numpy().copy() for n, t in zip(names, [p for lin in net._linears for p in (lin.weight, lin.bias)])}
    proj = w2_proj()

    def colstats(st):
        """Standardizer (_count, _sum, _sumsq) as raw (count, sum, sumsq) rows: the 1e-2 starting values removed."""
        cnt = np.round(np.asarray(st._count, dtype=np.float64) - 1e-2)
        return np.stack([np.broadcast_to(cnt, (IN_DIM,)), np.asarray(st._sum, dtype=np.float64),
                         np.asarray(st._sumsq, dtype=np.float64) - 1e-2])

    def split_store(v):
        W1, b1, W2, b2, W3, b3, ls = tr.split(torch.from_numpy(np.asarray(v, dtype=np.float64)), IN_DIM, ACT_DIM)
        flat = torch.cat([W1.reshape(-1), b1, b2, W3.reshape(-1), b3, ls]).numpy()
        return flat, (proj.astype(np.float64) @ W2.reshape(-1).numpy())

    arrays = dict(x=x, act=act, adv=adv, std_0=np.float64(STD_0),
                  **{k: np.float64(v) for k, v in CONF.items()},
                  init_log_sigma=np.full(ACT_DIM, np.log(STD_0), dtype=np.float32))
    arrays.update({f"init_{n}": v for n, v in init.items() if n != "w2"})
    for name, n_prior in (("a", 0), ("b", 50)):
        policy = copy.deepcopy(policy0)
        st = policy._mu._stand
        for b in range(n_prior):
            st.update_mean_std(prior[b * N_ROWS:(b + 1) * N_ROWS])
        for b in (x, x, xn):                          # VAILAgent.fit's own updates: fit start, V(x), V(x')
            st.update_mean_std(b)
        S = colstats(st)
        obs, a_t, adv_t = torch.from_numpy(x), torch.from_numpy(act), torch.from_numpy(adv)
        # ---- gail_TRPO.py:131-149 on the restated policy / TRPO
        old_policy = copy.deepcopy(policy)
        old_pol_dist = old_policy.distribution_t(obs)
        old_log_prob = old_policy.log_prob_t(obs, a_t).detach()
        for p in policy.parameters():
            p.grad = None
        loss = compute_loss(policy, obs, a_t, adv_t, old_log_prob)
        prev_loss = loss.item()
        loss.backward()
        g = torch.cat([p.grad.view(-1) for p in policy.parameters()])
        stepdir, k_run = conjugate_gradient(policy, g, obs, old_pol_dist)
        ls_out = line_search(policy, obs, a_t, adv_t, old_log_prob, old_pol_dist, prev_loss, stepdir)
        # ---- end
        theta = policy.get_weights()
        S_final = colstats(st)
        # the float64 restatement of the same step: the spread sets the case's tolerance
        theta0 = torch.from_numpy(policy0.get_weights())
        r64 = tr.trpo_step(theta0, torch.from_numpy(S), obs, a_t, adv_t.reshape(-1), **CONF)
        assert r64["j"] == ls_out["j"] and r64["k_run"] == k_run, (name, r64["j"], ls_out["j"], r64["k_run"], k_run)
        spread = [abs(r64[k] - v) / max(1.0, abs(v)) for k, v in (("prev_loss", prev_loss), ("shs", ls_out["shs"]),
                                                                   ("kl", ls_out["kl"]), ("J", ls_out["J"]))]
        for mine, ref in ((r64["stepdir"], stepdir), (r64["theta"], theta)):
            for u, v in zip(split_store(mine.numpy()), split_store(ref)):
                spread.append(float(np.linalg.norm(u - v) / np.linalg.norm(v)))
        tol = max(4.0 * max(spread), 1e-6)
        sd_flat, sd_proj = split_store(stepdir)
        th_flat, th_proj = split_store(theta)
        arrays.update({f"{name}_S": S, f"{name}_S_final": S_final, f"{name}_prev_loss": np.float64(prev_loss),
                       f"{name}_k_run": np.int64(k_run), f"{name}_shs": np.float64(ls_out["shs"]),
                       f"{name}_j": np.int64(ls_out["j"]), f"{name}_j_run": np.int64(ls_out["j_run"]),
                       f"{name}_kl": np.float64(ls_out["kl"]), f"{name}_J": np.float64(ls_out["J"]),
                       f"{name}_stepdir_flat": sd_flat.astype(np.float32), f"{name}_stepdir_w2proj": sd_proj,
                       f"{name}_theta_flat": th_flat.astype(np.float32), f"{name}_theta_w2proj": th_proj,
                       f"{name}_spread": np.float64(max(spread)), f"{name}_tol": np.float64(tol)})
        print(f"case {name}: k_run {k_run}, j {ls_out['j']}, kl {ls_out['kl']:.3e}, prev_loss {prev_loss:.6f}, "
              f"J {ls_out['J']:.6f}, f32/f64 spread {max(spread):.2e}")
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, "trpo_step.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
