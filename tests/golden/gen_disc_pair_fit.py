#!/usr/bin/env python3
"""Generate tests/golden/disc_pair_fit/{gail_ns,gail_sa,vail_ns,vail_sa}.npz by EXECUTING the reference's own
discriminators on PAIRED inputs (imitation_lib/utils/networks.py: DiscriminatorNetwork and VariationalNet with
use_next_states=True or use_actions=True, Standardizer; imitation_lib/utils/math.py: GailDiscriminatorLoss, VDBLoss;
imitation_lib/imitation/gail_TRPO.py: prepare_discrim_inputs, discrim_output, make_discrim_reward;
imitation_lib/imitation/vail_TRPO.py: VAIL.discrim_output) imported from the reference tree under the inert stubs of _ref_stubs.py.  Run in the build container only:

    python tests/golden/gen_disc_pair_fit.py [--out DIR]

Cases (the networks of create_gail_agent / create_vail_agent, examples/imitation_learning/utils.py:79-97,151-163, sized
as :81,153-154 size them for a 32-column state mask):
    gail_ns   GAIL (s, s')  32 + 32
    gail_sa   GAIL (s, a)   32 + 11, noisy targets, weight decay
    vail_ns   VAIL (s, s')  32 + 32
    vail_sa   VAIL (s, a)   32 + 11, noisy targets, weight decay
Each runs two epochs of _fit_discriminator (gail_TRPO.py:174-218) with three minibatches per epoch (512, 512, 256: the
last one partial), then one make_discrim_reward (:320-327) on a held-out batch.

mushroom-rl is absent, so three of its pieces are RESTATED here (marked below), as in gen_gail_disc_fit.py:
minibatch_generator's first batch for the demonstration draw (a shuffle of the rows, the first n, applied to both arrays
together), Regressor.fit's loop (a permutation of the concatenated rows cut into minibatches, each forward + loss +
backward + Adam step) and Regressor.__call__ (tensors in, numpy out).  Everything else is the reference's code, step for
step.  The shuffles are drawn here and stored, so the tests replay them.

Neither the inputs nor the initial weights are stored: inputs() rebuilds every array from a seeded numpy draw,
gail_init() / vail_init() the weights (the rules of gen_gail_disc_fit.py and gen_vail_disc_fit.py at the case's width).

The next states are NOT distributed like the states (0.6 s + 1.5 scale + noise of half the width): the Standardizer is
updated with the states and then with the next states on every forward (networks.py:224-227), so the two halves of a row
are standardised with different statistics, and only inputs whose halves differ tell that rule from a reading in which
both halves share one set of statistics.  The held-out batch is 4096 rows, about as many as the fit has fed the
Standardizer, so that the statistics before and after its next states differ visibly.  tests/test_disc_pair_cpu.py
asserts the gap.

LR is 5e-5 for GAIL (as gen_gail_disc_fit.py) and 2e-4 for VAIL: over six Adam steps every tensor then moves at least
50 times the device tolerance (2e-5 relative).  One file per case, each below 1 MiB.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_PLCY, OBS, ACT, DS, N_DEMO, N_HOLD, BATCH, N_EPOCHS = 640, 34, 13, 32, 1000, 4096, 512, 2
STATE_MASK = np.array([i for i in range(OBS) if i not in (3, 17)], dtype=np.int64)
ACT_MASK = np.array([i for i in range(ACT) if i not in (2, 9)], dtype=np.int64)
CASES = {
    "gail_ns": dict(algo="gail", pair="next_state", lr=5e-5, entcoeff=1e-3, noisy=False, wd=0.0),
    "gail_sa": dict(algo="gail", pair="action", lr=5e-5, entcoeff=0.05, noisy=True, wd=1e-3),
    "vail_ns": dict(algo="vail", pair="next_state", lr=2e-4, info_c=0.1, lr_beta=1e-2, noisy=False, wd=0.0),
    "vail_sa": dict(algo="vail", pair="action", lr=2e-4, info_c=1.0, lr_beta=0.05, noisy=True, wd=1e-3),
}
GAIL_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
VAIL_NAMES = ("enc_w0", "enc_b0", "enc_w1", "enc_b1", "mu_w", "mu_b", "lv_w", "lv_b", "dec_w", "dec_b")


def widths(case):
    """(Ds, D2) of a case."""
    return DS, (DS if CASES[case]["pair"] == "next_state" else len(ACT_MASK))


def names(case):
    return GAIL_NAMES if CASES[case]["algo"] == "gail" else VAIL_NAMES


def gail_init(in_dim, seed=31):
    """gen_gail_disc_fit.init_params at in_dim: xavier_uniform_ with the activation's gain, nn.Linear's bias rule."""
    rng = np.random.default_rng(seed)
    shapes = ((512, in_dim), (512,), (256, 512), (256,), (1, 256), (1,))
    out = []
    for i, shape in enumerate(shapes):
        if i % 2 == 0:
            gain = 5.0 / 3.0 if i < 4 else 1.0
            a = gain * np.sqrt(6.0 / (shape[0] + shape[1]))
            out.append(rng.uniform(-a, a, shape).astype(np.float32))
        else:
            out.append(rng.uniform(-1, 1, shape).astype(np.float32) / np.float32(np.sqrt(shapes[i - 1][1])))
    return out


def vail_init(in_dim, seed=11):
    """gen_vail_disc_fit.init_params at in_dim: NormcInitializer's rule on a standard-normal draw, nn.Linear's bias rule."""
    rng = np.random.default_rng(seed)
    shapes = ((256, in_dim), (256,), (128, 256), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,))
    out = []
    for i, shape in enumerate(shapes):
        if i % 2 == 0:
            g = rng.standard_normal(shape)
            out.append((g / np.sqrt(np.sum(np.square(g)))).astype(np.float32))
        else:
            out.append(rng.uniform(-1, 1, shape).astype(np.float32) / np.float32(np.sqrt(shapes[i - 1][1])))
    return out


def init_params(case):
    return (gail_init if CASES[case]["algo"] == "gail" else vail_init)(sum(widths(case)))


def inputs(seed=9):
    """Full-width float32 arrays: plcy_{obs,next,act} [640, .], demo_{states,next_states,actions} [1000, .] (the
    reference's `demonstrations` keys) and the held-out hold_{obs,next,act} [4096, .]."""
    rng = np.random.default_rng(seed)
    scale, shift = rng.uniform(0.3, 3.0, OBS), rng.normal(0, 2, OBS)
    a_scale = rng.uniform(0.2, 1.5, ACT)

    def block(n, mean, a_mean):
        s = rng.normal(mean, 1, (n, OBS)) * scale + shift
        nxt = 0.6 * s + 1.5 * scale + rng.normal(0, 0.5, (n, OBS)) * scale
        act = rng.normal(a_mean, 1, (n, ACT)) * a_scale
        return s.astype(np.float32), nxt.astype(np.float32), act.astype(np.float32)
    p, d, h = block(N_PLCY, 0.0, 0.0), block(N_DEMO, 0.3, 0.25), block(N_HOLD, 0.1, 0.1)
    return dict(plcy_obs=p[0], plcy_next=p[1], plcy_act=p[2], demo_states=d[0], demo_next_states=d[1], demo_actions=d[2],
                hold_obs=h[0], hold_next=h[1], hold_act=h[2])


def noise(case):
    """VAIL's reparameterisation noise, [N_EPOCHS * 2 N_PLCY + N_HOLD, 128], in the order the forwards consume it (the
    fit's minibatches, then the reward evaluation)."""
    seed = {"vail_ns": 23, "vail_sa": 24}[case]
    return np.random.default_rng(seed).standard_normal((N_EPOCHS * 2 * N_PLCY + N_HOLD, 128)).astype(np.float32)


def build_net(ns, case, stand):
    """(the network, its Linear layers in the order of names(case), the loss)."""
    import torch
    nw, im = ns.networks, ns.ilmath
    c = CASES[case]
    in_dim = sum(widths(case))
    flags = dict(use_actions=c["pair"] == "action", use_next_states=c["pair"] == "next_state")
    if c["algo"] == "gail":
        net = nw.DiscriminatorNetwork(input_shape=(in_dim,), output_shape=(1,), n_features=[512, 256],
                                      activations=["tanh", "tanh", "identity"], squeeze_out=False, standardizer=stand,
                                      **flags)
        lins = list(net._linears)
        loss_fn = im.GailDiscriminatorLoss(entcoeff=c["entcoeff"])
    else:
        enc = nw.FullyConnectedNetwork(input_shape=(in_dim,), output_shape=(128,), n_features=[256],
                                       activations=["relu", "relu"], standardizer=None, squeeze_out=False)
        dec = nw.FullyConnectedNetwork(input_shape=(128,), output_shape=(1,), n_features=[], activations=["identity"],
                                       standardizer=None, initializers=[nw.NormcInitializer(std=0.1)], squeeze_out=False)
        net = nw.VariationalNet(input_shape=(in_dim,), output_shape=(1,), z_size=128, encoder_net=enc, decoder_net=dec,
                                standardizer=stand, **flags)
        lins = [enc._linears[0], enc._linears[1], net.mu_out, net.logvar_out, dec._linears[0]]
        loss_fn = im.VDBLoss(info_constraint=c["info_c"], lr_beta=c["lr_beta"])
    with torch.no_grad():
        for i, p in enumerate(init_params(case)):
            t = lins[i // 2].weight if i % 2 == 0 else lins[i // 2].bias
            t.copy_(torch.from_numpy(p))
    return net, lins, loss_fn


def ns_vail(ns):
    """The reference's imitation_lib/imitation/vail_TRPO.py, imported under the stubs.  Its `from imitation_lib.imitation
    import GAIL_TRPO` is answered with the GAIL class that load_reference() imported (the package's __init__, which would
    pull every other algorithm, is not executed)."""
    import importlib
    sys.modules["imitation_lib.imitation"].GAIL_TRPO = ns.gail.GAIL
    return importlib.import_module("imitation_lib.imitation.vail_TRPO")


def run_case(ns, case, data, rng):
    import torch
    import torch.nn.functional as F
    c = CASES[case]
    gail = c["algo"] == "gail"
    stand = ns.networks.Standardizer()
    net, lins, loss_fn = build_net(ns, case, stand)
    opt = torch.optim.Adam(net.parameters(), lr=c["lr"], weight_decay=c["wd"])
    use_next = c["pair"] == "next_state"
    second_key = "next_states" if use_next else "actions"
    demonstrations = {"states": data["demo_states"], second_key: data["demo_" + second_key]}
    mask2 = STATE_MASK if use_next else ACT_MASK
    plcy_obs = data["plcy_obs"][:, STATE_MASK]                              # gail_TRPO.py:168-170
    plcy_2 = (data["plcy_next"] if use_next else data["plcy_act"])[:, mask2]
    n = plcy_obs.shape[0]
    rec = {k: [] for k in (("loss", "bce", "ent") if gail else ("loss", "bce", "kl", "beta"))}
    demo_idx, perms, targets_all = [], [], []
    eps = torch.from_numpy(noise(case)) if not gail else None
    pos = [0]

    def randn_like(t):
        out = eps[pos[0]:pos[0] + t.shape[0]].to(t.dtype)
        pos[0] += t.shape[0]
        return out
    orig = torch.randn_like
    if not gail:
        torch.randn_like = randn_like
    try:
        for epoch in range(N_EPOCHS):
            # ---- RESTATEMENT of next(minibatch_generator(n, states, second)): the first n of ONE shuffle of the rows
            idx = rng.permutation(N_DEMO)[:n]
            demo_obs, demo_2 = demonstrations["states"][idx], demonstrations[second_key][idx]
            # ---- end of the restatement
            demo_idx.append(idx)
            demo_obs = demo_obs[:, STATE_MASK]                               # :181-184 / :190-193
            demo_2 = demo_2[:, mask2]
            input_states = np.concatenate([plcy_obs, demo_obs.astype(np.float32)])
            input_second = np.concatenate([plcy_2, demo_2.astype(np.float32)])
            fit_inputs = (input_states, input_second)
            stand.update_mean_std(np.concatenate([plcy_obs, demo_obs.astype(np.float32)]))      # :206: the states only
            if c["noisy"]:
                demo_t = rng.uniform(low=0.80, high=0.99, size=(n, 1)).astype(np.float32)
                plcy_t = rng.uniform(low=0.01, high=0.10, size=(n, 1)).astype(np.float32)
            else:
                plcy_t = np.zeros(shape=(n, 1)).astype(np.float32)
                demo_t = np.ones(shape=(n, 1)).astype(np.float32)
            targets = np.concatenate([plcy_t, demo_t])
            targets_all.append(targets[:, 0])
            # ---- RESTATEMENT of mushroom-rl's Regressor.fit for a TorchApproximator (minibatch_generator + _fit_batch)
            rows = input_states.shape[0]
            perm = rng.permutation(rows)
            perms.append(perm)
            for b in range((rows + BATCH - 1) // BATCH):
                bi = perm[b * BATCH:min(rows, (b + 1) * BATCH)]
                y = net(*[torch.from_numpy(a[bi]) for a in fit_inputs])
                out = y if gail else y[0]
                t = torch.from_numpy(targets[bi]).type(out.dtype)
                with torch.no_grad():
                    if gail:
                        rec["bce"].append(torch.mean(torch.maximum(out, torch.zeros_like(out)) - out * t
                                                     + torch.log(1 + torch.exp(-torch.abs(out)))).item())
                        rec["ent"].append(torch.mean(loss_fn.logit_bernoulli_entropy(out)).item())
                    else:
                        rec["bce"].append(F.binary_cross_entropy_with_logits(torch.squeeze(out), torch.squeeze(t)).item())
                        rec["kl"].append(loss_fn.kl_divergence(y[1], y[2]).mean().item())
                loss = loss_fn(y, t)
                opt.zero_grad()
                loss.backward()
                opt.step()
                rec["loss"].append(loss.item())
                if not gail:
                    rec["beta"].append(float(loss_fn._beta))
            # ---- end of the restatement
        fit_stats = (np.asarray(stand._sum).copy(), np.asarray(stand._sumsq).copy(), np.asarray(stand._count).copy())

        # ---- one reward evaluation with the reference's own make_discrim_reward / discrim_output /
        # prepare_discrim_inputs (gail_TRPO.py:297-327, vail_TRPO.py:18-21) on a stand-in for the agent
        logits = []

        def regressor_call(*arrays):
            # ---- RESTATEMENT of mushroom-rl's Regressor.__call__ (TorchApproximator.predict): tensors in, numpy out
            with torch.no_grad():
                y = net(*[torch.from_numpy(np.asarray(a)) for a in arrays])
            y = tuple(v.detach().numpy() for v in y) if isinstance(y, tuple) else y.detach().numpy()
            # ---- end of the restatement
            logits.append(np.squeeze(y[0] if isinstance(y, tuple) else y).astype(np.float32))
            return y
        G = ns.gail.GAIL
        agent = types.SimpleNamespace(_use_next_state=use_next, _state_mask=STATE_MASK,
                                      _act_mask=np.array([], dtype=np.int64) if use_next else ACT_MASK, _D=regressor_call)
        agent.prepare_discrim_inputs = types.MethodType(G.prepare_discrim_inputs, agent)
        agent.discrim_output = types.MethodType((G if gail else ns_vail(ns).VAIL).discrim_output, agent)
        reward = G.make_discrim_reward(agent, data["hold_obs"], data["hold_act"], data["hold_next"])
    finally:
        torch.randn_like = orig
    arrays = {"demo_idx": np.stack(demo_idx).astype(np.int32), "perms": np.stack(perms).astype(np.int32),
              "fit_st_sum": fit_stats[0], "fit_st_sumsq": fit_stats[1], "fit_st_count": fit_stats[2],
              "st_sum": np.asarray(stand._sum), "st_sumsq": np.asarray(stand._sumsq), "st_count": np.asarray(stand._count),
              "state_mask": STATE_MASK, "act_mask": ACT_MASK, "lr": np.float64(c["lr"]), "batch": np.int64(BATCH),
              "noisy": np.int64(c["noisy"]), "wd": np.float64(c["wd"]),
              "reward_logits": logits[0], "reward": np.asarray(reward, dtype=np.float32)}
    for k in ("entcoeff", "info_c", "lr_beta"):
        if k in c:
            arrays[k] = np.float64(c[k])
    if c["noisy"]:
        arrays["targets"] = np.stack(targets_all).astype(np.float32)
    for k, v in rec.items():
        arrays[k] = np.array(v, dtype=np.float64)
    for i, name in enumerate(names(case)):
        t = lins[i // 2].weight if i % 2 == 0 else lins[i // 2].bias
        arrays[f"final_{name}"] = t.detach().numpy().copy()
    return arrays


def main():
    out_dir = os.path.join(HERE, "disc_pair_fit")
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
    sys.path.insert(0, HERE)
    import _ref_stubs as stubs
    ns = stubs.load_reference()
    import torch
    torch.manual_seed(5)
    torch.set_num_threads(1)          # one summation order, whatever the machine
    data = inputs()
    rng = np.random.default_rng(19)
    os.makedirs(out_dir, exist_ok=True)
    for case in CASES:
        path = os.path.join(out_dir, f"{case}.npz")
        np.savez_compressed(path, **run_case(ns, case, data, rng))
        print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
