#!/usr/bin/env python3
"""Generate tests/golden/gail_disc_fit/gail_disc_fit_{a,b}.npz by EXECUTING the reference's own GAIL discriminator
(imitation_lib/utils/networks.py: DiscriminatorNetwork, Standardizer; imitation_lib/utils/math.py:
GailDiscriminatorLoss) imported from the reference tree under the inert stubs of _ref_stubs.py.  Run in the build
container only:

    python tests/golden/gen_gail_disc_fit.py [--out DIR]

The network is the discriminator of create_gail_agent (examples/imitation_learning/utils.py:79-97) for a 32-wide masked
state: DiscriminatorNetwork(32 -> [512, 256] -> 1, tanh / tanh / identity, standardizer = the D_standardizer,
use_actions=False), fitted with torch.optim.Adam over GailDiscriminatorLoss(entcoeff).

mushroom-rl is absent, so two of its pieces are RESTATED here (marked below), as in gen_vail_disc_fit.py:
minibatch_generator's first batch for the demonstration draw (a shuffle of the demonstration rows, the first n), and
Regressor.fit's loop (a permutation of the concatenated rows cut into minibatches, the last one partial, each forward +
loss + backward + Adam step).  Everything else is the reference's _fit_discriminator (gail_TRPO.py:167-220) step for
step.  The shuffles are drawn here and stored, so the tests replay them.

Neither the inputs nor the initial weights are stored: inputs() rebuilds the observations from a seeded numpy draw;
init_params() rebuilds the weights through the network's default initialisation rule (networks.py:133-139:
xavier_uniform_ with the activation's gain, U(-a, a) with a = gain sqrt(6 / (fan_in + fan_out)), gain 5/3 for tanh and 1
for the output layer) and the biases through nn.Linear's (U(-1, 1) / sqrt(fan_in)), both from PCG64(seed).

LR is 5e-5, not HumanoidMuscle's 5e-6: over six Adam steps every tensor then moves at least 90 times the device
tolerance (2e-5 relative); at 5e-6 the smallest move is nine times it.  One file per case, each below 1 MiB.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_PLCY, OBS, IN_DIM, N_DEMO, BATCH, N_EPOCHS, LR = 640, 34, 32, 1000, 512, 2, 5e-5
STATE_MASK = np.array([i for i in range(OBS) if i not in (3, 17)], dtype=np.int64)
# case: (entcoeff, use_noisy_targets, weight_decay)
CASES = {"a": (1e-3, False, 0.0), "b": (0.05, True, 1e-3)}
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
SHAPES = ((512, IN_DIM), (512,), (256, 512), (256,), (1, 256), (1,))


def init_params(seed=31, in_dim=IN_DIM):
    """The initial parameters in torch order (W1, b1, W2, b2, W3, b3), float32."""
    rng = np.random.default_rng(seed)
    shapes = ((512, in_dim), (512,), (256, 512), (256,), (1, 256), (1,))
    out = []
    for i, shape in enumerate(shapes):
        if i % 2 == 0:
            gain = 5.0 / 3.0 if i < 4 else 1.0
            a = gain * np.sqrt(6.0 / (shape[0] + shape[1]))
            out.append(rng.uniform(-a, a, shape).astype(np.float32))
        else:
            fan_in = shapes[i - 1][1]
            out.append(rng.uniform(-1, 1, shape).astype(np.float32) / np.float32(np.sqrt(fan_in)))
    return out


def inputs(seed=9):
    """(plcy_obs [640, 34], demo_states [1000, 34]) float32: a scale and a shift per column."""
    rng = np.random.default_rng(seed)
    scale, shift = rng.uniform(0.3, 3.0, OBS), rng.normal(0, 2, OBS)
    plcy_obs = (rng.normal(0, 1, (N_PLCY, OBS)) * scale + shift).astype(np.float32)
    demo_states = (rng.normal(0.3, 1, (N_DEMO, OBS)) * scale + shift).astype(np.float32)
    return plcy_obs, demo_states


def run_case(ns, case, plcy_obs, demo_states, rng):
    import torch
    nw, im = ns.networks, ns.ilmath
    entcoeff, noisy, wd = CASES[case]
    stand = nw.Standardizer()
    net = nw.DiscriminatorNetwork(input_shape=(IN_DIM,), output_shape=(1,), n_features=[512, 256],
                                  activations=["tanh", "tanh", "identity"], squeeze_out=False, standardizer=stand,
                                  use_actions=False, use_next_states=False)
    lins = list(net._linears)
    with torch.no_grad():
        for i, p in enumerate(init_params()):
            t = lins[i // 2].weight if i % 2 == 0 else lins[i // 2].bias
            t.copy_(torch.from_numpy(p))
    loss_fn = im.GailDiscriminatorLoss(entcoeff=entcoeff)
    opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=wd)
    plcy = plcy_obs[:, STATE_MASK]
    n = plcy.shape[0]
    demo_idx, perms, targets_all, rec = [], [], [], {k: [] for k in ("loss", "bce", "ent")}
    for epoch in range(N_EPOCHS):
        # ---- RESTATEMENT of next(minibatch_generator(n, states)): the first n of a shuffle of the rows
        idx = rng.permutation(demo_states.shape[0])[:n]
        # ---- end of the restatement
        demo_idx.append(idx)
        demo_obs = demo_states[idx][:, STATE_MASK]
        input_states = np.concatenate([plcy, demo_obs.astype(np.float32)])
        stand.update_mean_std(np.concatenate([plcy, demo_obs.astype(np.float32)]))      # gail_TRPO.py:206
        if noisy:
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
            out = net(torch.from_numpy(input_states[bi]))
            t = torch.from_numpy(targets[bi]).type(out.dtype)
            with torch.no_grad():
                bce = torch.mean(torch.maximum(out, torch.zeros_like(out)) - out * t
                                 + torch.log(1 + torch.exp(-torch.abs(out))))
                rec["bce"].append(bce.item())
                rec["ent"].append(torch.mean(loss_fn.logit_bernoulli_entropy(out)).item())
            loss = loss_fn(out, t)
            opt.zero_grad()
            loss.backward()
            opt.step()
            rec["loss"].append(loss.item())
        # ---- end of the restatement
    arrays = {"demo_idx": np.stack(demo_idx).astype(np.int32), "perms": np.stack(perms).astype(np.int32),
              "st_sum": np.asarray(stand._sum), "st_sumsq": np.asarray(stand._sumsq), "st_count": np.asarray(stand._count),
              "hyper": np.array([entcoeff, float(noisy), wd], dtype=np.float64), "state_mask": STATE_MASK,
              "lr": np.float64(LR), "batch": np.int64(BATCH)}
    if noisy:
        arrays["targets"] = np.stack(targets_all).astype(np.float32)
    for k, v in rec.items():
        arrays[k] = np.array(v, dtype=np.float64)
    for i, name in enumerate(NAMES):
        t = lins[i // 2].weight if i % 2 == 0 else lins[i // 2].bias
        arrays[f"final_{name}"] = t.detach().numpy().copy()
    return arrays


def main():
    out_dir = os.path.join(HERE, "gail_disc_fit")
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
    sys.path.insert(0, HERE)
    import _ref_stubs as stubs
    ns = stubs.load_reference()
    import torch
    torch.manual_seed(5)
    torch.set_num_threads(1)          # one summation order, whatever the machine
    plcy_obs, demo_states = inputs()
    rng = np.random.default_rng(19)
    os.makedirs(out_dir, exist_ok=True)
    for case in CASES:
        path = os.path.join(out_dir, f"gail_disc_fit_{case}.npz")
        np.savez_compressed(path, **run_case(ns, case, plcy_obs, demo_states, rng))
        print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
