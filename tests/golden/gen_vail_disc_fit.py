#!/usr/bin/env python3
"""Generate tests/golden/vail_disc_fit/vail_disc_fit.npz by EXECUTING the reference's own VAIL discriminator
(imitation_lib/utils/networks.py: VariationalNet, FullyConnectedNetwork, Standardizer; imitation_lib/utils/math.py:
VDBLoss) imported from the reference tree under the inert stubs of _ref_stubs.py.  Run in the build container only:

    python tests/golden/gen_vail_disc_fit.py [--out DIR]

The network is the discriminator of examples/imitation_learning/utils.py:151-163 for a 32-wide masked state:
VariationalNet(encoder 32 -> [256] -> 128 relu / relu, mu / logvar 128 -> 128, decoder 128 -> 1, standardizer =
the D_standardizer), fitted with torch.optim.Adam(lr=5e-5) over VDBLoss.

mushroom-rl is absent, so two of its pieces are RESTATED here (marked below): minibatch_generator's first batch for the
demonstration draw (a shuffle of the demonstration rows, the first n), and Regressor.fit's loop (a permutation of the
concatenated rows cut into minibatches, the last one partial, each forward + loss + backward + Adam step).  Everything
else is the reference's _fit_discriminator (gail_TRPO.py:167-220) step for step.  The shuffles are drawn here and
stored, so the tests replay them.

Neither the initial weights nor the reparameterisation noise are stored: init_params() rebuilds the weights from a
seeded numpy draw through NormcInitializer's rule (networks.py:37-46: w / ||w||_F) and the biases from a seeded uniform
draw; noise() is the seeded PCG64 stream that torch.randn_like is patched to hand to the reference's reparameterize
(networks.py:21-24), minibatch after minibatch.  The fixture lives in its own directory: the fixtures of gen_golden.py
are the *.npz files of tests/golden/ itself.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_PLCY, OBS, IN_DIM, N_DEMO, BATCH, N_EPOCHS, LR = 640, 34, 32, 1000, 512, 2, 5e-5
STATE_MASK = np.array([i for i in range(OBS) if i not in (3, 17)], dtype=np.int64)
# case: (info_constraint, lr_beta, use_noisy_targets, weight_decay)
CASES = {"a": (0.1, 1e-2, False, 0.0), "b": (1.0, 0.05, True, 1e-3)}
NAMES = ("enc_w0", "enc_b0", "enc_w1", "enc_b1", "mu_w", "mu_b", "lv_w", "lv_b", "dec_w", "dec_b")
SHAPES = ((256, IN_DIM), (256,), (128, 256), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,))


def init_params(seed=11):
    """The initial parameters in oly_disc_pack's order: every weight NormcInitializer's rule on a standard-normal
    draw, every bias U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (nn.Linear's rule), both from PCG64(seed)."""
    rng = np.random.default_rng(seed)
    out = []
    for name, shape in zip(NAMES, SHAPES):
        if "_w" in name:
            g = rng.standard_normal(shape)
            out.append((g / np.sqrt(np.sum(np.square(g)))).astype(np.float32))
        else:
            fan_in = IN_DIM if name == "enc_b0" else 256 if name == "enc_b1" else 128
            out.append(rng.uniform(-1, 1, shape).astype(np.float32) / np.float32(np.sqrt(fan_in)))
    return out


def noise(case):
    """The reparameterisation noise of a case, [N_EPOCHS, 2 N_PLCY, 128], in the order the forwards consume it."""
    seed = {"a": 21, "b": 22}[case]
    return np.random.default_rng(seed).standard_normal((N_EPOCHS, 2 * N_PLCY, 128)).astype(np.float32)


def run_case(ns, case, plcy_obs, demo_states, rng):
    import torch
    import torch.nn.functional as F
    nw, im = ns.networks, ns.ilmath
    info_c, lr_beta, noisy, wd = CASES[case]
    stand = nw.Standardizer()
    enc = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(128,), n_features=[256],
                                   activations=["relu", "relu"], standardizer=None, squeeze_out=False)
    dec = nw.FullyConnectedNetwork(input_shape=(128,), output_shape=(1,), n_features=[], activations=["identity"],
                                   standardizer=None, initializers=[nw.NormcInitializer(std=0.1)], squeeze_out=False)
    net = nw.VariationalNet(input_shape=(IN_DIM,), output_shape=(1,), z_size=128, encoder_net=enc, decoder_net=dec,
                            standardizer=stand, use_actions=False, use_next_states=False)
    lins = [enc._linears[0], enc._linears[1], net.mu_out, net.logvar_out, dec._linears[0]]
    with torch.no_grad():
        for i, p in enumerate(init_params()):
            t = lins[i // 2].weight if i % 2 == 0 else lins[i // 2].bias
            t.copy_(torch.from_numpy(p))
    loss_fn = im.VDBLoss(info_constraint=info_c, lr_beta=lr_beta)
    opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=wd)
    eps = torch.from_numpy(noise(case).reshape(-1, 128))
    pos = [0]

    def randn_like(t):
        out = eps[pos[0]:pos[0] + t.shape[0]].to(t.dtype)
        pos[0] += t.shape[0]
        return out

    plcy = plcy_obs[:, STATE_MASK]
    n = plcy.shape[0]
    demo_idx, perms, targets_all, rec = [], [], [], {k: [] for k in ("loss", "bce", "kl", "beta")}
    orig = torch.randn_like
    torch.randn_like = randn_like
    try:
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
                out, mu, logvar = net(torch.from_numpy(input_states[bi]))
                t = torch.from_numpy(targets[bi]).type(out.dtype)
                with torch.no_grad():
                    rec["bce"].append(F.binary_cross_entropy_with_logits(torch.squeeze(out), torch.squeeze(t)).item())
                    rec["kl"].append(loss_fn.kl_divergence(mu, logvar).mean().item())
                loss = loss_fn((out, mu, logvar), t)
                opt.zero_grad()
                loss.backward()
                opt.step()
                rec["loss"].append(loss.item())
                rec["beta"].append(float(loss_fn._beta))
            # ---- end of the restatement
    finally:
        torch.randn_like = orig
    arrays = {f"{case}_demo_idx": np.stack(demo_idx).astype(np.int32), f"{case}_perms": np.stack(perms).astype(np.int32),
              f"{case}_st_sum": np.asarray(stand._sum), f"{case}_st_sumsq": np.asarray(stand._sumsq),
              f"{case}_st_count": np.asarray(stand._count),
              f"{case}_hyper": np.array([info_c, lr_beta, float(noisy), wd], dtype=np.float64)}
    if noisy:
        arrays[f"{case}_targets"] = np.stack(targets_all).astype(np.float32)
    for k, v in rec.items():
        arrays[f"{case}_{k}"] = np.array(v, dtype=np.float64)
    for i, name in enumerate(NAMES):
        t = lins[i // 2].weight if i % 2 == 0 else lins[i // 2].bias
        arrays[f"{case}_final_{name}"] = t.detach().numpy().copy()
    return arrays


def main():
    out_dir = os.path.join(HERE, "vail_disc_fit")
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
    sys.path.insert(0, HERE)
    import _ref_stubs as stubs
    ns = stubs.load_reference()
    import torch
    torch.manual_seed(5)
    rng = np.random.default_rng(9)
    scale, shift = rng.uniform(0.3, 3.0, OBS), rng.normal(0, 2, OBS)
    plcy_obs = (rng.normal(0, 1, (N_PLCY, OBS)) * scale + shift).astype(np.float32)
    demo_states = (rng.normal(0.3, 1, (N_DEMO, OBS)) * scale + shift).astype(np.float32)
    arrays = dict(plcy_obs=plcy_obs, demo_states=demo_states, state_mask=STATE_MASK, lr=np.float64(LR),
                  batch=np.int64(BATCH))
    for case in CASES:
        arrays.update(run_case(ns, case, plcy_obs, demo_states, rng))
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "vail_disc_fit.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
