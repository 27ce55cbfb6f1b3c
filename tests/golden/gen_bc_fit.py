#!/usr/bin/env python3
"""Generate tests/golden/bc_fit/bc_fit.npz by EXECUTING the reference's own network classes
(imitation_lib/utils/networks.py: FullyConnectedNetwork, Standardizer) imported from the reference tree under the inert
stubs of _ref_stubs.py, inside behavioural cloning's loop.  Run in the build container only:

    python tests/golden/gen_bc_fit.py [--out DIR]

The network is the actor of BehavioralCloning (imitation_lib/imitation/offline/behavioral_cloning.py:14-40) for a
32-wide observation and 11 actions: FullyConnectedNetwork(32 -> [512, 256] -> 22, relu / relu / identity,
standardizer=Standardizer()) with the class's default initialisation, fitted with torch.optim.Adam(lr=1e-3) over
torch.nn.GaussianNLLLoss(), batch 32, 200 demonstration rows, 6 steps.

mushroom-rl is absent, so the lines of fit_offline (:46-80) and of IQ_Learn_Policy (imitation_lib/imitation/iq_sac.py)
that go through it are RESTATED here and marked below: minibatch_generator's first batch (a permutation's first 32
entries, drawn here and stored, so the tests replay it), to_float_tensor, get_central_delta (iq_sac.py:43-44) and
get_mu_log_sigma's call of the Regressor (:132-151; the split and the clamp are its own lines, copied in meaning).  The
forward is the reference network's own (it updates the Standardizer, networks.py:68-81), the loss, backward and Adam are
torch's.

Layer 2's initial weight (256 x 512, the bulk of the parameters) is a seeded numpy draw, w2_init(), instead of torch's
generator, so that the tests rebuild it rather than the fixture storing it; the stepped layer-2 weights are not stored
either (the fixture stays under the size limit for a committed file).  The archive is written with fixed member dates:
running the generator again reproduces the file byte for byte.  The fixture holds data only.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "bc_fit")
if __name__ == "__main__" and "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]

N_ROWS, IN_DIM, ACT_DIM, BATCH, N_STEPS, LR = 200, 32, 11, 32, 6, 1e-3
SNAPSHOTS = (1, 3, 6)
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def w2_init():
    """Layer 2's initial weight: uniform in -+sqrt(2) sqrt(6 / (512 + 256)) (xavier_uniform_ with relu's gain, the rule
    of FullyConnectedNetwork's default initialisation) on a PCG64(7) draw."""
    bound = np.sqrt(2.0) * np.sqrt(6.0 / (512 + 256))
    return np.random.default_rng(7).uniform(-bound, bound, (256, 512)).astype(np.float32)


def inputs():
    """(states [200,32] f32 with a scale and a shift per column, actions [200,11] f32 inside the bounds, min_a, max_a f64
    of unequal widths), rebuilt from the seed."""
    rng = np.random.default_rng(19)
    scale, shift = rng.uniform(0.3, 3.0, IN_DIM), rng.standard_normal(IN_DIM) * 2.0
    states = (rng.standard_normal((N_ROWS, IN_DIM)) * scale + shift).astype(np.float32)
    min_a, max_a = -rng.uniform(0.5, 2.0, ACT_DIM), rng.uniform(0.5, 3.0, ACT_DIM)
    u = np.tanh(0.8 * rng.standard_normal((N_ROWS, ACT_DIM)) + 0.3 * (states[:, :1] - shift[0]) / scale[0])
    actions = (0.5 * (max_a + min_a) + 0.5 * (max_a - min_a) * u).astype(np.float32)
    return states, actions, min_a, max_a


def initial_params(g):
    """The six initial tensors from the fixture `g` and w2_init()."""
    return [w2_init() if n == "w2" else g[f"init_{n}"] for n in NAMES]


def write_npz(path, arrays):
    """An .npz (a zip of .npy members, deflated) whose bytes depend on the arrays alone: members in sorted order with
    a fixed date."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    sys.path.insert(0, HERE)
    import _ref_stubs as stubs
    ns = stubs.load_reference()
    import torch
    from torch.nn import GaussianNLLLoss
    nw = ns.networks
    torch.manual_seed(5)
    stand = nw.Standardizer()
    net = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(2 * ACT_DIM,), n_features=[512, 256],
                                   activations=["relu", "relu", "identity"], standardizer=stand, squeeze_out=False)
    with torch.no_grad():
        net._linears[1].weight.copy_(torch.from_numpy(w2_init()))
    states, actions, min_a, max_a = inputs()
    rng = np.random.default_rng(23)
    idx = np.stack([rng.permutation(N_ROWS)[:BATCH] for _ in range(N_STEPS)]).astype(np.int32)

    def params():
        return {n: t.detach().numpy().copy() for n, t in zip(NAMES, [p for lin in net._linears for p in (lin.weight, lin.bias)])}
    arrays = {f"init_{n}": v for n, v in params().items() if n != "w2"}
    # ---- RESTATEMENT (mushroom-rl pieces): to_float_tensor(.5 * (max_a -+ min_a)), iq_sac.py:43-44
    delta_a = torch.as_tensor(0.5 * (max_a - min_a), dtype=torch.float32)
    central_a = torch.as_tensor(0.5 * (max_a + min_a), dtype=torch.float32)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    actor_loss = GaussianNLLLoss()
    scalars = []
    for i in range(N_STEPS):
        # RESTATEMENT: next(minibatch_generator(batch_size, states, actions, ...)), to_float_tensor
        s = torch.as_tensor(states[idx[i]], dtype=torch.float32)
        target_actions = torch.as_tensor(actions[idx[i]], dtype=torch.float32)
        # behavioral_cloning.py:63-66
        target_actions = torch.clip((target_actions - central_a) / delta_a, -1.0 + 1e-7, 1.0 - 1e-7)
        target_actions = torch.arctanh(target_actions)
        # RESTATEMENT of get_mu_log_sigma (iq_sac.py:132-151): the Regressor's predict is the network's forward
        mu_log_sigma = net(s)
        mu, log_sigma = mu_log_sigma[:, 0:ACT_DIM], mu_log_sigma[:, ACT_DIM:2 * ACT_DIM]
        log_sigma = torch.clamp(log_sigma, LOG_STD_MIN, LOG_STD_MAX)
        # behavioral_cloning.py:71-75
        loss = actor_loss(input=mu, target=target_actions, var=torch.square(log_sigma.exp()))
        opt.zero_grad()
        loss.backward()
        opt.step()
        # logging(), :82-94, without the sampled entropy
        gauss_ent = ACT_DIM * (0.5 + 0.5 * np.log(2 * np.pi)) + torch.sum(log_sigma, axis=-1)     # entropy_from_logsigma
        mse = torch.nn.functional.mse_loss(mu, target_actions)
        scalars.append([np.mean(loss.detach().numpy()), np.mean(gauss_ent.detach().numpy()), np.mean(mse.detach().numpy())])
        if i + 1 in SNAPSHOTS:
            arrays.update({f"{n}_step{i + 1}": v for n, v in params().items() if n != "w2"})
    # ---- end of the restatement
    arrays.update(idx=idx, scalars=np.asarray(scalars, dtype=np.float64), st_sum=np.asarray(stand._sum, np.float64),
                  st_sumsq=np.asarray(stand._sumsq, np.float64), st_count=np.asarray(stand._count, np.float64),
                  lr=np.float64(LR), batch=np.int64(BATCH))
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, "bc_fit.npz")
    write_npz(path, arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
