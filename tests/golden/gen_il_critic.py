#!/usr/bin/env python3
"""Generate tests/golden/il_critic/il_critic_fit.npz by EXECUTING the reference's own critic
(imitation_lib/utils/networks.py: FullyConnectedNetwork, Standardizer, NormcInitializer) imported from the
reference tree under the inert stubs of _ref_stubs.py.  Run in the build container only:

    python tests/golden/gen_il_critic.py [--out DIR]

The network is the imitation critic of examples/imitation_learning/utils.py:136-149 for a 32-wide observation:
FullyConnectedNetwork(32 -> [512, 256] -> 1, relu / relu / identity, NormcInitializer(1, 1, 0.001),
standardizer=Standardizer()), fitted with torch.optim.Adam(lr=1e-4, weight_decay=0) over F.mse_loss.

mushroom-rl is absent, so its Regressor.fit loop is RESTATED here (marked below): per epoch a permutation cut
into minibatches of 256 (the last one partial, minibatch_generator), each passed through the reference
network's own forward (which updates the Standardizer, networks.py:68-81), F.mse_loss, backward, one Adam step
(TorchApproximator._fit_batch).  The permutations are drawn here and stored, so the tests replay them.

Layer 2's initial weight (256 x 512, the bulk of the parameters) is NormcInitializer's rule applied to a seeded
numpy draw, w2_init(), instead of torch's generator, so that it is rebuilt by the tests rather than stored (the
fixture stays under the size limit for a committed file).  It lives in its own directory: the fixtures of
gen_golden.py are the *.npz files of tests/golden/ itself.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "il_critic")
if "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]

N_ROWS, IN_DIM, BATCH, N_EPOCHS, LR = 1000, 32, 256, 2, 1e-4


def w2_init():
    """NormcInitializer(1.0) (networks.py:37-46) on a PCG64(7) standard-normal draw: w / ||w||_F."""
    g = np.random.default_rng(7).standard_normal((256, 512))
    return (g / np.sqrt(np.sum(np.square(g)))).astype(np.float32)


def main():
    sys.path.insert(0, HERE)
    import _ref_stubs as stubs
    ns = stubs.load_reference()
    import torch
    import torch.nn.functional as F
    nw = ns.networks
    torch.manual_seed(5)
    stand = nw.Standardizer()
    net = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(1,), n_features=[512, 256],
                                   activations=["relu", "relu", "identity"],
                                   initializers=[nw.NormcInitializer(1.0), nw.NormcInitializer(1.0),
                                                 nw.NormcInitializer(0.001)],
                                   standardizer=stand, squeeze_out=False)
    with torch.no_grad():
        net._linears[1].weight.copy_(torch.from_numpy(w2_init()))
    rng = np.random.default_rng(9)
    x = (rng.normal(0, 1, (N_ROWS, IN_DIM)) * rng.uniform(0.3, 3.0, IN_DIM) + rng.normal(0, 2, IN_DIM)).astype(np.float32)
    v_target = (rng.normal(0, 1, (N_ROWS, 1)) + 0.5 * x[:, :1]).astype(np.float32)
    perms = np.stack([rng.permutation(N_ROWS) for _ in range(N_EPOCHS)]).astype(np.int32)
    names = ["w1", "b1", "w2", "b2", "w3", "b3"]

    def params():
        return {n: t.detach().numpy().copy() for n, t in zip(names, [p for lin in net._linears for p in (lin.weight, lin.bias)])}
    init = params()
    # V(x) before the fit, through the reference forward (this updates the Standardizer, as compute_gae's calls do)
    with torch.no_grad():
        v0 = net(torch.from_numpy(x)).numpy()
    st0 = dict(st0_sum=np.asarray(stand._sum).copy(), st0_sumsq=np.asarray(stand._sumsq).copy(),
               st0_count=np.asarray(stand._count).copy())
    # ---- RESTATEMENT of mushroom-rl's Regressor.fit for a TorchApproximator (minibatch_generator + _fit_batch)
    opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=0.0)
    losses = []
    for e in range(N_EPOCHS):
        for b in range((N_ROWS + BATCH - 1) // BATCH):
            idx = perms[e, b * BATCH:min(N_ROWS, (b + 1) * BATCH)]
            out = net(torch.from_numpy(x[idx]))
            loss = F.mse_loss(out, torch.from_numpy(v_target[idx]))
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
    # ---- end of the restatement
    final = params()
    os.makedirs(OUT_DIR, exist_ok=True)
    arrays = dict(x=x, v_target=v_target, perms=perms, v0=v0, losses=np.array(losses, dtype=np.float64),
                  st_sum=np.asarray(stand._sum), st_sumsq=np.asarray(stand._sumsq), st_count=np.asarray(stand._count),
                  lr=np.float64(LR), batch=np.int64(BATCH), **st0)
    arrays.update({f"init_{n}": v for n, v in init.items() if n != "w2"})
    arrays.update({f"final_{n}": v for n, v in final.items()})
    path = os.path.join(OUT_DIR, "il_critic_fit.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
