#!/usr/bin/env python3
"""Generate tests/golden/disc_log/{gail_s,gail_ns,vail_s,vail_sa}.npz by EXECUTING the reference's own
_discriminator_logging (imitation_lib/imitation/gail_TRPO.py:222-249; VAIL's extension, vail_TRPO.py:23-32) with its
divide_data_to_demo_and_plcy, discrim_output and prepare_discrim_inputs, on the reference's DiscriminatorNetwork /
VariationalNet, Standardizer (imitation_lib/utils/networks.py) and GailDiscriminatorLoss / VDBLoss
(imitation_lib/utils/math.py), imported from the reference tree under the inert stubs of _ref_stubs.py.  Run in the
build container only:

    python tests/golden/gen_disc_log.py [--out DIR]

The methods are called on an instance of the reference's GAIL / VAIL class made without its constructor (which needs
mushroom-rl), carrying the attributes the methods read: _sw (a recording stand-in for the SummaryWriter), _loss, _D,
_iter, _state_mask, _act_mask, _use_next_state.  mushroom-rl is absent, so two of its pieces are RESTATED (marked below):
Regressor.__call__ as `_D` (a READING of mushroom's TorchApproximator.predict: the network's forward over the whole
batch, tensors in, numpy out) and to_float_tensor (torch.as_tensor(x).float()).  Everything else is the reference's code.

Cases (networks as gen_disc_pair_fit.py sizes them; 640 policy rows, 640 drawn demonstrations, 34 columns masked to 32):
    gail_s    GAIL, states only
    gail_ns   GAIL (s, s')  32 + 32: two Standardizer updates per forward
    vail_s    VAIL, states only
    vail_sa   VAIL (s, a)   32 + 11, noisy targets
The Standardizer starts from PRIOR_ROWS rows of a differently shifted distribution, so the six (seven) statistics the
forwards standardise with differ visibly.  VAIL's weights are not the initialiser's (whose logits all share one sign)
but a seeded draw at a trained network's scale (vail_params), so that accuracies lie strictly between 0 and 1 and the
bottleneck term is of the loss's order; lr_beta is large enough that the dual update the logging's copy of the loss takes
between its three evaluations shows.

Neither inputs, weights nor noise are stored: case_args() rebuilds them from the seeds the fixture names.  The accuracy
scalars are step functions of the logits, so the weight seed is the first for which no float64 logit of any forward
(tests/disc_log_restate.py) lies within 1e-4 of zero.  One file per case, each a few KiB.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
import gen_disc_pair_fit as gp  # noqa: E402  (inputs, the masks, gail_init)

N_PLCY, DS, PRIOR_ROWS, ITER = gp.N_PLCY, gp.DS, 3000, 7
CASES = {
    "gail_s": dict(algo="gail", pair=None, entcoeff=1e-3, noisy=False, prior_seed=41, draw_seed=51),
    "gail_ns": dict(algo="gail", pair="next_state", entcoeff=0.05, noisy=False, prior_seed=42, draw_seed=52),
    "vail_s": dict(algo="vail", pair=None, entcoeff=1e-3, info_c=0.5, lr_beta=1e-2, beta=0.25, noisy=False, prior_seed=43,
                   draw_seed=53, noise_seed=63),
    "vail_sa": dict(algo="vail", pair="action", entcoeff=1e-3, info_c=1.0, lr_beta=5e-3, beta=0.125, noisy=True,
                    prior_seed=44, draw_seed=54, noise_seed=64),
}


def widths(case):
    pair = CASES[case]["pair"]
    return DS, (0 if pair is None else DS if pair == "next_state" else len(gp.ACT_MASK))


def vail_params(in_dim, seed):
    """A seeded VariationalNet at a trained network's scale (torch order: enc_w0, enc_b0, enc_w1, enc_b1, mu_w, mu_b,
    lv_w, lv_b, dec_w, dec_b)."""
    rng = np.random.default_rng(seed)
    shapes = ((256, in_dim), (256,), (128, 256), (128,), (128, 128), (128,), (128, 128), (128,), (1, 128), (1,))
    gains = (1.4, 1.4, 0.3, 0.3, 2.0)
    out = []
    for i, shape in enumerate(shapes):
        if i % 2 == 0:
            out.append((rng.standard_normal(shape) * gains[i // 2] / np.sqrt(shape[1])).astype(np.float32))
        else:
            out.append((rng.uniform(-1, 1, shape) * 0.1).astype(np.float32))
    return out


def params(case, seed):
    in_dim = sum(widths(case))
    return gp.gail_init(in_dim, seed) if CASES[case]["algo"] == "gail" else vail_params(in_dim, seed)


def prior(case):
    """The rows the Standardizer has seen before the call: another shift and scale than the batch's."""
    rng = np.random.default_rng(CASES[case]["prior_seed"])
    return (rng.normal(1.0, 1.0, (PRIOR_ROWS, DS)) * rng.uniform(0.5, 4.0, DS) + rng.normal(0, 3, DS)).astype(np.float32)


def batch(case):
    """(x [1280,32], x2 or None, targets [1280] or None, demo_idx): the masked concatenated rows as _fit_discriminator
    builds them (gail_TRPO.py:168-216)."""
    c = CASES[case]
    data = gp.inputs()
    rng = np.random.default_rng(c["draw_seed"])
    idx = rng.permutation(gp.N_DEMO)[:N_PLCY]
    x = np.concatenate([data["plcy_obs"][:, gp.STATE_MASK], data["demo_states"][idx][:, gp.STATE_MASK].astype(np.float32)])
    x2 = None
    if c["pair"] == "next_state":
        x2 = np.concatenate([data["plcy_next"][:, gp.STATE_MASK], data["demo_next_states"][idx][:, gp.STATE_MASK]])
    elif c["pair"] == "action":
        x2 = np.concatenate([data["plcy_act"][:, gp.ACT_MASK], data["demo_actions"][idx][:, gp.ACT_MASK]])
    targets = None
    if c["noisy"]:
        demo_t = rng.uniform(low=0.80, high=0.99, size=(N_PLCY, 1)).astype(np.float32)
        plcy_t = rng.uniform(low=0.01, high=0.10, size=(N_PLCY, 1)).astype(np.float32)
        targets = np.concatenate([plcy_t, demo_t])[:, 0]
    return x, x2, targets, idx


def noise(case):
    """VAIL's reparameterisation noise of forwards 1 .. 6: blocks of [rows_k, 128] (all rows, demonstration half, policy
    half, twice)."""
    c = CASES[case]
    if c["algo"] != "vail":
        return None
    rng = np.random.default_rng(c["noise_seed"])
    n = 2 * N_PLCY
    return [rng.standard_normal((r, 128)).astype(np.float32) for r in (n, n - N_PLCY, N_PLCY) * 2]


def case_args(case, g):
    """restate_log's arguments for a fixture: everything rebuilt from the seeds it names, the start statistics from it."""
    c = CASES[case]
    x, x2, targets, idx = batch(case)
    assert np.array_equal(idx, g["demo_idx"])
    cs = np.stack([np.full(DS, float(g["st0_count"][0]) - 1e-2), g["st0_sum"].astype(np.float64),
                   g["st0_sumsq"].astype(np.float64) - 1e-2])
    return dict(algo=c["algo"], params=params(case, int(g["param_seed"])), colstats=cs, x=x, n_plcy=N_PLCY, x2=x2,
                pair=c["pair"], targets=targets, entcoeff=c["entcoeff"], beta=c.get("beta", 0.0), info_c=c.get("info_c", 0.0),
                lr_beta=c.get("lr_beta", 0.0), noise=noise(case))


def pick_seed(case):
    """The first weight seed for which no float64 logit of any forward is within the band of zero."""
    import disc_log_restate as rs
    c = CASES[case]
    x, x2, targets, _ = batch(case)
    st = rs.Stats(1e-2, np.zeros(DS), np.full(DS, 1e-2))
    st.add(prior(case))
    for seed in range(100, 200):
        out = rs.restate_log(c["algo"], params(case, seed), st.colstats(), x, N_PLCY, x2=x2, pair=c["pair"], targets=targets,
                             entcoeff=c["entcoeff"], beta=c.get("beta", 0.0), info_c=c.get("info_c", 0.0),
                             lr_beta=c.get("lr_beta", 0.0), noise=noise(case))
        if min(float(np.abs(d).min()) for d in out["logits"]) >= 2 * rs.BAND:
            return seed
    raise RuntimeError(f"{case}: no seed keeps every logit out of the band")


class Recorder:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


def run_case(ns, case):
    import torch
    c = CASES[case]
    gail = c["algo"] == "gail"
    seed = pick_seed(case)
    x, x2, targets, idx = batch(case)
    stand = ns.networks.Standardizer()
    stand.update_mean_std(prior(case))
    st0 = (np.asarray(stand._count, dtype=np.float64).copy(), np.asarray(stand._sum).copy(), np.asarray(stand._sumsq).copy())

    nw, im = ns.networks, ns.ilmath
    in_dim = sum(widths(case))
    flags = dict(use_actions=c["pair"] == "action", use_next_states=c["pair"] == "next_state")
    if gail:
        net = nw.DiscriminatorNetwork(input_shape=(in_dim,), output_shape=(1,), n_features=[512, 256],
                                      activations=["tanh", "tanh", "identity"], squeeze_out=False, standardizer=stand, **flags)
        lins = list(net._linears)
        loss_fn = im.GailDiscriminatorLoss(entcoeff=c["entcoeff"])
        cls = ns.gail.GAIL
    else:
        enc = nw.FullyConnectedNetwork(input_shape=(in_dim,), output_shape=(128,), n_features=[256],
                                       activations=["relu", "relu"], standardizer=None, squeeze_out=False)
        dec = nw.FullyConnectedNetwork(input_shape=(128,), output_shape=(1,), n_features=[], activations=["identity"],
                                       standardizer=None, squeeze_out=False)
        net = nw.VariationalNet(input_shape=(in_dim,), output_shape=(1,), z_size=128, encoder_net=enc, decoder_net=dec,
                                standardizer=stand, **flags)
        lins = [enc._linears[0], enc._linears[1], net.mu_out, net.logvar_out, dec._linears[0]]
        loss_fn = im.VDBLoss(info_constraint=c["info_c"], lr_beta=c["lr_beta"], entcoeff=c["entcoeff"])
        loss_fn._beta = c["beta"]
        cls = gp.ns_vail(ns).VAIL
    with torch.no_grad():
        for i, p in enumerate(params(case, seed)):
            (lins[i // 2].weight if i % 2 == 0 else lins[i // 2].bias).copy_(torch.from_numpy(p))

    blocks = noise(case)
    calls = [0]

    def randn_like(t):
        k = calls[0]
        calls[0] += 1
        if k >= 6:                      # forward 7 keeps mu and logvar only: its draw reaches no scalar
            return torch.zeros_like(t)
        assert tuple(blocks[k].shape) == tuple(t.shape), (k, blocks[k].shape, t.shape)
        return torch.from_numpy(blocks[k]).to(t.dtype)

    def regressor_call(*arrays):
        # ---- RESTATEMENT (a reading) of mushroom-rl's Regressor.__call__ / TorchApproximator.predict: the network's
        # forward over the whole batch, tensors in, numpy out
        with torch.no_grad():
            y = net(*[torch.from_numpy(np.asarray(a)) for a in arrays])
        return tuple(v.detach().numpy() for v in y) if isinstance(y, tuple) else y.detach().numpy()
        # ---- end of the restatement

    im.to_float_tensor = lambda a: torch.as_tensor(a).float()      # RESTATEMENT of mushroom_rl.utils.torch.to_float_tensor
    agent = cls.__new__(cls)
    sw = Recorder()
    agent._sw, agent._loss, agent._D, agent._iter = sw, loss_fn, regressor_call, ITER
    agent._state_mask = gp.STATE_MASK
    agent._use_next_state = c["pair"] == "next_state"
    agent._act_mask = gp.ACT_MASK if c["pair"] == "action" else np.array([], dtype=np.int64)
    inputs = (x,) if x2 is None else (x, x2.astype(np.float32))
    t = targets[:, None] if targets is not None else np.concatenate(
        [np.zeros(shape=(N_PLCY, 1)), np.ones(shape=(N_PLCY, 1))]).astype(np.float32)      # gail_TRPO.py:213-216
    orig = torch.randn_like
    torch.randn_like = randn_like
    try:
        agent._discriminator_logging(inputs, t)
    finally:
        torch.randn_like = orig
    assert calls[0] == (0 if gail else 7)
    if not gail:
        assert float(loss_fn._beta) == c["beta"]         # the agent's own loss is untouched: the copies took the updates
    tags = [r[0] for r in sw.rows]
    arrays = {"tags": np.array(tags), "values": np.array([r[1] for r in sw.rows], dtype=np.float64),
              "steps": np.array([r[2] for r in sw.rows], dtype=np.int64), "iter": np.int64(ITER),
              "st0_count": st0[0], "st0_sum": st0[1], "st0_sumsq": st0[2],
              "st_count": np.asarray(stand._count, dtype=np.float64), "st_sum": np.asarray(stand._sum),
              "st_sumsq": np.asarray(stand._sumsq), "param_seed": np.int64(seed), "prior_seed": np.int64(c["prior_seed"]),
              "draw_seed": np.int64(c["draw_seed"]), "demo_idx": idx.astype(np.int32), "entcoeff": np.float64(c["entcoeff"])}
    if not gail:
        arrays.update(noise_seed=np.int64(c["noise_seed"]), info_c=np.float64(c["info_c"]), lr_beta=np.float64(c["lr_beta"]),
                      beta=np.float64(c["beta"]),
                      noise_head=np.stack([b[0, :8] for b in blocks]), noise_sum=np.array([b.sum(dtype=np.float64) for b in blocks]))
    return arrays


def main():
    out_dir = os.path.join(HERE, "disc_log")
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
        print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB; seed {int(arrays['param_seed'])}; "
              + ", ".join(f"{t}={v:.6g}" for t, v in zip(arrays["tags"], arrays["values"])))


if __name__ == "__main__":
    main()
