#!/usr/bin/env python3
"""Generate tests/golden/iq_q_update/{iq_target,iq_notarget,sqil}.npz by EXECUTING the reference's own critic update:
IQ_SAC.update_Q_function, _lossQ, getV, get_targetV, regularizer_loss, update_Q_parameters, logging_loss and
_update_all_targets (imitation_lib/imitation/iq_sac.py:421-429, 467-595, 621-647, 674-676), SQIL._lossQ
(imitation_lib/imitation/sqil_sac.py:64-136) and IQ_Learn_Policy (iq_sac.py:18-167), imported from the reference tree
under the inert stubs of _ref_stubs.py, on the reference's FullyConnectedNetwork and Standardizer
(imitation_lib/utils/networks.py).  Run in the build container only:

    python tests/golden/gen_iq_q_update.py [--out DIR]

The setting: policy 12 -> [512, 256] -> 10 and critic 17 -> [512, 256] -> 1, both with Standardizers, B = 18 rows of which
the first n_policy = 9 are the policy's (so the obs | act seam and the policy | expert seam both fall inside a 16-wide
tile), about a fifth of the rows absorbing in both halves, 4 iterations, every one logging, Adam(lr = 3e-4) on the
critic, tau = 0.005, gamma = 0.99, alpha = exp(float32(log 1e-3)).  iq_target: plcy_loss_mode value, regularizer
exp_and_plcy, a target.  iq_notarget: the same without one.  sqil: SQIL with plcy_loss_mode value, R_min 0, R_max 1, a
target (value runs the pass on obs, which plcy does not, and SQIL logs AFTER that pass where IQ logs before it).

The agents are built with __new__ and given the attributes those methods read.  IQ: update_Q_function, then
_update_all_targets, then _iter += 1 (fit's and iq_update's lines).  SQIL: its iq_update's lines (_lossQ, the LossQ scalar,
_update_target), because the inherited update_Q_function unpacks three losses.

mushroom-rl is absent, so what goes through it is RESTATED below and marked: the Regressor's call (the network's
forward on tensors; a numpy action, getV's round trip, becomes a tensor again), get_weights / set_weights (the flat
float32 vector), to_float_tensor, to_parameter, and DeepAC._update_target (float32 arrays times a Python float:
f32(tau) * w + f32(1 - tau) * t, two products and one add).  DeepAC, Policy and ReplayMemory are inert.

The noise: Normal.rsample is wrapped: the generator's state is saved, the sample drawn, the state restored and the same
standard normal drawn again (rsample is loc + eps * scale with eps = torch.empty(shape).normal_()); the wrapper asserts
that mu + sigma * eps reproduces the sample bit for bit and stores eps.  The actions and log-probabilities the policy
returned on next_obs and on obs are stored too (a_next, logp_next, a_pi, logp_pi): the CPU test feeds them to the twin.  Per iteration IQ draws for next_obs (18 rows),
the expert rows (9, logging_loss's draw_action) and obs (18); SQIL for next_obs, obs and then the expert rows.

The float64 twin is tests/iq_restate.py (torch autograd and Adam, the statistics pass by pass) in float64 on the actions
and log-probabilities the reference run produced; the reference's forward narrows its input to float32 by its own
line, so its lines cannot run in float64 themselves.  Stored per tensor group (parameters, target, scalars, statistics):
the largest |reference float32 - float64 twin|.  The tests allow 4 x that spread and never less than 2e-5 for the
parameters (the factor covers an fma-chain order other than torch's, as for kl in DESIGN section 17).  Measured at the
first setting tried, which was kept: 4.1e-6 (iq_target), 5.8e-6 (iq_notarget: its tolerance is 4 x that, 2.3e-5) and the
spread printed for sqil.  Part of it is the reference's Standardizer summing the float32 rows in float32 (numpy's
x.sum on the tensor's own array) where the twin and the device add them in float64.  Asserted here: the parameter
spread stays under 1e-5, a hundredth of what either wrong reading below misses by, so the twin follows the reference.

Two wrong readings are run through the twin and must miss the true run's parameters by more than the tolerance; by how
much is stored: one_stats (the live Standardizer takes every pass's rows first and all passes are standardised alike)
and shared_target (the target goes through the live Standardizer).  shared_target does not apply without a target (the
target network is never run): 0 is stored there.

Layer 2's initial weights (256 x 512 each) are seeded numpy draws, w2_init(seed), rebuilt by the tests; of the stepped
layer-2 weights the first 16 rows are stored.  The archives have fixed member dates (gen_bc_fit.write_npz): running the
generator again reproduces the files byte for byte.  The fixtures hold data only.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "iq_q_update")
if __name__ == "__main__" and "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_bc_fit as fit  # noqa: E402  (write_npz)

IN_DIM, ACT_DIM, B, N_POLICY, N_ITER = 12, 5, 18, 9, 4
D = IN_DIM + ACT_DIM
LR, TAU, GAMMA, INIT_ALPHA, REG_MULT = 3e-4, 0.005, 0.99, 1e-3, 0.5
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
W3_SCALE, LOG_SIGMA_SHIFT = 0.1, -0.5      # the policy's output layer, as gen_bc_log.py: a well-conditioned log-probability
NAMES = fit.NAMES
TOL = 2e-5
W2_HEAD = 16
FIXTURES = dict(iq_target=dict(algo="iq", mode="value", reg="exp_and_plcy", use_target=True),
                iq_notarget=dict(algo="iq", mode="value", reg="exp_and_plcy", use_target=False),
                sqil=dict(algo="sqil", mode="value", reg="exp_and_plcy", use_target=True))
ACTION_TAGS = ("Actions/mean squared action expert (from data)", "Actions/mean squared action expert (from policy)",
               "Actions/mean squared action policy", "Actions/mean squared action both", "Action-Value/Norm of Q net: ")


def w2_init(seed):
    """A layer-2 initial weight: uniform in -+sqrt(2) sqrt(6 / (512 + 256)) (xavier_uniform_ with relu's gain) on a
    PCG64(seed) draw.  Seed 11: the policy, seed 12: the critic."""
    bound = np.sqrt(2.0) * np.sqrt(6.0 / (512 + 256))
    return np.random.default_rng(seed).uniform(-bound, bound, (256, 512)).astype(np.float32)


def inputs():
    """Per iteration obs, next_obs [4,18,12], act [4,18,5] in the action bounds, absorbing [4,18] with rows 1, 6 (policy)
    and 11, 16 (expert) set and one more drawn per iteration; min_a, max_a f64 of unequal widths."""
    rng = np.random.default_rng(29)
    scale, shift = rng.uniform(0.3, 3.0, IN_DIM), rng.standard_normal(IN_DIM) * 2.0
    obs = (rng.standard_normal((N_ITER, B, IN_DIM)) * scale + shift).astype(np.float32)
    nxt = (obs + 0.1 * rng.standard_normal((N_ITER, B, IN_DIM)) * scale).astype(np.float32)
    min_a, max_a = -rng.uniform(0.5, 2.0, ACT_DIM), rng.uniform(0.5, 3.0, ACT_DIM)
    u = np.tanh(0.8 * rng.standard_normal((N_ITER, B, ACT_DIM)))
    act = (0.5 * (max_a + min_a) + 0.5 * (max_a - min_a) * u).astype(np.float32)
    absorbing = np.zeros((N_ITER, B), np.float32)
    absorbing[:, [1, 6, 11, 16]] = 1.0
    for i in range(N_ITER):
        absorbing[i, rng.integers(0, B)] = 1.0
    return obs, act, nxt, absorbing, min_a, max_a


def install_stubs():
    """_ref_stubs.install() and the extra stand-ins iq_sac.py and sqil_sac.py import.  Inert: DeepAC (but for
    _update_target, RESTATED), Policy, ReplayMemory.  RESTATED: to_float_tensor, to_parameter."""
    import torch
    import _ref_stubs as stubs
    stubs.install()

    class Parameter:
        # RESTATEMENT of mushroom_rl.utils.parameters.Parameter: a constant value behind a call
        def __init__(self, value):
            self._value = value

        def __call__(self, *a, **k):
            return self._value

        def get_value(self, *a, **k):
            return self._value

    def to_parameter(x):
        return x if isinstance(x, Parameter) else Parameter(x)

    def to_float_tensor(x, use_cuda=False):
        # RESTATEMENT of mushroom_rl.utils.torch.to_float_tensor
        return torch.tensor(x, dtype=torch.float)

    class DeepAC:
        def _update_target(self, online, target):
            # RESTATEMENT of DeepAC._update_target for one model per Regressor
            weights = self._tau() * online.get_weights()
            weights += (1 - self._tau.get_value()) * target.get_weights()
            target.set_weights(weights)

    class Policy:
        def _add_save_attr(self, **kw):
            pass

    class ReplayMemory:
        def __init__(self, *a, **k):
            pass

    sys.modules["mushroom_rl.utils.torch"].to_float_tensor = to_float_tensor
    stubs._mod("mushroom_rl.utils.replay_memory", ReplayMemory=ReplayMemory)
    stubs._mod("mushroom_rl.utils.parameters", to_parameter=to_parameter, Parameter=Parameter)
    sys.modules["mushroom_rl.algorithms.actor_critic.deep_actor_critic"].DeepAC = DeepAC
    stubs._mod("mushroom_rl.policy", Policy=Policy)
    return to_parameter


class Reg:
    """RESTATEMENT of Regressor(TorchApproximator, network=...) as these methods use it: the call and predict are the
    network's forward on tensors, get_weights / set_weights the flat float32 vector of its parameters."""

    def __init__(self, network):
        self.model = types.SimpleNamespace(network=network, use_cuda=False)

    def __call__(self, *x, output_tensor=False, **kw):
        import torch
        ts = [a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)) for a in x]
        y = self.model.network(*ts)
        return y if output_tensor else y.detach().numpy()

    predict = __call__

    def get_weights(self):
        return np.concatenate([p.data.detach().numpy().flatten() for p in self.model.network.parameters()])

    def set_weights(self, w):
        import torch
        o = 0
        for p in self.model.network.parameters():
            n = p.numel()
            p.data = torch.from_numpy(np.asarray(w[o:o + n], np.float32).reshape(tuple(p.shape)).copy())
            o += n


class Recorder:
    def __init__(self):
        self.rows = {}

    def add_scalar(self, name, val, it):
        import torch
        self.rows.setdefault(int(it), {})[name] = float(val.detach()) if torch.is_tensor(val) else float(val)


def params_of(net):
    return {n: t.detach().numpy().copy() for n, t in zip(NAMES, [p for lin in net._linears for p in (lin.weight, lin.bias)])}


def stats_of(st, dim):
    """(count, sum, sumsq) of the rows alone [3, dim]: the Standardizer starts _count and _sumsq at 1e-2 (and holds
    scalars until its first rows)."""
    b = lambda v: np.broadcast_to(np.asarray(v, np.float64), (dim,))
    return np.stack([b(st._count) - 1e-2, b(st._sum), b(st._sumsq) - 1e-2])


def run(name, spec):
    import importlib
    import torch
    from copy import deepcopy
    to_parameter = install_stubs()
    nw = importlib.import_module("imitation_lib.utils.networks")
    iq = importlib.import_module("imitation_lib.imitation.iq_sac")
    sq = importlib.import_module("imitation_lib.imitation.sqil_sac")
    import _abi_tags
    obs, act, nxt, absorbing, min_a, max_a = inputs()
    torch.manual_seed(5)
    pnet = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(2 * ACT_DIM,), n_features=[512, 256],
                                    activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    cnet = nw.FullyConnectedNetwork(input_shape=(D,), output_shape=(1,), n_features=[512, 256],
                                    activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    with torch.no_grad():
        pnet._linears[1].weight.copy_(torch.from_numpy(w2_init(11)))
        pnet._linears[2].weight.mul_(W3_SCALE)
        pnet._linears[2].bias[ACT_DIM:].add_(LOG_SIGMA_SHIFT)
        cnet._linears[1].weight.copy_(torch.from_numpy(w2_init(12)))
    tnet = deepcopy(cnet)                             # target_critic_params = deepcopy(critic_params), iq_sac.py:291
    p_init, c_init = params_of(pnet), params_of(cnet)
    policy = iq.IQ_Learn_Policy(Reg(pnet), min_a, max_a, LOG_STD_MIN, LOG_STD_MAX)
    cls = iq.IQ_SAC if spec["algo"] == "iq" else sq.SQIL
    ag = cls.__new__(cls)
    ag.mdp_info = types.SimpleNamespace(gamma=GAMMA)
    ag.policy, ag._use_cuda = policy, False
    ag._critic_approximator, ag._target_critic_approximator = Reg(cnet), Reg(tnet)
    ag._use_target = spec["use_target"]
    ag._log_alpha = torch.tensor(np.log(INIT_ALPHA), dtype=torch.float32)
    ag._plcy_loss_mode, ag._regularizer_mode = spec["mode"], spec["reg"]
    ag._gp_lambda, ag._reg_mult, ag._treat_absorbing_states = 0.0, REG_MULT, False
    ag._R_min, ag._R_max = 0.0, 1.0
    ag._iter, ag._logging_iter, ag._sw = 1, 1, Recorder()
    ag._tau = to_parameter(TAU)
    ag._critic_optimizer = torch.optim.Adam(cnet.parameters(), lr=LR)
    alpha = float(ag._alpha)

    # the noise and the policy's outputs, pass by pass
    eps_log, pass_log = [], []
    Normal = torch.distributions.Normal
    rsample0 = Normal.rsample

    def rsample(self, sample_shape=torch.Size()):
        state = torch.get_rng_state()
        s = rsample0(self, sample_shape)
        torch.set_rng_state(state)
        eps = torch.empty(s.shape, dtype=torch.float32).normal_()
        assert torch.equal(s, self.loc + eps * self.scale), "eps does not reproduce rsample()"
        eps_log.append(eps.numpy().copy())
        return s
    cap0 = policy.compute_action_and_log_prob_t

    def cap(state, compute_log_prob=True):
        r = cap0(state, compute_log_prob=compute_log_prob)
        pass_log.append(tuple(t.detach().numpy().copy() for t in (r if compute_log_prob else (r,))))
        return r
    policy.compute_action_and_log_prob_t = cap
    Normal.rsample = rsample
    is_expert = torch.cat([torch.zeros(N_POLICY, dtype=torch.bool), torch.ones(B - N_POLICY, dtype=torch.bool)])
    torch.manual_seed(41)
    try:
        for i in range(N_ITER):
            args = (torch.from_numpy(obs[i]), torch.from_numpy(act[i]), torch.from_numpy(nxt[i]),
                    torch.from_numpy(absorbing[i]), is_expert)
            if spec["algo"] == "iq":
                ag.update_Q_function(*args)           # iq_update, :411-412
                ag._update_all_targets()              # :418-419
            else:
                lossQ = ag._lossQ(*args)              # SQIL.iq_update, sqil_sac.py:18-22
                ag.sw_add_scalar("IQ-Loss/LossQ", lossQ, ag._iter)
                ag._update_target(ag._critic_approximator, ag._target_critic_approximator)     # :60-62
            ag._iter += 1                             # fit, :405
    finally:
        Normal.rsample = rsample0
    assert len(eps_log) == len(pass_log) == 3 * N_ITER
    order = ("next", "expert", "pi") if spec["algo"] == "iq" else ("next", "pi", "expert")
    eps = {k: np.stack([eps_log[3 * i + order.index(k)] for i in range(N_ITER)]) for k in order}
    passes = {k: [pass_log[3 * i + order.index(k)] for i in range(N_ITER)] for k in order}

    tags = _abi_tags.IQ_Q_TAGS
    scal = np.full((N_ITER, 16), np.nan)
    extra = np.full((N_ITER, len(ACTION_TAGS)), np.nan)
    for i in range(N_ITER):
        row = ag._sw.rows[i + 1]
        for k, t in enumerate(tags):
            t = "IQ-Loss/LossQ" if (k == 0 and spec["algo"] == "sqil") else t
            if t in row:
                scal[i, k] = row[t]
        for k, t in enumerate(ACTION_TAGS):
            extra[i, k] = row[t]
    c_fin, t_fin = params_of(cnet), params_of(tnet)

    # ---- the float64 twin and the wrong readings (tests/iq_restate.py)
    import iq_restate as R
    cfg = R.Cfg(algo=spec["algo"], mode=spec["mode"], reg=spec["reg"], treat=False, use_target=spec["use_target"],
                standardizer=True, gamma=GAMMA, alpha=alpha, reg_mult=REG_MULT, R_min=0.0, R_max=1.0, lr=LR, tau=TAU)
    steps = [dict(obs=obs[i], act=act[i], next_obs=nxt[i], absorbing=absorbing[i], a_next=passes["next"][i][0],
                  logp_next=passes["next"][i][1], a_pi=passes["pi"][i][0], logp_pi=passes["pi"][i][1])
             for i in range(N_ITER)]
    init = [c_init[n] for n in NAMES]
    twin, twin_out = R.run(init, cfg, steps, N_POLICY)
    flat = lambda d: np.concatenate([np.asarray(d[n], np.float64).reshape(-1) for n in NAMES])
    sp_par = float(np.abs(flat(c_fin) - np.concatenate([a.reshape(-1) for a in twin["params"]])).max())
    sp_tgt = float(np.abs(flat(t_fin) - np.concatenate([a.reshape(-1) for a in twin["target"]])).max())
    logged = ~np.isnan(scal)
    sp_scal = float(np.abs(scal - twin_out)[logged].max())
    cs, tcs = stats_of(cnet._stand, D), stats_of(tnet._stand, D)
    sp_stat = max(float(np.abs(cs - twin["colstats"]).max()), float(np.abs(tcs - twin["tcolstats"]).max()))
    print(f"{name}: spreads params {sp_par:.3e} target {sp_tgt:.3e} scalars {sp_scal:.3e} statistics {sp_stat:.3e}")
    assert sp_par <= 1e-5 and sp_tgt <= 1e-5, "the float64 twin does not follow the reference"
    tol_par = max(TOL, 4 * sp_par)
    miss = {}
    for wrong in ("one_stats", "shared_target"):
        w, _ = R.run(init, cfg, steps, N_POLICY, wrong=wrong)
        miss[wrong] = float(np.abs(np.concatenate([a.reshape(-1) for a in w["params"]]) -
                                   np.concatenate([a.reshape(-1) for a in twin["params"]])).max())
        print(f"{name}: the {wrong} reading misses the parameters by {miss[wrong] / tol_par:.1f} tolerances")
        if wrong == "one_stats" or spec["use_target"]:
            assert miss[wrong] > tol_par, wrong
        else:
            assert miss[wrong] == 0.0
    arrays = dict(obs=obs, act=act, next_obs=nxt, absorbing=absorbing, min_a=min_a, max_a=max_a,
                  eps_next=eps["next"], eps_pi=eps["pi"], eps_expert=eps["expert"], scalars=scal, action_scalars=extra,
                  a_next=np.stack([p[0] for p in passes["next"]]), logp_next=np.stack([p[1] for p in passes["next"]]),
                  a_pi=np.stack([p[0] for p in passes["pi"]]), logp_pi=np.stack([p[1] for p in passes["pi"]]),
                  colstats=cs, target_colstats=tcs, policy_colstats=stats_of(pnet._stand, IN_DIM),
                  spread_params=np.float64(sp_par), spread_target=np.float64(sp_tgt), spread_scalars=np.float64(sp_scal),
                  spread_stats=np.float64(sp_stat), miss_one_stats=np.float64(miss["one_stats"]),
                  miss_shared_target=np.float64(miss["shared_target"]), lr=np.float64(LR), tau=np.float64(TAU),
                  gamma=np.float64(GAMMA), alpha=np.float64(alpha), reg_mult=np.float64(REG_MULT),
                  n_policy=np.int64(N_POLICY), use_target=np.int64(spec["use_target"]))
    for n in NAMES:
        if n != "w2":
            arrays[f"policy_init_{n}"] = p_init[n]
            arrays[f"critic_init_{n}"] = c_init[n]
            arrays[f"critic_{n}"] = c_fin[n]
            arrays[f"target_{n}"] = t_fin[n]
    arrays["critic_w2_head"], arrays["target_w2_head"] = c_fin["w2"][:W2_HEAD], t_fin["w2"][:W2_HEAD]
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    fit.write_npz(path, arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    # the tags of the 16 scalars live in olympic_hip._abi; imported by path so that the package's library is not needed
    import importlib.util
    root = os.path.dirname(os.path.dirname(HERE))
    spec = importlib.util.spec_from_file_location("_abi_tags", os.path.join(root, "olympics-mujoco_amd", "olympic_hip",
                                                                            "_abi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules["_abi_tags"] = mod
    for name, s in FIXTURES.items():
        run(name, s)


if __name__ == "__main__":
    main()
