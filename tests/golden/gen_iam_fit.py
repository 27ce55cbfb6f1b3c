"""Generate tests/golden/iam_fit/{iqfo,lsiqfo}.npz by EXECUTING the reference's own from-observations agents:
IQfO_SAC.fit and train_action_model (imitation_lib/imitation/iqfo_sac.py:59-120, 133-268), LSIQfO.fit
(imitation_lib/imitation/lsiqfo.py:59-123, with its np.clip at :90), IQ_SAC.iq_update / LSIQ's critic loss under them,
and GaussianInvActionModel.fit / draw_action / __call__ / entropy / get_mu_log_sigma
(imitation_lib/utils/action_models.py:322-503), imported from the reference tree under gen_iq_q_update.install_stubs(),
on the reference's FullyConnectedNetwork and Standardizer.  Run in the build container:

    python tests/golden/gen_iam_fit.py [--out DIR]

fit() runs whole for four iterations, every one logging.  The agent is built with __new__ and given the attributes its
methods read, as gen_iq_pi_update.py and gen_lsiq_h_update.py build theirs; the action model likewise.  mushroom-rl is
absent, so two things fit reaches through it are the generator's own code and marked: `Memory` stands in for
ReplayMemory (add, initialized, size, get(n)) and serves the stored index arrays in the order fit asks for them (the
fits_per_step model batches, the logging sample, the policy batch: get asserts each size, so a different order would
fail here); `minibatch_generator` serves the stored demonstration rows (train_action_model's sample, then fit's).
_optimize_actor_parameters is restated as in gen_iq_pi_update.py.

The setting is the issue's: in = 6 (row width 12), A = 5, batch 9, action-model batch 7, fits_per_step = 2,
Standardizers on all networks, the model's Adam(lr = 1e-3) and log_std in [-5, 2], the agent's hyperparameters
iam_restate.FO.  The replay actions lie at and beyond the bounds (|u| >= 1 in both fixtures).  The noise of all eight
sampled passes of an iteration (the two logging draws, the expert draw, iq_update's five) is recovered by
gen_iq_q_update's rsample wrapper.

Stored: the inputs, samples and noise; the action model's parameters per iteration, its statistics, the eight
Action-Model/... scalars and the drawn expert actions; the policy, the critic and its target after the run, their
statistics, the Actor/... scalars.  Per group the largest |reference float32 - float64 twin| (tests/iam_restate.py:
sequence_twin for the model, fo_fit_twin for the whole fit); tests allow max(2e-5, 4 x spread).  Two wrong readings run
through both twins and must miss by more than that; by how much is stored: `draw` (the expert draw does not feed the
model's Standardizer) and `logging` (the logging passes do not); through the drawn actions they reach the critic and
the policy.  Fixed member dates: running the generator again reproduces the files byte for byte.  Data only."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "iam_fit")
if __name__ == "__main__" and "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_bc_fit as fit  # noqa: E402  (write_npz)
import gen_iq_q_update as gq  # noqa: E402  (install_stubs, Reg, w2_init, params_of, stats_of)
import iam_restate as ir  # noqa: E402

RING, DEMO = 40, 30
NAMES = gq.NAMES
W2_SEED = 13
ACTOR_TAGS = ("Actor/Loss", "Gradients/Norm2 Gradient Q wrt. Pi-parameters", "Actor/Entropy Expert States",
              "Actor/Entropy Policy States", "Actor/Entropy from Gaussian Policy States", "Actor/Entropy Lower Bound",
              "Actor/Entropy from Gaussian Expert States")
SPECS = {"iqfo": dict(clip=False, seed=1), "lsiqfo": dict(clip=True, seed=2)}


def inputs(seed):
    rng = np.random.default_rng(9100 + seed)
    D, A, T = ir.SEQ_IN, ir.SEQ_A, ir.SEQ_ITERS
    f = np.float32
    scale, shift = rng.uniform(0.3, 3.0, D), rng.standard_normal(D) * 2.0
    min_a, max_a = -rng.uniform(0.5, 2.0, A), rng.uniform(0.5, 3.0, A)
    central, delta = (0.5 * (max_a + min_a)).astype(f), (0.5 * (max_a - min_a)).astype(f)

    def block(n):
        s = (rng.standard_normal((n, D)) * scale + shift).astype(f)
        ns = (s + 0.1 * rng.standard_normal((n, D)) * scale).astype(f)
        a = (central + delta * np.tanh(rng.standard_normal((n, A)))).astype(f)
        return s, ns, a
    ring_s, ring_ns, ring_a = block(RING)
    where = rng.uniform(0, 1, ring_a.shape)
    ring_a = np.where(where < 0.08, f(min_a)[None, :], ring_a)
    ring_a = np.where(where > 0.92, (f(max_a) + f(0.25))[None, :], ring_a).astype(f)
    demo_s, demo_ns, demo_a = block(DEMO)
    assert (np.abs((ring_a - central) / delta) >= 1).any()
    return dict(ring_s=ring_s, ring_ns=ring_ns, ring_a=ring_a, demo_s=demo_s, demo_ns=demo_ns, demo_a=demo_a,
                central=central, delta=delta, min_a=min_a, max_a=max_a,
                ring_abs=(rng.uniform(0, 1, RING) < 0.15).astype(f), demo_abs=(rng.uniform(0, 1, DEMO) < 0.15).astype(f),
                ip_fit=rng.integers(0, RING, (T, ir.SEQ_B)),
                fit_idx=rng.integers(0, RING, (T, ir.SEQ_FITS, ir.SEQ_AMB)), ip=rng.integers(0, RING, (T, ir.SEQ_AMB)),
                ie=np.stack([rng.permutation(DEMO)[:ir.SEQ_AMB] for _ in range(T)]),
                ie_draw=np.stack([rng.permutation(DEMO)[:ir.SEQ_B] for _ in range(T)]))


AM_TAGS = ("Action-Model/Loss Policy", "Action-Model/Loss Exp", "Action-Model/Entropy Plcy", "Action-Model/Entropy Exp",
           "Action-Model/Std Exp", "Action-Model/Std", "Action-Model/Mu Exp", "Action-Model/Mu")


class Memory:
    """The generator's own stand-in for mushroom-rl's ReplayMemory as IQfO_SAC.fit uses it: add() (the ring is fixed:
    its 40 transitions are there from the start), initialized, size, and get(n), which serves the stored index arrays
    in the order fit asks for them: fits_per_step samples of the model's batch, the logging sample, the policy batch."""

    def __init__(self, fx):
        self.fx, self.it, self.k, self.size, self.initialized = fx, 0, 0, RING, True

    def add(self, dataset):
        pass

    def get(self, n):
        fx, k = self.fx, self.k
        idx = fx["fit_idx"][self.it, k] if k < ir.SEQ_FITS else fx["ip"][self.it] if k == ir.SEQ_FITS else fx["ip_fit"][self.it]
        assert len(idx) == n
        self.k += 1
        if self.k == ir.SEQ_FITS + 2:
            self.k, self.it = 0, self.it + 1
        z = np.zeros(n, np.float32)
        return fx["ring_s"][idx], fx["ring_a"][idx], z, fx["ring_ns"][idx], fx["ring_abs"][idx], z


def run(name, spec):
    import types
    from copy import deepcopy
    import torch
    to_parameter = gq.install_stubs()

    class Serializable:      # inert: action_models.py imports it as a base class
        def _add_save_attr(self, **kw):
            pass
    sys.modules["mushroom_rl.core"].Serializable = Serializable
    for mod, attr in (("mushroom_rl.approximators", "Regressor"), ("mushroom_rl.approximators.parametric", "TorchApproximator")):
        if not hasattr(sys.modules[mod], attr):
            setattr(sys.modules[mod], attr, object)
    nw = importlib.import_module("imitation_lib.utils.networks")
    am = importlib.import_module("imitation_lib.utils.action_models")
    iq = importlib.import_module("imitation_lib.imitation.iq_sac")
    fo = importlib.import_module("imitation_lib.imitation.lsiqfo" if spec["clip"] else "imitation_lib.imitation.iqfo_sac")
    to_float_tensor = sys.modules["mushroom_rl.utils.torch"].to_float_tensor
    fx = inputs(spec["seed"])
    A, IN, D, F = ir.SEQ_A, ir.SEQ_IN, 2 * ir.SEQ_IN, ir.FO
    mk = lambda i, o: nw.FullyConnectedNetwork(input_shape=(i,), output_shape=(o,), n_features=[512, 256],
                                               activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    torch.manual_seed(7)
    net, pnet, cnet = mk(D, 2 * A), mk(IN, 2 * A), mk(IN + A, 1)
    with torch.no_grad():
        net._linears[1].weight.copy_(torch.from_numpy(gq.w2_init(W2_SEED)))
        pnet._linears[1].weight.copy_(torch.from_numpy(gq.w2_init(W2_SEED + 1)))
        pnet._linears[2].weight.mul_(gq.W3_SCALE)
        cnet._linears[1].weight.copy_(torch.from_numpy(gq.w2_init(W2_SEED + 2)))
    tnet = deepcopy(cnet)
    init, p_init, c_init = gq.params_of(net), gq.params_of(pnet), gq.params_of(cnet)
    m = am.GaussianInvActionModel.__new__(am.GaussianInvActionModel)
    m._approximator, m._target_approximator, m._use_cuda = gq.Reg(net), None, False
    m._action_model_loss = torch.nn.GaussianNLLLoss()
    m._action_model_optimizer = torch.optim.Adam(net.parameters(), lr=ir.SEQ_LR)
    m._output_shape, m._half_out_shape = 2 * A, A
    m._delta_a = to_float_tensor(.5 * (fx["max_a"] - fx["min_a"]))
    m._central_a = to_float_tensor(.5 * (fx["max_a"] + fx["min_a"]))
    m.use_mean, m._eps_log_prob = False, 1e-6
    m._log_std_min, m._log_std_max = to_parameter(ir.SEQ_LO), to_parameter(ir.SEQ_HI)

    # the agent, built with __new__ and given the attributes fit, train_action_model and iq_update read (as
    # gen_iq_pi_update.py and gen_lsiq_h_update.py build theirs)
    policy = iq.IQ_Learn_Policy(gq.Reg(pnet), fx["min_a"], fx["max_a"], F["ls_min"], F["ls_max"])
    cls = fo.LSIQfO if spec["clip"] else fo.IQfO_SAC
    ag = cls.__new__(cls)
    ag.mdp_info = types.SimpleNamespace(gamma=F["gamma"], action_space=types.SimpleNamespace(low=fx["min_a"], high=fx["max_a"]))
    ag.policy, ag._use_cuda = policy, False
    ag._critic_approximator, ag._target_critic_approximator = gq.Reg(cnet), gq.Reg(tnet)
    ag._use_target = True
    ag._log_alpha = torch.tensor(np.log(F["init_alpha"]), dtype=torch.float32).requires_grad_()
    ag._alpha_optim = torch.optim.Adam([ag._log_alpha], lr=3e-4)
    ag._learnable_alpha, ag._target_entropy = False, -np.float32(A)
    ag._plcy_loss_mode, ag._regularizer_mode = "value", "exp_and_plcy"
    ag._gp_lambda, ag._reg_mult, ag._treat_absorbing_states = 0.0, F["reg_mult"], False
    ag._R_min, ag._R_max = 0.0, 1.0
    if spec["clip"]:
        ag._Q_max, ag._Q_min, ag._loss_mode_exp, ag._Q_exp_loss = F["Q_max"], F["Q_min"], "fix", "MSE"
        ag._target_clipping, ag._lossQ_type = True, "iq_like"
    ag._iter, ag._logging_iter, ag._sw = 1, 1, gq.Recorder()
    ag._tau = to_parameter(F["tau"])
    ag._delay_Q, ag._delay_pi, ag._warmup_transitions = 1, 1, to_parameter(0)
    ag._train_policy_only_on_own_states = False
    ag._critic_optimizer = torch.optim.Adam(cnet.parameters(), lr=F["lr"])
    actor_optimizer = torch.optim.Adam(pnet.parameters(), lr=F["lr_actor"])

    def _optimize_actor_parameters(loss):
        # RESTATEMENT of mushroom-rl's DeepAC._optimize_actor_parameters (no clipping)
        actor_optimizer.zero_grad()
        loss.backward()
        actor_optimizer.step()
    ag._optimize_actor_parameters = _optimize_actor_parameters
    # what IQfO_SAC's own constructor sets (iqfo_sac.py:36-48)
    ag._action_model = m
    ag._action_model_fit_params = dict(fits_per_step=ir.SEQ_FITS, init_epochs=0)
    ag._action_model_initialized, ag._action_model_batch_size = False, ir.SEQ_AMB
    ag._add_noise_to_obs, ag.ext_normalizer_action_model = False, None
    ag._interpolate_expert_states, ag._interpolation_coef = False, 1.0
    ag._state_mask = np.arange(IN)
    ag._batch_size = to_parameter(ir.SEQ_B)
    ag._demonstrations = dict(states=fx["demo_s"], next_states=fx["demo_ns"], absorbing=fx["demo_abs"], actions=fx["demo_a"])
    ag._replay_memory = Memory(fx)
    served = []

    def minibatch_generator(batch_size, *arrays):
        # the generator's own stand-in for mushroom_rl.utils.minibatches.minibatch_generator: the stored demonstration
        # rows, first train_action_model's sample (with actions), then fit's (with absorbing)
        it, k = divmod(len(served), 2)
        idx = (fx["ie"] if k == 0 else fx["ie_draw"])[it]
        assert len(idx) == batch_size and len(arrays) == 3
        served.append(k)
        yield tuple(a[idx] for a in arrays)
    fo.minibatch_generator = minibatch_generator

    eps_log = []
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
    drawn, snaps, stats = [], [], []
    draw0 = m.draw_action

    def draw_action(state, n_state):          # __call__ goes through it too: the expert draw of fit is the one of B rows
        a = draw0(state, n_state)
        if len(a) == ir.SEQ_B:
            drawn.append(np.asarray(a, np.float64))
        return a
    m.draw_action = draw_action
    Normal.rsample = rsample
    torch.manual_seed(43)
    try:
        for it in range(ir.SEQ_ITERS):
            ag.fit(None)                      # IQfO_SAC.fit / LSIQfO.fit whole
            snaps.append(gq.params_of(net))
            stats.append(gq.stats_of(net._stand, D))
    finally:
        Normal.rsample = rsample0
    order = ("plcy", "exp", "draw", "next", "expert", "pi", "ppi", "plog")
    assert len(eps_log) == len(order) * ir.SEQ_ITERS and len(served) == 2 * ir.SEQ_ITERS and ag._iter == 1 + ir.SEQ_ITERS
    for k, key in enumerate(order):
        fx["eps_" + key] = np.stack(eps_log[k::len(order)])
    assert fx["eps_draw"].shape == (ir.SEQ_ITERS, ir.SEQ_B, A) and fx["eps_plog"].shape == (ir.SEQ_ITERS, 2 * ir.SEQ_B, A)
    rows = ag._sw.rows
    am_scal = np.array([[rows[i + 1][t] for t in AM_TAGS] for i in range(ir.SEQ_ITERS)])
    actor_scal = np.array([[rows[i + 1][t] for t in ACTOR_TAGS] for i in range(ir.SEQ_ITERS)])
    if spec["clip"]:
        drawn = [np.clip(a, fx["min_a"], fx["max_a"]) for a in drawn]          # lsiqfo.py:90, as fit applies it
    ref = dict(params=[[s[n].astype(np.float64) for n in NAMES] for s in snaps], colstats=np.stack(stats),
               scalars=am_scal, drawn=np.stack(drawn))
    p0 = [init[n] for n in NAMES]
    pick = lambda t: t["scalars"][:, 2:]           # the twin's row holds the two fit losses first, which fit does not log
    twin = ir.sequence_twin(fx, p0, clip=spec["clip"])
    spread = group_miss(ref, dict(twin, scalars=pick(twin)))
    assert spread["params"] < 1e-5, spread

    # ---- the whole fit: the float64 twin and the two wrong readings, on all three networks
    fin = dict(policy=gq.params_of(pnet), critic=gq.params_of(cnet), target=gq.params_of(tnet))
    flat = lambda d: np.concatenate([np.asarray(d[n], np.float64).reshape(-1) for n in NAMES])
    cat = lambda xs: np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])
    algo = "lsiqfo" if spec["clip"] else "iqfo"

    def whole(wrong=None):
        t = ir.fo_fit_twin(fx, algo, p0, [p_init[n] for n in NAMES], [c_init[n] for n in NAMES], wrong=wrong)
        tscal = np.array([[t["actor_scalars"][i + 1][k] for k in ACTOR_TAGS] for i in range(ir.SEQ_ITERS)])
        return dict(policy=float(np.abs(flat(fin["policy"]) - cat(t["policy"]["params"])).max()),
                    critic=float(np.abs(flat(fin["critic"]) - cat(t["critic"]["params"])).max()),
                    target=float(np.abs(flat(fin["target"]) - cat(t["critic"]["target"])).max()),
                    actor_scalars=float(np.abs(actor_scal - tscal).max())), t
    sp, t = whole()
    print(name, "model spread", spread, "agent spread", sp)
    assert max(sp["policy"], sp["critic"], sp["target"]) < 1e-5, "the float64 twin does not follow the reference"
    pst, cst = gq.stats_of(pnet._stand, IN), gq.stats_of(cnet._stand, IN + A)
    tst = gq.stats_of(tnet._stand, IN + A)
    assert np.abs(pst[0] - t["policy"]["colstats"][0]).max() < 1e-9 and np.abs(cst[0] - t["critic"]["colstats"][0]).max() < 1e-9
    miss, miss_model = {}, {}
    for w in ("draw", "logging"):
        d = group_miss(ref, (lambda tw: dict(tw, scalars=pick(tw)))(ir.sequence_twin(fx, p0, wrong=w, clip=spec["clip"])))
        miss_model[w] = max(d["params"], d["scalars"])
        miss[w] = whole(w)[0]
    print(name, "miss (model)", miss_model, "miss (agent)", miss)
    out = {k: v for k, v in fx.items()}
    for n in NAMES:
        if n != "w2":
            out[f"init_{n}"], out[f"policy_init_{n}"], out[f"critic_init_{n}"] = init[n], p_init[n], c_init[n]
            for g in fin:
                out[f"{g}_{n}"] = fin[g][n]
            for it in range(ir.SEQ_ITERS):
                out[f"{n}_it{it}"] = snaps[it][n]
    out["w2_rows_final"] = snaps[-1]["w2"][:16]
    for g in fin:
        out[f"{g}_w2_head"] = fin[g]["w2"][:16]
    out.update(colstats=ref["colstats"], scalars=ref["scalars"], drawn=ref["drawn"], actor_scalars=actor_scal,
               policy_colstats=pst, critic_colstats=cst, target_colstats=tst)
    for g, v in spread.items():
        out[f"spread_{g}"] = np.float64(v)
    for g, v in sp.items():
        out[f"spread_{g}"] = np.float64(v)
    for w in miss:
        out[f"miss_{w}"] = np.float64(miss_model[w])
        out[f"miss_{w}_critic"] = np.float64(miss[w]["critic"])
        out[f"miss_{w}_policy"] = np.float64(miss[w]["policy"])
    os.makedirs(OUT_DIR, exist_ok=True)
    fit.write_npz(os.path.join(OUT_DIR, name + ".npz"), out)
    print(name, os.path.getsize(os.path.join(OUT_DIR, name + ".npz")))


def group_miss(ref, twin):
    """The largest |a - b| per tensor group; layer 2's weights count whole."""
    far = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max())
    p = max(far(a, b) for ra, rb in zip(ref["params"], twin["params"]) for a, b in zip(ra, rb))
    return dict(params=p, colstats=far(ref["colstats"], twin["colstats"]), scalars=far(ref["scalars"], twin["scalars"]),
                drawn=far(ref["drawn"], twin["drawn"]))


def main():
    for name, spec in SPECS.items():
        run(name, spec)


if __name__ == "__main__":
    main()
