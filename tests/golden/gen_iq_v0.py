#!/usr/bin/env python3
"""Generate tests/golden/iq_v0/*.npz by EXECUTING the reference's own critic update with plcy_loss_mode "v0":
IQ_SAC._lossQ (imitation_lib/imitation/iq_sac.py:467-563, the v0 branch at :508-510) and LSIQ._lossQ_iq_like
(imitation_lib/imitation/lsiq.py:33-112, :90-92) with everything they inherit (update_Q_function, getV, get_targetV,
regularizer_loss, update_Q_parameters, logging_loss, _update_all_targets) and IQ_Learn_Policy, imported from the reference
tree under the stubs and restatements of gen_iq_q_update.py (install_stubs, Reg, Recorder), on the reference's
FullyConnectedNetwork and Standardizer.  Run in the build container only:

    python tests/golden/gen_iq_v0.py [--out DIR]

The setting is gen_lsiq_q_update.py's: policy 12 -> [512, 256] -> 10, critic 17 -> [512, 256] -> 1, both with Standardizers,
B = 18 rows of which the first n_policy = 9 are the policy's, gen_iq_q_update's inputs, 4 iterations, every one logging,
tau = 0.005, gamma = 0.99, alpha = exp(float32(log 1e-3)), the critic's output layer scaled by 2 and shifted by 0.5, the
bounds Q_min = -0.25, Q_max = 0.3, Adam's lr 3e-5 (gen_lsiq_q_update.py says why).

The fixtures, each with the wrong readings (tests/iq_v0_restate.py) it must tell from the reference:
  iq_v0     IQ_SAC, v0, exp_and_plcy, a target                    v0_reuses_sample, v0_no_stats, v_pass_gradient
  lsiq_v0   LSIQ iq_like, fix / MSE, v0, clipping, exp, no target    v0_reuses_sample, v0_no_stats, v_pass_gradient
  lsiq_offline   LSIQ_Offline whole (run_offline below): B = 18 expert rows, fix / MSE, regularizer exp, a target, the
                 policy trained by its own update_policy (Adam, lr 3e-4)            the same three, on the critic

The agent is built with __new__ and given the attributes the methods read; per iteration update_Q_function, then
_update_all_targets, then _iter += 1.  The policy's noise is recorded as gen_iq_q_update.py records it; per iteration the
policy draws for next_obs (18 rows), the expert rows (9, logging_loss's draw_action), obs (18, getV(obs)) and the expert
rows again (9, getV(obs[is_expert]) of v0).

The float64 twin is tests/iq_v0_restate.py on the actions and log-probabilities the reference run produced.  Stored per
tensor group (parameters, target, scalars, statistics): the largest |reference float32 - float64 twin|; the tests allow
4 x that and never less than 2e-5.  Asserted here: the parameter spread stays under 1e-5; the twin's margins (no next_v
within 1e-3 of a bound, no pre-activation within 1e-6 of 0) hold at every update; each wrong reading misses the
true run's parameters by more than the tolerance (by how much is stored).  The fixtures hold data only and regenerate
byte for byte (gen_bc_fit.write_npz; main() writes each twice and compares)."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "iq_v0")
if __name__ == "__main__" and "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_bc_fit as fit  # noqa: E402  (write_npz)
import gen_iq_q_update as G  # noqa: E402
import gen_lsiq_q_update as GL  # noqa: E402

IN_DIM, ACT_DIM, B, N_POLICY, N_ITER, D = G.IN_DIM, G.ACT_DIM, G.B, G.N_POLICY, G.N_ITER, G.D
LR, TAU, GAMMA, INIT_ALPHA, REG_MULT = GL.LR, G.TAU, G.GAMMA, G.INIT_ALPHA, G.REG_MULT
Q_W3_SCALE, Q_B3_SHIFT, Q_MIN, Q_MAX = GL.Q_W3_SCALE, GL.Q_B3_SHIFT, GL.Q_MIN, GL.Q_MAX
NAMES, TOL, W2_HEAD, ACTION_TAGS, w2_init = G.NAMES, G.TOL, G.W2_HEAD, G.ACTION_TAGS, G.w2_init
WRONG = ("v0_reuses_sample", "v0_no_stats", "v_pass_gradient")
FIXTURES = dict(
    iq_v0=dict(algo="iq", exp_mode="bootstrap", exp_loss=None, clip=False, reg="exp_and_plcy", treat=False, use_target=True,
               wrong=WRONG),
    lsiq_v0=dict(algo="lsiq", exp_mode="fix", exp_loss="MSE", clip=True, reg="exp", treat=False, use_target=False,
                 wrong=WRONG))
PASSES = ("next", "expert", "pi", "v0")


def twin_cfg(spec, alpha, lr=LR, tau=TAU, gamma=GAMMA):
    import iq_v0_restate as V
    return V.LCfg(type="iq_like", exp_mode=spec["exp_mode"], exp_loss=spec["exp_loss"], clip=spec["clip"], q_min=Q_MIN,
                  q_max=Q_MAX, mode="v0", reg=spec["reg"], treat=spec["treat"], use_target=spec["use_target"],
                  standardizer=True, gamma=gamma, alpha=alpha, reg_mult=REG_MULT, lr=lr, tau=tau)


def run(name, spec, out_dir):
    import importlib
    import torch
    from copy import deepcopy
    to_parameter = G.install_stubs()
    nw = importlib.import_module("imitation_lib.utils.networks")
    iq = importlib.import_module("imitation_lib.imitation.iq_sac")
    ls = importlib.import_module("imitation_lib.imitation.lsiq")
    import _abi_tags
    obs, act, nxt, absorbing, min_a, max_a = G.inputs()
    torch.manual_seed(5)
    pnet = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(2 * ACT_DIM,), n_features=[512, 256],
                                    activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    cnet = nw.FullyConnectedNetwork(input_shape=(D,), output_shape=(1,), n_features=[512, 256],
                                    activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    with torch.no_grad():
        pnet._linears[1].weight.copy_(torch.from_numpy(w2_init(11)))
        pnet._linears[2].weight.mul_(G.W3_SCALE)
        pnet._linears[2].bias[ACT_DIM:].add_(G.LOG_SIGMA_SHIFT)
        cnet._linears[1].weight.copy_(torch.from_numpy(w2_init(12)))
        cnet._linears[2].weight.mul_(Q_W3_SCALE)
        cnet._linears[2].bias.mul_(Q_W3_SCALE).add_(Q_B3_SHIFT)
    tnet = deepcopy(cnet)                             # target_critic_params = deepcopy(critic_params), iq_sac.py:291
    p_init, c_init = G.params_of(pnet), G.params_of(cnet)
    policy = iq.IQ_Learn_Policy(G.Reg(pnet), min_a, max_a, G.LOG_STD_MIN, G.LOG_STD_MAX)
    cls = iq.IQ_SAC if spec["algo"] == "iq" else ls.LSIQ
    ag = cls.__new__(cls)
    ag.mdp_info = types.SimpleNamespace(gamma=GAMMA)
    ag.policy, ag._use_cuda = policy, False
    ag._critic_approximator, ag._target_critic_approximator = G.Reg(cnet), G.Reg(tnet)
    ag._use_target = spec["use_target"]
    ag._log_alpha = torch.tensor(np.log(INIT_ALPHA), dtype=torch.float32)
    ag._plcy_loss_mode, ag._regularizer_mode = "v0", spec["reg"]
    ag._gp_lambda, ag._reg_mult, ag._treat_absorbing_states = 0.0, REG_MULT, spec["treat"]
    ag._R_min, ag._R_max = 0.0, 1.0
    ag._Q_max, ag._Q_min, ag._loss_mode_exp, ag._Q_exp_loss = Q_MAX, Q_MIN, spec["exp_mode"], spec["exp_loss"]
    ag._target_clipping, ag._lossQ_type = spec["clip"], "iq_like"
    ag._iter, ag._logging_iter, ag._sw = 1, 1, G.Recorder()
    ag._tau = to_parameter(TAU)
    ag._critic_optimizer = torch.optim.Adam(cnet.parameters(), lr=LR)
    alpha = float(ag._alpha)

    # the noise and the policy's outputs, pass by pass (as gen_iq_q_update.py)
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
            ag.update_Q_function(torch.from_numpy(obs[i]), torch.from_numpy(act[i]), torch.from_numpy(nxt[i]),
                                 torch.from_numpy(absorbing[i]), is_expert)      # iq_update, iq_sac.py:411-412
            ag._update_all_targets()                                              # :418-419
            ag._iter += 1                                                         # fit, :405
    finally:
        Normal.rsample = rsample0
    n = len(PASSES)
    assert len(eps_log) == len(pass_log) == n * N_ITER
    eps = {k: np.stack([eps_log[n * i + PASSES.index(k)] for i in range(N_ITER)]) for k in PASSES}
    passes = {k: [pass_log[n * i + PASSES.index(k)] for i in range(N_ITER)] for k in PASSES}
    n_e = B - N_POLICY
    assert eps["pi"].shape == (N_ITER, B, ACT_DIM) and eps["expert"].shape == eps["v0"].shape == (N_ITER, n_e, ACT_DIM)

    tags = _abi_tags.IQ_Q_TAGS
    scal = np.full((N_ITER, 16), np.nan)
    extra = np.full((N_ITER, len(ACTION_TAGS)), np.nan)
    for i in range(N_ITER):
        row = ag._sw.rows[i + 1]
        for k, t in enumerate(tags):
            if t in row:
                scal[i, k] = row[t]
        for k, t in enumerate(ACTION_TAGS):
            extra[i, k] = row[t]
    c_fin, t_fin = G.params_of(cnet), G.params_of(tnet)

    # ---- the float64 twin and the wrong readings (tests/iq_v0_restate.py)
    import iq_v0_restate as V
    cfg = twin_cfg(spec, alpha)
    steps = [dict(obs=obs[i], act=act[i], next_obs=nxt[i], absorbing=absorbing[i], a_next=passes["next"][i][0],
                  logp_next=passes["next"][i][1], a_pi=passes["pi"][i][0], logp_pi=passes["pi"][i][1],
                  a_v0=passes["v0"][i][0], logp_v0=passes["v0"][i][1]) for i in range(N_ITER)]
    init = [c_init[k] for k in NAMES]
    twin, twin_out, margins = V.run(init, cfg, steps, N_POLICY, check=True)
    if spec["clip"]:
        for m in margins:
            print(f"{name}: next_v below / inside / above the range {m['below']} / {m['inside']} / {m['above']} (nearest to "
                  f"a bound {m['clip_margin']:.2e})")
    # the distances hold at every update; rows of every kind occur in the run (without a target the fit of Q[expert] to
    # Q_max pulls every next_v down together: by the fourth update none is left above the range)
    V.L.assert_margins(margins, name, counts=False)
    if spec["clip"]:
        assert min(sum(m[k] for m in margins) for k in ("below", "inside", "above")) >= 2 * (N_ITER - 1), name
    catp = lambda ps: np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in ps])
    flat = lambda d: catp([d[k] for k in NAMES])
    sp_par = float(np.abs(flat(c_fin) - catp(twin["params"])).max())
    sp_tgt = float(np.abs(flat(t_fin) - catp(twin["target"])).max())
    logged = ~np.isnan(scal)
    sp_scal = float(np.abs(scal - twin_out)[logged].max())
    cs, tcs = G.stats_of(cnet._stand, D), G.stats_of(tnet._stand, D)
    sp_stat = max(float(np.abs(cs - twin["colstats"]).max()), float(np.abs(tcs - twin["tcolstats"]).max()))
    print(f"{name}: spreads params {sp_par:.3e} target {sp_tgt:.3e} scalars {sp_scal:.3e} statistics {sp_stat:.3e}")
    assert np.array_equal(cs[0], twin["colstats"][0]) and np.array_equal(tcs[0], twin["tcolstats"][0])
    assert sp_par <= 1e-5 and sp_tgt <= 1e-5, "the float64 twin does not follow the reference"
    tol_par = max(TOL, 4 * sp_par)
    miss = dict.fromkeys(WRONG, 0.0)
    for wrong in spec["wrong"]:
        w, _ = V.run(init, cfg, steps, N_POLICY, wrong=wrong)
        miss[wrong] = float(np.abs(catp(w["params"]) - catp(twin["params"])).max())
        print(f"{name}: the {wrong} reading misses the parameters by {miss[wrong] / tol_par:.1f} tolerances")
        assert miss[wrong] > tol_par, wrong
    arrays = dict(obs=obs, act=act, next_obs=nxt, absorbing=absorbing, min_a=min_a, max_a=max_a,
                  eps_next=eps["next"], eps_pi=eps["pi"], eps_expert=eps["expert"], eps_v0=eps["v0"], scalars=scal,
                  action_scalars=extra,
                  a_next=np.stack([p[0] for p in passes["next"]]), logp_next=np.stack([p[1] for p in passes["next"]]),
                  a_pi=np.stack([p[0] for p in passes["pi"]]), logp_pi=np.stack([p[1] for p in passes["pi"]]),
                  a_v0=np.stack([p[0] for p in passes["v0"]]), logp_v0=np.stack([p[1] for p in passes["v0"]]),
                  colstats=cs, target_colstats=tcs, policy_colstats=G.stats_of(pnet._stand, IN_DIM),
                  spread_params=np.float64(sp_par), spread_target=np.float64(sp_tgt), spread_scalars=np.float64(sp_scal),
                  spread_stats=np.float64(sp_stat), lr=np.float64(LR), tau=np.float64(TAU),
                  gamma=np.float64(GAMMA), alpha=np.float64(alpha), reg_mult=np.float64(REG_MULT),
                  Q_min=np.float64(Q_MIN), Q_max=np.float64(Q_MAX), n_policy=np.int64(N_POLICY),
                  use_target=np.int64(spec["use_target"]))
    for wrong in WRONG:
        arrays["miss_" + wrong] = np.float64(miss[wrong])
    for k in NAMES:
        if k != "w2":
            arrays[f"policy_init_{k}"] = p_init[k]
            arrays[f"critic_init_{k}"] = c_init[k]
            arrays[f"critic_{k}"] = c_fin[k]
            arrays[f"target_{k}"] = t_fin[k]
    arrays["critic_w2_head"], arrays["target_w2_head"] = c_fin["w2"][:W2_HEAD], t_fin["w2"][:W2_HEAD]
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, name + ".npz")
    fit.write_npz(path, arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")
    return path


# ---- (iii) LSIQ_Offline whole
OFFLINE = dict(exp_mode="fix", exp_loss="MSE", reg="exp", use_target=True)
OFFLINE_WRONG = ("v0_reuses_sample", "v0_no_stats", "v_pass_gradient")
Q_Q_MULTIPLIER, ABS_MULT = 1.0, 1.0       # the attributes the reference reads and never sets: the neutral reading
LR_ACTOR = 3e-4
ACTOR_TAGS = ("Actor/Loss", "Gradients/Norm2 Gradient Q wrt. Pi-parameters", "Actor/Entropy Expert States",
              "Actor/Entropy Policy States", "Actor/Entropy from Gaussian Policy States", "Actor/Entropy Lower Bound",
              "Actor/Entropy from Gaussian Expert States")
OFFLINE_PASSES = ("next", "expert", "pi", "v0", "ppi", "plog")
OFFLINE_ACTION_TAGS = (ACTION_TAGS[0], ACTION_TAGS[1], ACTION_TAGS[4])


def offline_cfgs(alpha, lr=LR, tau=TAU, gamma=GAMMA):
    import iq_pi_restate as P
    import iq_v0_restate as V
    qcfg = V.offline_cfg(exp_mode=OFFLINE["exp_mode"], exp_loss=OFFLINE["exp_loss"], reg=OFFLINE["reg"],
                         use_target=OFFLINE["use_target"], q_min=Q_MIN, q_max=Q_MAX, standardizer=True, gamma=gamma, alpha=alpha,
                         reg_mult=REG_MULT, lr=lr, tau=tau)
    cfg = P.PiCfg(standardizer=True, lr=LR_ACTOR, own_states=False, learnable=False, init_alpha=INIT_ALPHA,
                  ls_min=G.LOG_STD_MIN, ls_max=G.LOG_STD_MAX)
    return cfg, qcfg


def run_offline(name, out_dir):
    """LSIQ_Offline (imitation_lib/imitation/offline/lsiq_offline.py:9-210): fit_offline's loop body (iq_update on a batch
    of B expert rows, then _iter += 1 and policy.iter += 1; the minibatch draw itself is mushroom-rl's) with its own _lossQ,
    logging_loss, iq_update and update_policy.  The three attributes the class reads and nothing sets are set by hand:
    _Q_Q_multiplier = _abs_mult = 1.0 and _act_mask = arange(A), and stored in the file."""
    import importlib
    import torch
    from copy import deepcopy
    to_parameter = G.install_stubs()
    nw = importlib.import_module("imitation_lib.utils.networks")
    iq = importlib.import_module("imitation_lib.imitation.iq_sac")
    off = importlib.import_module("imitation_lib.imitation.offline.lsiq_offline")
    import _abi_tags
    obs, act, nxt, absorbing, min_a, max_a = G.inputs()
    torch.manual_seed(5)
    pnet = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(2 * ACT_DIM,), n_features=[512, 256],
                                    activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    cnet = nw.FullyConnectedNetwork(input_shape=(D,), output_shape=(1,), n_features=[512, 256],
                                    activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    with torch.no_grad():
        pnet._linears[1].weight.copy_(torch.from_numpy(w2_init(11)))
        pnet._linears[2].weight.mul_(G.W3_SCALE)
        pnet._linears[2].bias[ACT_DIM:].add_(G.LOG_SIGMA_SHIFT)
        cnet._linears[1].weight.copy_(torch.from_numpy(w2_init(12)))
        cnet._linears[2].weight.mul_(Q_W3_SCALE)
        cnet._linears[2].bias.mul_(Q_W3_SCALE).add_(Q_B3_SHIFT)
    tnet = deepcopy(cnet)
    p_init, c_init = G.params_of(pnet), G.params_of(cnet)
    policy = iq.IQ_Learn_Policy(G.Reg(pnet), min_a, max_a, G.LOG_STD_MIN, G.LOG_STD_MAX)
    ag = off.LSIQ_Offline.__new__(off.LSIQ_Offline)
    ag.mdp_info = types.SimpleNamespace(gamma=GAMMA)
    ag.policy, ag._use_cuda = policy, False
    ag._critic_approximator, ag._target_critic_approximator = G.Reg(cnet), G.Reg(tnet)
    ag._use_target = OFFLINE["use_target"]
    ag._log_alpha = torch.tensor(np.log(INIT_ALPHA), dtype=torch.float32).requires_grad_()
    ag._learnable_alpha = False
    ag._plcy_loss_mode, ag._regularizer_mode = "v0", OFFLINE["reg"]            # lsiq_offline.py:11-19
    ag._gp_lambda, ag._reg_mult = 0.0, REG_MULT
    ag._Q_max, ag._Q_min, ag._loss_mode_exp, ag._Q_exp_loss = Q_MAX, Q_MIN, OFFLINE["exp_mode"], OFFLINE["exp_loss"]
    ag._Q_Q_multiplier, ag._abs_mult, ag._act_mask = Q_Q_MULTIPLIER, ABS_MULT, np.arange(ACT_DIM)
    ag._iter, ag._logging_iter, ag._sw = 1, 1, G.Recorder()
    ag._tau = to_parameter(TAU)
    ag._delay_Q, ag._delay_pi = 1, 1
    ag._train_policy_only_on_own_states = False
    ag._critic_optimizer = torch.optim.Adam(cnet.parameters(), lr=LR)
    actor_optimizer = torch.optim.Adam(pnet.parameters(), lr=LR_ACTOR)

    def _optimize_actor_parameters(loss):
        # RESTATEMENT of mushroom-rl's DeepAC._optimize_actor_parameters (no clipping)
        actor_optimizer.zero_grad()
        loss.backward()
        actor_optimizer.step()
    ag._optimize_actor_parameters = _optimize_actor_parameters
    alpha = float(ag._alpha)

    eps_log, rows_log = [], []
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
    gmls0 = policy.get_mu_log_sigma

    def gmls(state):                                  # the rows of every pass through the policy's network, in order
        rows_log.append(int(state.shape[0]))
        return gmls0(state)
    policy.get_mu_log_sigma = gmls
    Normal.rsample = rsample
    is_expert = torch.ones(B, dtype=torch.bool)       # fit_offline, :42
    torch.manual_seed(41)
    try:
        for i in range(N_ITER):
            ag.iq_update(torch.from_numpy(obs[i]), torch.from_numpy(act[i]), torch.from_numpy(nxt[i]),
                         torch.from_numpy(absorbing[i]), is_expert)               # :45
            ag._iter += 1                                                          # :47-48
            policy.iter += 1
    finally:
        Normal.rsample = rsample0
    n = len(OFFLINE_PASSES)
    assert len(eps_log) == n * N_ITER
    # the eight policy passes of a logging iteration: six draws, then get_mu_log_sigma on no rows and on all
    assert rows_log == [B, B, B, B, B, B, 0, B] * N_ITER, rows_log
    eps = {k: np.stack([eps_log[n * i + OFFLINE_PASSES.index(k)] for i in range(N_ITER)]) for k in OFFLINE_PASSES}
    assert all(v.shape == (N_ITER, B, ACT_DIM) for v in eps.values())

    tags = _abi_tags.IQ_Q_TAGS
    scal = np.full((N_ITER, 16), np.nan)
    ascal = np.full((N_ITER, len(ACTOR_TAGS)), np.nan)
    extra = np.full((N_ITER, len(OFFLINE_ACTION_TAGS)), np.nan)
    for i in range(N_ITER):
        row = ag._sw.rows[i + 1]
        for k, t in enumerate(tags):
            if t in row:
                scal[i, k] = row[t]
        for k, t in enumerate(ACTOR_TAGS):
            ascal[i, k] = row[t]
        for k, t in enumerate(OFFLINE_ACTION_TAGS):
            extra[i, k] = row[t]
    # what the offline logging_loss leaves out, and what it logs as NaN (torch's mean of nothing)
    assert np.isnan(scal[:, (6, 7, 8, 10, 12)]).all() and np.isnan(scal[:, 14]).all() and np.isnan(ascal[:, (3, 4)]).all()
    logged = np.ones(16, bool)
    logged[[6, 7, 8, 10, 12, 14]] = False
    assert not np.isnan(scal[:, logged]).any()
    p_fin, c_fin, t_fin = G.params_of(pnet), G.params_of(cnet), G.params_of(tnet)
    cs, tcs, pcs = G.stats_of(cnet._stand, D), G.stats_of(tnet._stand, D), G.stats_of(pnet._stand, IN_DIM)

    # ---- the float64 twin and the wrong readings (tests/iq_v0_restate.py's OfflineTwin)
    import iq_v0_restate as V
    cfg, qcfg = offline_cfgs(alpha)
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)

    def twin_run(wrong=None):
        t = V.OfflineTwin([p_init[k] for k in NAMES], [c_init[k] for k in NAMES], central, delta, cfg, qcfg, wrong=wrong)
        outs = [t.iq_update(dict(obs=obs[i], act=act[i], next_obs=nxt[i], absorbing=absorbing[i]),
                            {k: v[i] for k, v in eps.items()})[0] for i in range(N_ITER)]
        return t, np.asarray(outs)
    catp = lambda ps: np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in ps])
    flat = lambda d: catp([d[k] for k in NAMES])
    t, t_out = twin_run()
    st = t.state()
    sp_pol = float(np.abs(flat(p_fin) - catp(st["policy"]["params"])).max())
    sp_par = float(np.abs(flat(c_fin) - catp(st["critic"]["params"])).max())
    sp_tgt = float(np.abs(flat(t_fin) - catp(st["critic"]["target"])).max())
    sp_scal = float(np.abs(scal - t_out)[:, logged].max())
    t_ascal = np.array([[t.scalars[i + 1][k] for k in ACTOR_TAGS] for i in range(N_ITER)])
    assert np.array_equal(np.isnan(t_ascal), np.isnan(ascal))
    sp_ascal = float(np.nanmax(np.abs(ascal - t_ascal)))
    sp_stat = max(float(np.abs(cs - st["critic"]["colstats"]).max()), float(np.abs(tcs - st["critic"]["tcolstats"]).max()))
    sp_pstat = float(np.abs(pcs - st["policy"]["colstats"]).max())
    print(f"{name}: spreads policy {sp_pol:.3e} critic {sp_par:.3e} target {sp_tgt:.3e} scalars {sp_scal:.3e} actor scalars "
          f"{sp_ascal:.3e} critic statistics {sp_stat:.3e} policy statistics {sp_pstat:.3e}")
    assert np.array_equal(cs[0], st["critic"]["colstats"][0]) and np.array_equal(tcs[0], st["critic"]["tcolstats"][0])
    assert np.array_equal(pcs[0], st["policy"]["colstats"][0]) and pcs[0, 0] == N_ITER * 7 * B
    assert max(sp_pol, sp_par, sp_tgt) <= 1e-5, "the float64 twin does not follow the reference"
    tol_par = max(TOL, 4 * sp_par)
    miss = {}
    for wrong in OFFLINE_WRONG:
        w = twin_run(wrong)[0].state()
        miss[wrong] = float(np.abs(catp(w["critic"]["params"]) - catp(st["critic"]["params"])).max())
        print(f"{name}: the {wrong} reading misses the critic's parameters by {miss[wrong] / tol_par:.1f} tolerances")
        assert miss[wrong] > tol_par, wrong
    arrays = dict(obs=obs, act=act, next_obs=nxt, absorbing=absorbing, min_a=min_a, max_a=max_a, scalars=scal,
                  actor_scalars=ascal, action_scalars=extra, colstats=cs, target_colstats=tcs, policy_colstats=pcs,
                  spread_policy=np.float64(sp_pol), spread_params=np.float64(sp_par), spread_target=np.float64(sp_tgt),
                  spread_scalars=np.float64(sp_scal), spread_actor_scalars=np.float64(sp_ascal),
                  spread_stats=np.float64(sp_stat), spread_policy_stats=np.float64(sp_pstat), lr=np.float64(LR),
                  lr_actor=np.float64(LR_ACTOR), tau=np.float64(TAU), gamma=np.float64(GAMMA), alpha=np.float64(alpha),
                  reg_mult=np.float64(REG_MULT), Q_min=np.float64(Q_MIN), Q_max=np.float64(Q_MAX),
                  use_target=np.int64(OFFLINE["use_target"]), Q_Q_multiplier=np.float64(Q_Q_MULTIPLIER),
                  abs_mult=np.float64(ABS_MULT), act_mask=np.arange(ACT_DIM, dtype=np.int64))
    for k in OFFLINE_PASSES:
        arrays["eps_" + k] = eps[k]
    for wrong in OFFLINE_WRONG:
        arrays["miss_" + wrong] = np.float64(miss[wrong])
    for k in NAMES:
        if k != "w2":
            arrays[f"policy_init_{k}"] = p_init[k]
            arrays[f"critic_init_{k}"] = c_init[k]
            arrays[f"policy_{k}"] = p_fin[k]
            arrays[f"critic_{k}"] = c_fin[k]
            arrays[f"target_{k}"] = t_fin[k]
    arrays["policy_w2_head"] = p_fin["w2"][:W2_HEAD]
    arrays["critic_w2_head"], arrays["target_w2_head"] = c_fin["w2"][:W2_HEAD], t_fin["w2"][:W2_HEAD]
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, name + ".npz")
    fit.write_npz(path, arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")
    return path


def main():
    # the tags of the 16 scalars live in olympic_hip._abi; imported by path so that the package's library is not needed
    import importlib.util
    import tempfile
    root = os.path.dirname(os.path.dirname(HERE))
    spec = importlib.util.spec_from_file_location("_abi_tags", os.path.join(root, "olympics-mujoco_amd", "olympic_hip",
                                                                            "_abi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules["_abi_tags"] = mod
    for name, s in FIXTURES.items():
        path = run(name, s, OUT_DIR)
        with tempfile.TemporaryDirectory() as again:      # the fixture regenerates byte for byte
            assert open(run(name, s, again), "rb").read() == open(path, "rb").read(), f"{name} does not regenerate"
        assert os.path.getsize(path) < 1 << 20
    path = run_offline("lsiq_offline", OUT_DIR)
    with tempfile.TemporaryDirectory() as again:
        assert open(run_offline("lsiq_offline", again), "rb").read() == open(path, "rb").read(), "lsiq_offline does not regenerate"
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
