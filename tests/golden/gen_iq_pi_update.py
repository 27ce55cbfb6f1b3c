#!/usr/bin/env python3
"""Generate tests/golden/iq_pi_update/{iq,iq_own_states_alpha,sqil}.npz by EXECUTING the reference's own iq_update whole:
IQ_SAC.iq_update, update_Q_function, update_policy, _actor_loss, _update_alpha and _update_all_targets
(imitation_lib/imitation/iq_sac.py:408-465, 587-595, 674-676), SQIL.iq_update (imitation_lib/imitation/sqil_sac.py:16-62)
and IQ_Learn_Policy (iq_sac.py:18-178), imported from the reference tree under gen_iq_q_update.install_stubs(), on
gen_iq_q_update's networks and inputs.  Run in the build container only:

    python tests/golden/gen_iq_pi_update.py [--out DIR]

The setting is gen_iq_q_update's (policy 12 -> [512, 256] -> 10, critic 17 -> [512, 256] -> 1, both with Standardizers,
B = 18, n_policy = 9, a target critic, 4 iterations of whole iq_updates, every one logging, delay_Q = delay_pi = 1, no
warm-up), with Adam(lr = 3e-4) on the actor.  iq: IQ_SAC.  iq_own_states_alpha: IQ_SAC with
train_policy_only_on_own_states (Bp = 9) and learnable_alpha (lr_alpha = 3e-4, target_entropy = -5).  sqil: SQIL with
plcy_loss_mode value.

mushroom-rl is absent.  Beside what gen_iq_q_update restates, DeepAC._optimize_actor_parameters is RESTATED below and
marked, from its published definition without clipping: zero_grad, backward, step on the actor's optimiser.

The noise is recovered by gen_iq_q_update's rsample wrapper (restated here around the same lines): per iteration IQ draws
for next_obs (18 rows), the expert rows (9), obs (18), then update_policy's pass (Bp) and its logging pass (18); SQIL for
next_obs, obs, the expert rows, then the same two.

The float64 twin is tests/iq_pi_restate.py's Twin (torch autograd and Adam over the whole iq_update, the policy's passes
its own).  Stored per tensor group (policy parameters, critic parameters, critic statistics, policy statistics, scalars,
alpha block) the largest |reference float32 - float64 twin|; the alpha block's moments relative to their own size
(iq_pi_restate.alpha_err).  The tests allow max(2e-5, 4 x that spread).  Asserted here: the parameter spreads stay under
1e-5.  Measured at the first setting tried, which was kept: see the printed lines.

Two wrong readings are run through the twin and must miss the true run by more than the tolerance; by how much is
stored: critic_stats_untouched (the policy update leaves the critic's Standardizer alone), on the critic's statistics and
on the policy's parameters after the following iterations; alpha_from_first_pass (_update_alpha takes update_policy's first
log-probabilities on a logging iteration), on the alpha block (0 is stored where alpha is not learnable).

Layer 2's initial weights are gen_iq_q_update.w2_init's seeded draws, rebuilt by the tests; of the stepped layer-2 weights
the first 16 rows are stored.  The archives have fixed member dates (gen_bc_fit.write_npz): running the generator again
reproduces the files byte for byte.  The fixtures hold data only.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "iq_pi_update")
if __name__ == "__main__" and "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_bc_fit as fit  # noqa: E402  (write_npz)
import gen_iq_q_update as gq  # noqa: E402

IN_DIM, ACT_DIM, B, N_POLICY, N_ITER, D = gq.IN_DIM, gq.ACT_DIM, gq.B, gq.N_POLICY, gq.N_ITER, gq.D
LR_ACTOR, LR_ALPHA = 3e-4, 3e-4
NAMES, TOL, W2_HEAD = gq.NAMES, gq.TOL, gq.W2_HEAD
FIXTURES = dict(iq=dict(algo="iq", mode="value", reg="exp_and_plcy", use_target=True, own_states=False, learnable=False),
                iq_own_states_alpha=dict(algo="iq", mode="value", reg="exp_and_plcy", use_target=True, own_states=True,
                                         learnable=True),
                sqil=dict(algo="sqil", mode="value", reg="exp_and_plcy", use_target=True, own_states=False, learnable=False))
ACTOR_TAGS = ("Actor/Loss", "Gradients/Norm2 Gradient Q wrt. Pi-parameters", "Actor/Entropy Expert States",
              "Actor/Entropy Policy States", "Actor/Entropy from Gaussian Policy States", "Actor/Entropy Lower Bound",
              "Actor/Entropy from Gaussian Expert States")


def run(name, spec):
    import importlib
    import torch
    from copy import deepcopy
    to_parameter = gq.install_stubs()
    nw = importlib.import_module("imitation_lib.utils.networks")
    iq = importlib.import_module("imitation_lib.imitation.iq_sac")
    sq = importlib.import_module("imitation_lib.imitation.sqil_sac")
    obs, act, nxt, absorbing, min_a, max_a = gq.inputs()
    torch.manual_seed(5)
    pnet = nw.FullyConnectedNetwork(input_shape=(IN_DIM,), output_shape=(2 * ACT_DIM,), n_features=[512, 256],
                                    activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    cnet = nw.FullyConnectedNetwork(input_shape=(D,), output_shape=(1,), n_features=[512, 256],
                                    activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    with torch.no_grad():
        pnet._linears[1].weight.copy_(torch.from_numpy(gq.w2_init(11)))
        pnet._linears[2].weight.mul_(gq.W3_SCALE)
        pnet._linears[2].bias[ACT_DIM:].add_(gq.LOG_SIGMA_SHIFT)
        cnet._linears[1].weight.copy_(torch.from_numpy(gq.w2_init(12)))
    tnet = deepcopy(cnet)
    p_init, c_init = gq.params_of(pnet), gq.params_of(cnet)
    policy = iq.IQ_Learn_Policy(gq.Reg(pnet), min_a, max_a, gq.LOG_STD_MIN, gq.LOG_STD_MAX)
    cls = iq.IQ_SAC if spec["algo"] == "iq" else sq.SQIL
    ag = cls.__new__(cls)
    ag.mdp_info = types.SimpleNamespace(gamma=gq.GAMMA)
    ag.policy, ag._use_cuda = policy, False
    ag._critic_approximator, ag._target_critic_approximator = gq.Reg(cnet), gq.Reg(tnet)
    ag._use_target = spec["use_target"]
    ag._log_alpha = torch.tensor(np.log(gq.INIT_ALPHA), dtype=torch.float32).requires_grad_()      # iq_sac.py:328-333
    ag._alpha_optim = torch.optim.Adam([ag._log_alpha], lr=LR_ALPHA)                             # :335
    ag._learnable_alpha = spec["learnable"]
    ag._target_entropy = -np.prod((ACT_DIM,)).astype(np.float32)                                 # :281-282
    ag._plcy_loss_mode, ag._regularizer_mode = spec["mode"], spec["reg"]
    ag._gp_lambda, ag._reg_mult, ag._treat_absorbing_states = 0.0, gq.REG_MULT, False
    ag._R_min, ag._R_max = 0.0, 1.0
    ag._iter, ag._logging_iter, ag._sw = 1, 1, gq.Recorder()
    ag._tau = to_parameter(gq.TAU)
    ag._delay_Q, ag._delay_pi = 1, 1
    ag._warmup_transitions = to_parameter(0)
    ag._replay_memory = types.SimpleNamespace(size=100)
    ag._train_policy_only_on_own_states = spec["own_states"]
    ag._critic_optimizer = torch.optim.Adam(cnet.parameters(), lr=gq.LR)
    actor_optimizer = torch.optim.Adam(pnet.parameters(), lr=LR_ACTOR)

    def _optimize_actor_parameters(loss):
        # RESTATEMENT of mushroom-rl's DeepAC._optimize_actor_parameters (no clipping)
        actor_optimizer.zero_grad()
        loss.backward()
        actor_optimizer.step()
    ag._optimize_actor_parameters = _optimize_actor_parameters

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
    Normal.rsample = rsample
    is_expert = torch.cat([torch.zeros(N_POLICY, dtype=torch.bool), torch.ones(B - N_POLICY, dtype=torch.bool)])
    torch.manual_seed(41)
    try:
        for i in range(N_ITER):
            ag.iq_update(torch.from_numpy(obs[i]), torch.from_numpy(act[i]), torch.from_numpy(nxt[i]),
                         torch.from_numpy(absorbing[i]), is_expert)
            ag._iter += 1                             # fit, :405-406
            policy.iter += 1
    finally:
        Normal.rsample = rsample0
    assert len(eps_log) == 5 * N_ITER
    order = (("next", "expert", "pi") if spec["algo"] == "iq" else ("next", "pi", "expert")) + ("ppi", "plog")
    eps = {k: np.stack([eps_log[5 * i + order.index(k)] for i in range(N_ITER)]) for k in order}
    Bp = N_POLICY if spec["own_states"] else B
    assert eps["ppi"].shape == (N_ITER, Bp, ACT_DIM) and eps["plog"].shape == (N_ITER, B, ACT_DIM)

    scal = np.full((N_ITER, len(ACTOR_TAGS)), np.nan)
    for i in range(N_ITER):
        row = ag._sw.rows[i + 1]
        for k, t in enumerate(ACTOR_TAGS):
            scal[i, k] = row[t]
    p_fin, c_fin = gq.params_of(pnet), gq.params_of(cnet)
    ast = ag._alpha_optim.state.get(ag._log_alpha, {})
    ablock = np.array([float(ag._log_alpha.detach()), float(ast.get("exp_avg", 0.0)), float(ast.get("exp_avg_sq", 0.0))])
    cs, pcs = gq.stats_of(cnet._stand, D), gq.stats_of(pnet._stand, IN_DIM)

    # ---- the float64 twin and the wrong readings (tests/iq_pi_restate.py)
    import iq_pi_restate as R
    import iq_restate as Q
    qcfg = Q.Cfg(algo=spec["algo"], mode=spec["mode"], reg=spec["reg"], treat=False, use_target=spec["use_target"],
                 standardizer=True, gamma=gq.GAMMA, reg_mult=gq.REG_MULT, R_min=0.0, R_max=1.0, lr=gq.LR, tau=gq.TAU)
    cfg = R.PiCfg(standardizer=True, lr=LR_ACTOR, own_states=spec["own_states"], learnable=spec["learnable"],
                  lr_alpha=LR_ALPHA, init_alpha=gq.INIT_ALPHA, ls_min=gq.LOG_STD_MIN, ls_max=gq.LOG_STD_MAX)
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)

    def twin_run(wrong=None):
        t = R.Twin([p_init[n] for n in NAMES], [c_init[n] for n in NAMES], central, delta, cfg, qcfg=qcfg, wrong=wrong)
        for i in range(N_ITER):
            t.iq_update(dict(obs=obs[i], act=act[i], next_obs=nxt[i], absorbing=absorbing[i]), N_POLICY,
                        {k: v[i] for k, v in eps.items()})
        return t
    flat = lambda d: np.concatenate([np.asarray(d[n], np.float64).reshape(-1) for n in NAMES])
    t = twin_run()
    st = t.state()
    sp_par = float(np.abs(flat(p_fin) - R.cat(st["policy"]["params"])).max())
    sp_cpar = float(np.abs(flat(c_fin) - R.cat(st["critic"]["params"])).max())
    sp_cstat = float(np.abs(cs - st["critic"]["colstats"]).max())
    sp_pstat = float(np.abs(pcs - st["policy"]["colstats"]).max())
    tscal = np.array([[t.scalars[i + 1][k] for k in ACTOR_TAGS] for i in range(N_ITER)])
    sp_scal = float(np.abs(scal - tscal).max())
    sp_alpha = R.alpha_err(ablock, st["alpha"])
    print(f"{name}: spreads policy {sp_par:.3e} critic {sp_cpar:.3e} critic statistics {sp_cstat:.3e} policy statistics "
          f"{sp_pstat:.3e} scalars {sp_scal:.3e} alpha block {sp_alpha:.3e}")
    assert np.array_equal(cs[0], st["critic"]["colstats"][0]) and np.array_equal(pcs[0], st["policy"]["colstats"][0])
    assert sp_par <= 1e-5 and sp_cpar <= 1e-5, "the float64 twin does not follow the reference"
    tol_par, tol_stat, tol_alpha = max(TOL, 4 * sp_par), max(TOL, 4 * sp_cstat), max(TOL, 4 * sp_alpha)
    w = twin_run("critic_stats_untouched").state()
    miss_stats = float(np.abs(w["critic"]["colstats"] - st["critic"]["colstats"]).max())
    miss_par = float(np.abs(R.cat(w["policy"]["params"]) - R.cat(st["policy"]["params"])).max())
    print(f"{name}: critic_stats_untouched misses the critic's statistics by {miss_stats / tol_stat:.1f} tolerances, the "
          f"policy's parameters by {miss_par / tol_par:.1f}")
    assert miss_stats > tol_stat and miss_par > tol_par
    miss_alpha = 0.0
    if spec["learnable"]:
        miss_alpha = R.alpha_err(twin_run("alpha_from_first_pass").state()["alpha"], st["alpha"])
        print(f"{name}: alpha_from_first_pass misses the alpha block by {miss_alpha / tol_alpha:.1f} tolerances")
        assert miss_alpha > tol_alpha
    arrays = dict(obs=obs, act=act, next_obs=nxt, absorbing=absorbing, min_a=min_a, max_a=max_a,
                  eps_next=eps["next"], eps_pi=eps["pi"], eps_expert=eps["expert"], eps_ppi=eps["ppi"],
                  eps_plog=eps["plog"], scalars=scal, colstats=cs, policy_colstats=pcs, alpha_block=ablock,
                  spread_policy=np.float64(sp_par), spread_critic=np.float64(sp_cpar),
                  spread_critic_stats=np.float64(sp_cstat), spread_policy_stats=np.float64(sp_pstat),
                  spread_scalars=np.float64(sp_scal), spread_alpha=np.float64(sp_alpha),
                  miss_critic_stats_untouched_stats=np.float64(miss_stats),
                  miss_critic_stats_untouched_params=np.float64(miss_par),
                  miss_alpha_from_first_pass=np.float64(miss_alpha), lr=np.float64(gq.LR), lr_actor=np.float64(LR_ACTOR),
                  lr_alpha=np.float64(LR_ALPHA), tau=np.float64(gq.TAU), gamma=np.float64(gq.GAMMA),
                  reg_mult=np.float64(gq.REG_MULT), n_policy=np.int64(N_POLICY),
                  target_entropy=np.float64(ag._target_entropy))
    for n in NAMES:
        if n != "w2":
            arrays[f"policy_init_{n}"] = p_init[n]
            arrays[f"critic_init_{n}"] = c_init[n]
            arrays[f"policy_{n}"] = p_fin[n]
            arrays[f"critic_{n}"] = c_fin[n]
    arrays["policy_w2_head"], arrays["critic_w2_head"] = p_fin["w2"][:W2_HEAD], c_fin["w2"][:W2_HEAD]
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    fit.write_npz(path, arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) <= 224 * 1024


def main():
    for name, s in FIXTURES.items():
        run(name, s)


if __name__ == "__main__":
    main()
