#!/usr/bin/env python3
"""Generate tests/golden/lsiq_q_update/*.npz by EXECUTING the reference's own LSIQ critic update: LSIQ._lossQ,
_lossQ_iq_like and _lossQ_sqil_like (imitation_lib/imitation/lsiq.py:9-195) with everything they inherit from IQ_SAC
(update_Q_function, getV, get_targetV, regularizer_loss, update_Q_parameters, logging_loss, _update_all_targets,
imitation_lib/imitation/iq_sac.py) and IQ_Learn_Policy, imported from the reference tree under the stubs and
restatements of gen_iq_q_update.py (install_stubs, Reg, Recorder), on the reference's FullyConnectedNetwork and
Standardizer.  Run in the build container only:

    python tests/golden/gen_lsiq_q_update.py [--out DIR]

The setting is gen_iq_q_update.py's: policy 12 -> [512, 256] -> 10, critic 17 -> [512, 256] -> 1, both with Standardizers,
B = 18 rows of which the first n_policy = 9 are the policy's, the same inputs, 4 iterations, every one logging, tau =
0.005, gamma = 0.99, alpha = exp(float32(log 1e-3)).  What differs, and why: this critic's next_v spans -0.74 .. 0.21
with a median near -0.25 on these inputs, so with the reference's default bounds +-1 no row would ever clip.  Its output
layer is scaled by 2 and its output bias raised by 0.5 (next_v then spans about -1 .. 0.9 around 0) and the bounds are
Q_min = -0.25, Q_max = 0.3; scale and shift are the first pair of a short grid (scale 2, 3, 1; shift 0.3 .. 0.8) at which
all four fixtures hold the margins below at all four updates.  Adam's lr is 3e-5, because at 3e-4 every Q moves by several
tenths per update (all weights step downhill together) and the rows leave the clip range after the first update.  The
sqil_like fixtures take reg_mult 2 (rewards -+0.5, and 100 times that on absorbing rows), so that Huber's residuals lie on
both of its branches.

The four fixtures, each with the wrong reading (tests/lsiq_restate.py) it must tell from the reference:
  iq_fix          iq_like, fix / MSE, clipping, value, exp_and_plcy, a target            unclipped_target
  iq_bootstrap    iq_like, bootstrap, clipping, no target, value_q_old_policy, exp        clip_grad_through
  sqil_value_plcy sqil_like, bootstrap / Huber, value_plcy, treat_absorbing_states, a target   stats_all_rows
  sqil_fix_value  sqil_like, fix / MSE, value, treat_absorbing_states, no target          fix_grad_to_y, absorbing_rmin

The agent is built with __new__ and given the attributes the methods read; per iteration update_Q_function, then
_update_all_targets, then _iter += 1 (iq_update's and fit's lines).  The policy's noise is recorded as
gen_iq_q_update.py records it; per iteration iq_like draws for next_obs (18 rows), the expert rows (9) and obs (18),
sqil_like for next_obs, obs (value: 18 rows, value_plcy: the 9 policy rows) and then the expert rows.

The float64 twin is tests/lsiq_restate.py on the actions and log-probabilities the reference run produced.  Stored per
tensor group (parameters, target, scalars, statistics): the largest |reference float32 - float64 twin|; the tests allow
4 x that and never less than 2e-5.  Asserted here: the parameter spread stays under 1e-5; the twin's margins
(lsiq_restate.assert_margins: no next_v within 1e-3 of a bound, no Huber residual within 1e-3 of 1, no pre-activation
within 1e-6 of 0, two rows of every kind) hold at every update; each wrong reading misses the true run's parameters by more than the tolerance (by how much
is stored).  The fixtures hold data only and regenerate byte for byte."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "lsiq_q_update")
if __name__ == "__main__" and "--out" in sys.argv:
    _i = sys.argv.index("--out")
    OUT_DIR = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_bc_fit as fit  # noqa: E402  (write_npz)
import gen_iq_q_update as G  # noqa: E402

IN_DIM, ACT_DIM, B, N_POLICY, N_ITER, D = G.IN_DIM, G.ACT_DIM, G.B, G.N_POLICY, G.N_ITER, G.D
LR, TAU, GAMMA, INIT_ALPHA = 3e-5, G.TAU, G.GAMMA, G.INIT_ALPHA
Q_W3_SCALE, Q_B3_SHIFT, Q_MIN, Q_MAX = 2.0, 0.5, -0.25, 0.3
NAMES, TOL, W2_HEAD, ACTION_TAGS, w2_init = G.NAMES, G.TOL, G.W2_HEAD, G.ACTION_TAGS, G.w2_init
FIXTURES = dict(
    iq_fix=dict(type="iq_like", exp_mode="fix", exp_loss="MSE", clip=True, mode="value", reg="exp_and_plcy", treat=False,
                use_target=True, reg_mult=0.5, wrong=("unclipped_target",)),
    iq_bootstrap=dict(type="iq_like", exp_mode="bootstrap", exp_loss=None, clip=True, mode="value_q_old_policy", reg="exp",
                      treat=False, use_target=False, reg_mult=0.5, wrong=("clip_grad_through",)),
    sqil_value_plcy=dict(type="sqil_like", exp_mode="bootstrap", exp_loss="Huber", clip=True, mode="value_plcy",
                         reg="exp_and_plcy", treat=True, use_target=True, reg_mult=2.0, wrong=("stats_all_rows",)),
    sqil_fix_value=dict(type="sqil_like", exp_mode="fix", exp_loss="MSE", clip=True, mode="value", reg="exp_and_plcy",
                        treat=True, use_target=False, reg_mult=2.0, wrong=("fix_grad_to_y", "absorbing_rmin")))
WRONG = ("unclipped_target", "clip_grad_through", "stats_all_rows", "fix_grad_to_y", "absorbing_rmin")


def twin_cfg(spec, alpha, lr=LR, tau=TAU, gamma=GAMMA):
    import lsiq_restate as L
    return L.LCfg(type=spec["type"], exp_mode=spec["exp_mode"], exp_loss=spec["exp_loss"], clip=spec["clip"], q_min=Q_MIN,
                  q_max=Q_MAX, mode=spec["mode"], reg=spec["reg"], treat=spec["treat"], use_target=spec["use_target"],
                  standardizer=True, gamma=gamma, alpha=alpha, reg_mult=spec["reg_mult"], lr=lr, tau=tau)


def run(name, spec):
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
    ag = ls.LSIQ.__new__(ls.LSIQ)
    ag.mdp_info = types.SimpleNamespace(gamma=GAMMA)
    ag.policy, ag._use_cuda = policy, False
    ag._critic_approximator, ag._target_critic_approximator = G.Reg(cnet), G.Reg(tnet)
    ag._use_target = spec["use_target"]
    ag._log_alpha = torch.tensor(np.log(INIT_ALPHA), dtype=torch.float32)
    ag._plcy_loss_mode, ag._regularizer_mode = spec["mode"], spec["reg"]
    ag._gp_lambda, ag._reg_mult, ag._treat_absorbing_states = 0.0, spec["reg_mult"], spec["treat"]
    ag._Q_max, ag._Q_min, ag._loss_mode_exp, ag._Q_exp_loss = Q_MAX, Q_MIN, spec["exp_mode"], spec["exp_loss"]
    ag._target_clipping, ag._lossQ_type = spec["clip"], spec["type"]
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
    assert len(eps_log) == len(pass_log) == 3 * N_ITER
    order = ("next", "expert", "pi") if spec["type"] == "iq_like" else ("next", "pi", "expert")
    eps = {k: np.stack([eps_log[3 * i + order.index(k)] for i in range(N_ITER)]) for k in order}
    passes = {k: [pass_log[3 * i + order.index(k)] for i in range(N_ITER)] for k in order}
    n_pi = N_POLICY if spec["mode"] == "value_plcy" else B
    assert eps["pi"].shape == (N_ITER, n_pi, ACT_DIM) and eps["expert"].shape == (N_ITER, B - N_POLICY, ACT_DIM)

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

    # ---- the float64 twin and the wrong readings (tests/lsiq_restate.py)
    import lsiq_restate as L
    cfg = twin_cfg(spec, alpha)
    steps = [dict(obs=obs[i], act=act[i], next_obs=nxt[i], absorbing=absorbing[i], a_next=passes["next"][i][0],
                  logp_next=passes["next"][i][1], a_pi=passes["pi"][i][0], logp_pi=passes["pi"][i][1])
             for i in range(N_ITER)]
    init = [c_init[n] for n in NAMES]
    twin, twin_out, margins = L.run(init, cfg, steps, N_POLICY, check=True)
    for m in margins:
        print(f"{name}: next_v below / inside / above the range {m['below']} / {m['inside']} / {m['above']} (nearest to a "
              f"bound {m['clip_margin']:.2e}); Huber quadratic / linear {m['quadratic']} / {m['linear']} (nearest to 1 "
              f"{m['huber_margin']:.2e})")
    L.assert_margins(margins, name)
    catp = lambda ps: np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in ps])
    flat = lambda d: catp([d[n] for n in NAMES])
    sp_par = float(np.abs(flat(c_fin) - catp(twin["params"])).max())
    sp_tgt = float(np.abs(flat(t_fin) - catp(twin["target"])).max())
    logged = ~np.isnan(scal)
    sp_scal = float(np.abs(scal - twin_out)[logged].max())
    cs, tcs = G.stats_of(cnet._stand, D), G.stats_of(tnet._stand, D)
    sp_stat = max(float(np.abs(cs - twin["colstats"]).max()), float(np.abs(tcs - twin["tcolstats"]).max()))
    print(f"{name}: spreads params {sp_par:.3e} target {sp_tgt:.3e} scalars {sp_scal:.3e} statistics {sp_stat:.3e}")
    assert sp_par <= 1e-5 and sp_tgt <= 1e-5, "the float64 twin does not follow the reference"
    tol_par = max(TOL, 4 * sp_par)
    miss = dict.fromkeys(WRONG, 0.0)
    for wrong in spec["wrong"]:
        w, _ = L.run(init, cfg, steps, N_POLICY, wrong=wrong)
        miss[wrong] = float(np.abs(catp(w["params"]) - catp(twin["params"])).max())
        print(f"{name}: the {wrong} reading misses the parameters by {miss[wrong] / tol_par:.1f} tolerances")
        assert miss[wrong] > tol_par, wrong
    arrays = dict(obs=obs, act=act, next_obs=nxt, absorbing=absorbing, min_a=min_a, max_a=max_a,
                  eps_next=eps["next"], eps_pi=eps["pi"], eps_expert=eps["expert"], scalars=scal, action_scalars=extra,
                  a_next=np.stack([p[0] for p in passes["next"]]), logp_next=np.stack([p[1] for p in passes["next"]]),
                  a_pi=np.stack([p[0] for p in passes["pi"]]), logp_pi=np.stack([p[1] for p in passes["pi"]]),
                  colstats=cs, target_colstats=tcs, policy_colstats=G.stats_of(pnet._stand, IN_DIM),
                  spread_params=np.float64(sp_par), spread_target=np.float64(sp_tgt), spread_scalars=np.float64(sp_scal),
                  spread_stats=np.float64(sp_stat), lr=np.float64(LR), tau=np.float64(TAU),
                  gamma=np.float64(GAMMA), alpha=np.float64(alpha), reg_mult=np.float64(spec["reg_mult"]),
                  Q_min=np.float64(Q_MIN), Q_max=np.float64(Q_MAX), n_policy=np.int64(N_POLICY),
                  use_target=np.int64(spec["use_target"]))
    for wrong in WRONG:
        arrays["miss_" + wrong] = np.float64(miss[wrong])
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
