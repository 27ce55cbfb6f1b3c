#!/usr/bin/env python3
"""Generate tests/golden/lsiq_h_update/*.npz by EXECUTING the reference's own LSIQ_H and LSIQ_HC
(imitation_lib/imitation/lsiq_h.py, lsiq_hc.py) for whole iq_updates: _lossQ_iq_like with update_H_function inside it,
getV / get_targetV without the entropy, update_policy with the two-critic _actor_loss, _update_all_targets and
_update_target_H, with everything they inherit from
LSIQ and IQ_SAC and IQ_Learn_Policy, imported from the reference tree under the stubs and restatements of
gen_iq_q_update.py (install_stubs, Reg, Recorder), on the reference's FullyConnectedNetwork and Standardizer.  Run in the
build container only:

    python tests/golden/gen_lsiq_h_update.py [--out DIR]

The setting is gen_lsiq_q_update.py's: policy 12 -> [512, 256] -> 10, Q critic and H critic 17 -> [512, 256] -> 1, all with
Standardizers, B = 18 rows of which the first n_policy = 9 are the policy's, the same inputs (absorbing rows 1, 6 among
the policy's and 11, 16 among the expert's, and one more drawn per iteration), 4 iterations, every one logging, gamma =
0.99, the Q critic scaled and bounded as there (Q_min = -0.25, Q_max = 0.3, lr 3e-5).  What differs, and why:
  * alpha = exp(float32(log 0.2)) and the running maximum's rates 0.3 (up) and 0.1 (down), for the reasons
    tests/lsiq_h_restate.py gives for its sweep: at alpha = 1e-3 the entropy moves no target by more than a tolerance, and
    at the default rates a maximum read before its update cannot be told from the updated one.  The Q critic's values
    carry no entropy here (getV / get_targetV), so alpha does not reach it.
  * H's output layer is scaled by 10 (its initial weights drawn after the other two networks', layer 2 from
    w2_init(H_W2_SEED)), so that LSIQ_HC's Huber residuals lie on both branches; H's lr is 6e-5, its own.  H_W2_SEED = 18 is
    the first seed from 13 upwards at which all three fixtures hold every margin at all four updates and every wrong
    reading misses by more than three tolerances (at the others a relu pre-activation, a clip or a Huber residual of one
    fixture lies within its margin).
  * LSIQ_HC takes reg_mult 2: the squared reward's clip is then +-0.5 and Q_target - y reaches it.  Its Q critic's tau
    is 0.5, not 0.005: measured with 0.005, the target moves so little per update that reading it after its soft update
    changed the H loss by 1.3 tolerances; the parameters then differed by up to 2 lr in single entries of layer 2 whose
    gradient nearly cancels (Adam steps by the sign), which is why a miss is measured on the stored parameters and the
    scalars, whichever is larger, and the scalars carry it.

The fixtures, each with the wrong readings (tests/lsiq_h_restate.py) it must tell from the reference:
  h_iq         LSIQ_H, iq_like fix / MSE, a target, the expert clip            row_wise, clip_old_max, h_step_clipped
  hc_huber     LSIQ_HC, Huber, a target, tau 0.5, H_tau 0.2                          row_wise, target_after
  hc_mse       LSIQ_HC, MSE, the Q critic WITHOUT a target, tau 0.5, H_tau 0.2         row_wise, target_after

The agent is built with __new__ and given the attributes the methods read; per iteration iq_update (update_Q_function,
update_policy, _update_all_targets; the actor's lr is 3e-4, _optimize_actor_parameters is RESTATED as in
gen_iq_pi_update.py), then _iter += 1 and policy.iter += 1 (fit's lines).  After the passes below come update_policy's
two: the training pass (18 rows) and, logging, the second pass (18).  Every reading of WRONG is measured on every fixture;
the readings of the policy's side (h_before_q, no_h: the actor loss without H) with a twin that runs the policy itself on
the recorded noise (tests/lsiq_h_restate.py's whole_twin), which must first follow the reference run, the policy's
parameters included.  To keep a fixture near the size of the others, of each final network the first W1_HEAD rows of
layer 1 and the first W2_HEAD rows of layer 2 are stored.  update_H_function's `absorbing` is whatever
_lossQ_iq_like hands it: nothing here reshapes it, so the [B] against [B, 1] broadcast is the reference's own.  The
policy's noise and outputs are recorded pass by pass: next_obs (18 rows), the expert rows (9), obs (18), then
update_H_function's next_obs (18) and, for LSIQ_HC, get_targetV's obs (18).

The float64 twin is tests/lsiq_h_restate.py's whole_twin, which runs the policy itself on the recorded noise.
Stored per tensor group (both critics' parameters and targets, the H scalars, the running maximum): the largest
|reference float32 - float64 twin|; the tests allow 4 x that and never less than 2e-5.  Asserted here: the parameter
spreads stay under 1e-5; the twin's margins hold at every update (distances; the counts of expert rows on either side of
the maximum are printed, not asserted: the log-probabilities are the reference policy's own); each wrong reading misses
the reference run by more than the tolerance (by how much is stored); "H updated before Q's step" (h_before_q) is
measured on every fixture with a twin that runs the policy itself on the recorded noise, because only the order of the
policy's passes, each of which feeds its Standardizer, carries it.  The actor loss without H is not a reading of this
update: tests/test_lsiq_h_cpu.py holds it on the actor step's own cases.  The fixtures hold data only and regenerate byte
for byte."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "lsiq_h_update")
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
LR, H_LR, TAU, H_TAU, GAMMA, INIT_ALPHA = GL.LR, 6e-5, G.TAU, 0.2, G.GAMMA, 0.2
TAU_UP, TAU_DOWN, H_W3_SCALE, H_W2_SEED, Q_MIN, Q_MAX = 0.3, 0.1, 10.0, 18, GL.Q_MIN, GL.Q_MAX
NAMES, TOL, w2_init = G.NAMES, G.TOL, G.w2_init
W1_HEAD, W2_HEAD, LR_ACTOR = 64, 4, 3e-4
H_TAGS = ("H function/Loss", "H function/H", "H function/H plcy", "H function/H expert", "H function/H_step",
          "H function/H_step plcy", "H function/H_step expert")
FIXTURES = dict(
    h_iq=dict(cost=False, loss="MSE", use_target=True, reg_mult=0.5, tau=TAU,
              wrong=("row_wise", "clip_old_max", "h_step_clipped")),
    hc_huber=dict(cost=True, loss="Huber", use_target=True, reg_mult=2.0, tau=0.5,
                  wrong=("row_wise", "clip_old_max", "h_step_clipped", "target_after")),
    hc_mse=dict(cost=True, loss="MSE", use_target=False, reg_mult=2.0, tau=0.5,
                wrong=("row_wise", "clip_old_max", "h_step_clipped", "target_after")))
WRONG = ("row_wise", "clip_old_max", "h_step_clipped", "target_after", "h_before_q", "no_h")
PASSES = ("next", "expert", "pi", "h_next", "h_pi")      # update_Q_function's
PI_PASSES = ("ppi", "plog")                              # update_policy's


def twin_cfgs(spec, alpha):
    import lsiq_h_restate as H
    import lsiq_restate as L
    lcfg = L.LCfg(type="iq_like", exp_mode="fix", exp_loss="MSE", clip=True, q_min=Q_MIN, q_max=Q_MAX, mode="value",
                  reg="exp_and_plcy", treat=False, use_target=spec["use_target"], standardizer=True, gamma=GAMMA, alpha=0.0,
                  reg_mult=spec["reg_mult"], lr=LR, tau=spec["tau"])
    hcfg = H.HCfg(cost=spec["cost"], loss=spec["loss"], clip_expert=True, tau_up=TAU_UP, tau_down=TAU_DOWN, q_min=Q_MIN,
                  q_max=Q_MAX, standardizer=True, gamma=GAMMA, alpha=alpha, reg_mult=spec["reg_mult"], lr=H_LR,
                  tau=H_TAU if spec["cost"] else TAU)
    return lcfg, hcfg


class RegList(G.Reg):
    """G.Reg as LSIQ_HC._update_target_H indexes it: a Regressor of one model."""

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self


def run(name, spec):
    import importlib
    import torch
    from copy import deepcopy
    to_parameter = G.install_stubs()
    nw = importlib.import_module("imitation_lib.utils.networks")
    iq = importlib.import_module("imitation_lib.imitation.iq_sac")
    mod = importlib.import_module("imitation_lib.imitation.lsiq_hc" if spec["cost"] else "imitation_lib.imitation.lsiq_h")
    cls = mod.LSIQ_HC if spec["cost"] else mod.LSIQ_H
    obs, act, nxt, absorbing, min_a, max_a = G.inputs()
    torch.manual_seed(5)
    net = lambda i, o: nw.FullyConnectedNetwork(input_shape=(i,), output_shape=(o,), n_features=[512, 256],
                                                activations=["relu", "relu", "identity"], standardizer=nw.Standardizer())
    pnet, cnet, hnet = net(IN_DIM, 2 * ACT_DIM), net(D, 1), net(D, 1)
    with torch.no_grad():
        pnet._linears[1].weight.copy_(torch.from_numpy(w2_init(11)))
        pnet._linears[2].weight.mul_(G.W3_SCALE)
        pnet._linears[2].bias[ACT_DIM:].add_(G.LOG_SIGMA_SHIFT)
        cnet._linears[1].weight.copy_(torch.from_numpy(w2_init(12)))
        cnet._linears[2].weight.mul_(GL.Q_W3_SCALE)
        cnet._linears[2].bias.mul_(GL.Q_W3_SCALE).add_(GL.Q_B3_SHIFT)
        hnet._linears[1].weight.copy_(torch.from_numpy(w2_init(H_W2_SEED)))
        hnet._linears[2].weight.mul_(H_W3_SCALE)
        hnet._linears[2].bias.mul_(H_W3_SCALE)
    tnet, thnet = deepcopy(cnet), deepcopy(hnet)
    p_init, c_init, h_init = G.params_of(pnet), G.params_of(cnet), G.params_of(hnet)
    policy = iq.IQ_Learn_Policy(G.Reg(pnet), min_a, max_a, G.LOG_STD_MIN, G.LOG_STD_MAX)
    ag = cls.__new__(cls)
    ag.mdp_info = types.SimpleNamespace(gamma=GAMMA)
    ag.policy, ag._use_cuda = policy, False
    ag._critic_approximator, ag._target_critic_approximator = G.Reg(cnet), G.Reg(tnet)
    ag._H_approximator, ag._target_H_approximator = RegList(hnet), RegList(thnet)
    ag._use_target = spec["use_target"]
    ag._log_alpha = torch.tensor(np.log(INIT_ALPHA), dtype=torch.float32)
    ag._plcy_loss_mode, ag._regularizer_mode = "value", "exp_and_plcy"
    ag._gp_lambda, ag._reg_mult, ag._treat_absorbing_states = 0.0, spec["reg_mult"], False
    ag._Q_max, ag._Q_min, ag._loss_mode_exp, ag._Q_exp_loss = Q_MAX, Q_MIN, "fix", "MSE"
    ag._target_clipping, ag._lossQ_type = True, "iq_like"
    ag._iter, ag._logging_iter, ag._sw = 1, 1, G.Recorder()
    ag._tau = to_parameter(spec["tau"])
    ag._critic_optimizer = torch.optim.Adam(cnet.parameters(), lr=LR)
    ag._H_optimizer = torch.optim.Adam(hnet.parameters(), lr=H_LR)
    ag._clip_expert_entropy_to_policy_max, ag._max_H_policy = True, None
    ag._max_H_policy_tau_down, ag._max_H_policy_tau_up = TAU_DOWN, TAU_UP
    if spec["cost"]:
        ag._H_tau, ag._H_loss_mode = to_parameter(H_TAU), spec["loss"]
    alpha = float(ag._alpha)
    ag._delay_Q, ag._delay_pi, ag._warmup_transitions = 1, 1, to_parameter(0)
    ag._replay_memory = types.SimpleNamespace(size=100)
    ag._train_policy_only_on_own_states, ag._learnable_alpha = False, False
    actor_optimizer = torch.optim.Adam(pnet.parameters(), lr=LR_ACTOR)

    def _optimize_actor_parameters(loss):
        # RESTATEMENT of mushroom-rl's DeepAC._optimize_actor_parameters (no clipping)
        actor_optimizer.zero_grad()
        loss.backward()
        actor_optimizer.step()
    ag._optimize_actor_parameters = _optimize_actor_parameters

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
    maxima = []
    try:
        for i in range(N_ITER):
            ag.iq_update(torch.from_numpy(obs[i]), torch.from_numpy(act[i]), torch.from_numpy(nxt[i]),
                         torch.from_numpy(absorbing[i]), is_expert)
            ag._iter += 1
            policy.iter += 1
            maxima.append(float(ag._max_H_policy))
    finally:
        Normal.rsample = rsample0
    order = (PASSES if spec["cost"] else PASSES[:4]) + PI_PASSES
    n = len(order)
    assert len(eps_log) == len(pass_log) == n * N_ITER
    eps = {k: np.stack([eps_log[n * i + order.index(k)] for i in range(N_ITER)]) for k in order}
    passes = {k: [pass_log[n * i + order.index(k)] for i in range(N_ITER)] for k in order}
    for k in order:
        assert eps[k].shape == (N_ITER, B - N_POLICY if k == "expert" else B, ACT_DIM), (k, eps[k].shape)
    scal = np.full((N_ITER, 16), np.nan)
    for i in range(N_ITER):
        for k, t in enumerate(H_TAGS):
            scal[i, k] = ag._sw.rows[i + 1][t]
    fin = dict(critic=G.params_of(cnet), target=G.params_of(tnet), h=G.params_of(hnet), h_target=G.params_of(thnet),
               policy=G.params_of(pnet))
    heads = lambda d: {"w1_head": d["w1"][:W1_HEAD], "w2_head": d["w2"][:W2_HEAD], **{k: d[k] for k in NAMES if k not in ("w1", "w2")}}
    stored = {f"{group}_{k}": v for group, d in fin.items() for k, v in heads(d).items()}

    # ---- the float64 twin and the wrong readings (tests/lsiq_h_restate.py)
    import lsiq_h_restate as H
    lcfg, hcfg = twin_cfgs(spec, alpha)
    steps = [dict(obs=obs[i], act=act[i], next_obs=nxt[i], absorbing=absorbing[i]) for i in range(N_ITER)]
    q_init, h0 = [c_init[k] for k in NAMES], [h_init[k] for k in NAMES]
    # the twin runs the policy itself on the recorded noise and trains it by the two-critic actor loss: the policy step's
    # forward of each critic feeds that critic's Standardizer, so the critic side cannot be followed without it
    import iq_pi_restate as P
    central, delta = (0.5 * (max_a + min_a)).astype(np.float32), (0.5 * (max_a - min_a)).astype(np.float32)
    case = dict(pparams=[p_init[k] for k in NAMES], qparams=q_init, hparams=h0, central=central, delta=delta, lcfg=lcfg,
                hcfg=hcfg, pcfg=P.PiCfg(lr=LR_ACTOR, ls_min=G.LOG_STD_MIN, ls_max=G.LOG_STD_MAX))
    noise = [{k: eps[k][i] for k in order} for i in range(N_ITER)]

    def whole_run(wrong=None, check=False):
        tw = H.whole_twin(case, wrong=wrong, check=check)
        return tw, np.asarray([tw.iq_update(s, N_POLICY, e)[1] for s, e in zip(steps, noise)])
    twin, twin_out = whole_run(check=True)
    for m in twin.critic.h.margins:
        print(f"{name}: expert rows clipped / free {m['exp_clipped']} / {m['exp_free']} (nearest {m['exp_margin']:.2e}), the "
              f"maximum's branch {m.get('branch', 'first')}, Huber quadratic / linear {m['quadratic']} / {m['linear']}, "
              f"absorbing rows {m['abs_policy']} + {m['abs_expert']}" + (f", LSIQ_HC's clips {m['cost']}" if "cost" in m else ""))
    H.assert_margins(twin.critic.h.margins, name, counts=False)
    st = twin.state()
    err = lambda params, prefix: H.fixture_errors(stored, sys.modules[__name__], params, prefix)
    spreads = dict(critic=err(st["q"]["params"], "critic"), target=err(st["q"]["target"], "target"),
                   h=err(st["h"]["params"], "h"), h_target=err(st["h"]["target"], "h_target"),
                   policy=err(st["policy"]["params"], "policy"),
                   scalars=float(np.abs(scal[:, :7] - twin_out[:, :7]).max()),
                   max=float(np.abs(np.asarray(maxima) - twin_out[:, 8]).max()))
    print(f"{name}: spreads " + " ".join(f"{k} {v:.3e}" for k, v in spreads.items()))
    assert max(spreads[k] for k in ("critic", "target", "h", "h_target", "policy")) <= 1e-5, "the float64 twin does not follow the reference"
    for key, net in (("policy", pnet), ("q", cnet), ("h", hnet)):
        assert np.array_equal(st[key]["colstats"][0], G.stats_of(net._stand, IN_DIM if key == "policy" else D)[0]), key
    tol_par, tol_scal, tol_pol = max(TOL, 4 * spreads["h"]), max(TOL, 4 * spreads["scalars"]), max(TOL, 4 * spreads["policy"])
    rel = lambda o: float((np.abs(o[:, :7] - scal[:, :7]) / np.maximum(1.0, np.abs(scal[:, :7]))).max())
    miss = dict.fromkeys(WRONG, 0.0)
    for wrong in spec["wrong"] + ("h_before_q", "no_h"):
        w, o = whole_run(wrong)
        ws_ = w.state()
        parts = (err(ws_["h"]["params"], "h") / tol_par, rel(o) / tol_scal, err(ws_["policy"]["params"], "policy") / tol_pol)
        miss[wrong] = max(parts)
        print(f"{name}: the {wrong} reading misses the reference run by {parts[0]:.1f} (H's parameters) / {parts[1]:.1f} (the H "
              f"scalars) / {parts[2]:.1f} (the policy's parameters) tolerances")
        assert miss[wrong] > 3.0, wrong
    arrays = dict(obs=obs, act=act, next_obs=nxt, absorbing=absorbing, min_a=min_a, max_a=max_a, scalars=scal,
                  maxima=np.asarray(maxima), policy_colstats=G.stats_of(pnet._stand, IN_DIM),
                  colstats=G.stats_of(cnet._stand, D), target_colstats=G.stats_of(tnet._stand, D),
                  h_colstats=G.stats_of(hnet._stand, D), h_target_colstats=G.stats_of(thnet._stand, D),
                  lr=np.float64(LR), h_lr=np.float64(H_LR), tau=np.float64(spec["tau"]), h_tau=np.float64(H_TAU),
                  tau_up=np.float64(TAU_UP), tau_down=np.float64(TAU_DOWN), gamma=np.float64(GAMMA), alpha=np.float64(alpha),
                  reg_mult=np.float64(spec["reg_mult"]), Q_min=np.float64(Q_MIN), Q_max=np.float64(Q_MAX),
                  n_policy=np.int64(N_POLICY), use_target=np.int64(spec["use_target"]))
    for k in order:
        arrays["eps_" + k] = eps[k]
        if k not in ("expert",) + PI_PASSES:
            arrays["a_" + k] = np.stack([p[0] for p in passes[k]])
            arrays["logp_" + k] = np.stack([p[1] for p in passes[k]])
    for k, v in spreads.items():
        arrays["spread_" + k] = np.float64(v)
    for wrong in WRONG:
        arrays["miss_" + wrong] = np.float64(miss[wrong])
    for k in NAMES:
        if k != "w2":
            arrays[f"policy_init_{k}"], arrays[f"critic_init_{k}"], arrays[f"h_init_{k}"] = p_init[k], c_init[k], h_init[k]
    arrays.update(stored)
    arrays["lr_actor"] = np.float64(LR_ACTOR)
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    fit.write_npz(path, arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    for name, s in FIXTURES.items():
        run(name, s)


if __name__ == "__main__":
    main()
