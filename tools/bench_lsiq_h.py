#!/usr/bin/env python3
"""The H update of LSIQ_H / LSIQ_HC, one JSON line: at in = 32, A = 11 and B = 64 and 512 rows, with both critics'
Standardizers, in the same process
  lsiq      DeviceLSIQ.update_Q_function (iq_like, fix / MSE, clipping): the update the two agents extend
  lsiq_h    DeviceLSIQH.update_Q_function: that update with alpha 0, the H update's policy pass, oly_iq_q_update "lsiq_h"
  lsiq_hc   DeviceLSIQHC.update_Q_function: also the two target-critic passes, Huber, the deferred target update
each whole (`update_us_*`, with its launch count), update_policy (K27; `pi_us_*`: with one critic for lsiq, with Q + H for
the other two), one whole iq_update (`iq_update_us_*`, with its launch count) and the oly_iq_q_update call of the H update
alone (`h_us_*`), timed in
TWO runs (both shown: [run 1, run 2], the median of REPS windows each), and in torch eager on the same GPU
update_H_function of both classes with the reference's [B, B] broadcast (`torch_h_us_*`), the two-critic actor step
(`torch_pi_us_*`) and one whole iq_update (`torch_iq_update_us_*`).  tools/bench_lsiq_q.py's protocol.

    python tools/bench_lsiq_h.py [--out FILE] [--kernel-only]
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_iq_q import ACT_DIM, IN_DIM, MANY, REPS, D, Stand, launches, mlp, timed  # noqa: E402

Q_MIN, Q_MAX, ALPHA = -1.0, 1.0, 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="time the device path alone")
    args = ap.parse_args()
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceLSIQHCSAC, DeviceLSIQHSAC, DeviceLSIQSAC, DeviceSoftQCritic
    from olympic_hip.synthetic import il_synthetic_transitions
    eng = Engine(0)
    torch.manual_seed(0)
    warnings.simplefilter("ignore")
    res = {"device": torch.cuda.get_device_name(0), "in_dim": IN_DIM, "act_dim": ACT_DIM, "reps": REPS, "runs": 2}
    demo = il_synthetic_transitions(64, IN_DIM, ACT_DIM, seed=1)
    twice = lambda fn, many: [timed(lambda: [fn() for _ in range(many)], REPS) * 1e3 / many for _ in range(2)]
    critic = lambda: DeviceSoftQCritic(eng, [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)],
                                       standardizer=DeviceStandardizer(eng, D), lr=3e-4, tau=0.005)
    for B in (64, 512):
        n_p = B // 2
        t = {k: torch.as_tensor(v).cuda() for k, v in il_synthetic_transitions(B, IN_DIM, ACT_DIM, seed=2, absorbing_frac=0.2).items()}
        obs, act, nxt, ab = t["states"], t["actions"], t["next_states"], t["absorbing"]
        eps = {k: torch.randn((B - n_p if k == "expert" else B, ACT_DIM), device="cuda")
               for k in ("next", "pi", "expert", "h_next", "h_pi")}
        for name in ("lsiq", "lsiq_h", "lsiq_hc"):
            tag = f"{name}_b{B}"
            p_lins = [torch.nn.Linear(IN_DIM, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * ACT_DIM)]
            pol = DeviceSquashedGaussianPolicy(eng, p_lins, -np.ones(ACT_DIM), np.ones(ACT_DIM),
                                               standardizer=DeviceStandardizer(eng, IN_DIM))
            kw = dict(gamma=0.99, batch_size=n_p, use_target=True, logging_iter=10 ** 9, max_replay_size=8, Q_min=Q_MIN,
                      Q_max=Q_MAX, target_clipping=True, lossQ_type="iq_like", loss_mode_exp="fix", Q_exp_loss="MSE",
                      init_alpha=ALPHA)
            if name == "lsiq":
                ag = DeviceLSIQSAC(eng, pol, critic(), demo, **kw)
            elif name == "lsiq_h":
                ag = DeviceLSIQHSAC(eng, pol, critic(), demo, h_critic=critic(), **kw)
            else:
                ag = DeviceLSIQHCSAC(eng, pol, critic(), demo, h_critic=critic(), H_tau=0.01, H_loss_mode="Huber", **kw)
            upd = lambda: ag.update_Q_function(obs, act, nxt, ab, n_p, eps=eps)
            res[f"update_us_{tag}"] = twice(upd, MANY)
            res[f"launches_{tag}"] = launches(upd)
            eps_pi = dict(pi=torch.randn((B, ACT_DIM), device="cuda"))
            pi = lambda: ag.update_policy(obs, n_p, eps=eps_pi)
            res[f"pi_us_{tag}"] = twice(pi, MANY)
            res[f"pi_launches_{tag}"] = launches(pi)
            ag.replay.add(dict(states=obs[:8], actions=act[:8], next_states=nxt[:8], absorbing=ab[:8]))   # past the warm-up
            whole = lambda: ag.iq_update(obs, act, nxt, ab, n_p, eps=dict(q=eps, pi=eps_pi))
            res[f"iq_update_us_{tag}"] = twice(whole, MANY)
            res[f"iq_update_launches_{tag}"] = launches(whole)
            if name == "lsiq":
                continue
            h, cost = ag.h_critic, name == "lsiq_hc"
            a_n, lp_n = ag._policy_pass(nxt, eps["h_next"], None)
            q_t = ag.critic.predict_target(obs, act).reshape(-1) if cost else None
            v_t = ag.critic.predict_target(obs, a_n).reshape(-1) if cost else None
            ws = ag._workspace(B)
            block = dict(Q_min=Q_MIN, Q_max=Q_MAX, h=dict(loss="Huber" if cost else "MSE", cost=cost, clip_expert=True,
                                                          max_state=ag.h_max_state, q_t=q_t, v_t=v_t))

            def h_update():
                eng.iq_q_update(obs, act, nxt, ab, a_n, lp_n, None, None, n_p, h.stand.colstats, h.target_stand.colstats,
                                h.param, h.exp_avg, h.exp_avg_sq, h.packed, h.target_param, h.target_packed, ws, h.step, h.lr,
                                algo="lsiq_h", alpha=ag.alpha, reg_mult=ag.reg_mult, tau=h.tau, lsiq=block)
                h.step += 1
            res[f"h_us_{tag}"] = twice(h_update, MANY)
            res[f"h_launches_{tag}"] = launches(h_update)
            if args.kernel_only:
                continue
            # torch eager: update_H_function's lines on the same GPU, the [B] absorbing against [B, 1] terms
            pnet, hnet, thnet, tqnet = mlp(IN_DIM, 2 * ACT_DIM), mlp(D, 1), mlp(D, 1), mlp(D, 1)
            thnet.load_state_dict(hnet.state_dict())
            ps, hs, ths, tqs = Stand(IN_DIM), Stand(D), Stand(D), Stand(D)
            opt = torch.optim.Adam(hnet.parameters(), lr=3e-4)
            gamma, tau, reg = 0.99, 0.005, 0.5
            is_exp = torch.arange(B, device="cuda") >= n_p
            state = {"max": None}

            def act_logp(x, e):
                with torch.no_grad():
                    y = pnet(ps(x))
                    mu, lsg = y[:, :ACT_DIM], torch.clamp(y[:, ACT_DIM:], -20.0, 2.0)
                    raw = mu + lsg.exp() * e
                    a = torch.tanh(raw)
                    lp = torch.distributions.Normal(mu, lsg.exp()).log_prob(raw).sum(1) - torch.log(1.0 - a.pow(2) + 1e-6).sum(1)
                return a, lp

            def torch_update():
                H = hnet(hs(torch.cat([obs, act], 1)))
                a1, lp1 = act_logp(nxt, eps["h_next"])
                squared = 0.0
                if cost:
                    with torch.no_grad():
                        q = tqnet(tqs(torch.cat([obs, act], 1)))
                        a2, _ = act_logp(obs, eps["h_pi"])
                        v = tqnet(tqs(torch.cat([obs, a2], 1)))
                        y = (1 - ab) * gamma * torch.clip(v, Q_MIN, Q_MAX)
                        squared = (1 - ab) * reg * torch.square(torch.clip(q - y, -1 / reg, 1 / reg)) + \
                            ab * (1.0 - gamma) * reg * torch.square(torch.clip(q - y, Q_MIN, Q_MAX))
                neg = -lp1
                cur = torch.max(neg[~is_exp])
                if state["max"] is None:
                    state["max"] = cur
                elif cur > state["max"]:                 # the reference's data-dependent branch: a read-back
                    state["max"] = (1 - 1e-2) * state["max"] + 1e-2 * cur
                else:
                    state["max"] = (1 - 1e-4) * state["max"] + 1e-4 * cur
                neg[is_exp] = torch.clip(neg[is_exp], state["max"], 100000)
                with torch.no_grad():
                    next_H = thnet(ths(torch.cat([nxt, a1], 1))) + ALPHA * neg.unsqueeze(1)
                target = squared + (1 - ab) * gamma * next_H
                target = torch.clip(target, -1000, (1 / reg) ** 2 / (1 - gamma) + 100) if cost else torch.clip(target, -10000, 1000)
                loss = F.huber_loss(H, target) if cost else F.mse_loss(H, target)
                opt.zero_grad()
                loss.backward()
                opt.step()
                with torch.no_grad():
                    for p, q_ in zip(hnet.parameters(), thnet.parameters()):
                        q_.copy_(tau * p + (1 - tau) * q_)
            res[f"torch_h_us_{tag}"] = twice(torch_update, 50)
            res[f"torch_h_launches_{tag}"] = launches(torch_update)
            # the two-critic actor step (lsiq_h.py:104-108) and one whole iq_update in eager: LSIQ's Q update with the
            # entropy-free values (tools/bench_lsiq_q.py's lines), update_H_function above, the actor step
            qnet, qs = mlp(D, 1), Stand(D)
            tqnet.load_state_dict(qnet.state_dict())
            qopt = torch.optim.Adam(qnet.parameters(), lr=3e-4)
            popt = torch.optim.Adam(pnet.parameters(), lr=3e-4)

            def act_logp_grad(x, e):
                y = pnet(ps(x))
                mu, lsg = y[:, :ACT_DIM], torch.clamp(y[:, ACT_DIM:], -20.0, 2.0)
                raw = mu + lsg.exp() * e
                a = torch.tanh(raw)
                return a, torch.distributions.Normal(mu, lsg.exp()).log_prob(raw).sum(1) - torch.log(1.0 - a.pow(2) + 1e-6).sum(1)

            def stand(st, x):
                # the Standardizer takes the rows (its sums carry no gradient), the row itself carries it
                with torch.no_grad():
                    st(x)
                    cnt = st.cs[0] + 1e-2
                    mean = st.cs[1] / cnt
                    sd = torch.sqrt(torch.clamp((st.cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
                return ((x.double() - mean) / sd).float()

            def torch_policy():
                a_new, lp = act_logp_grad(obs, eps_pi["pi"])
                xa = torch.cat([obs, a_new], 1)
                soft_q = qnet(stand(qs, xa)) + hnet(stand(hs, xa))
                loss = (ALPHA * lp - soft_q).mean()
                popt.zero_grad()
                loss.backward()
                popt.step()

            def torch_q():
                q = qnet(qs(torch.cat([obs, act], 1)))
                a1, _ = act_logp(nxt, eps["next"])
                with torch.no_grad():
                    nv = tqnet(tqs(torch.cat([nxt, a1], 1)))
                y = (1 - ab.unsqueeze(1)) * gamma * torch.clip(nv, Q_MIN, Q_MAX)
                a2, _ = act_logp(obs, eps["pi"])
                v = qnet(qs(torch.cat([obs, a2], 1)))
                loss = F.mse_loss(q[is_exp], torch.ones_like(q[is_exp]) * Q_MAX) + (v - y).mean() + \
                    (reg * torch.square(q - y)).mean()
                qopt.zero_grad()
                loss.backward()
                qopt.step()

            def torch_whole():
                torch_q()
                torch_update()
                torch_policy()
                with torch.no_grad():
                    for p, q_ in zip(qnet.parameters(), tqnet.parameters()):
                        q_.copy_(tau * p + (1 - tau) * q_)
            res[f"torch_pi_us_{tag}"] = twice(torch_policy, 50)
            res[f"torch_pi_launches_{tag}"] = launches(torch_policy)
            res[f"torch_iq_update_us_{tag}"] = twice(torch_whole, 50)
            res[f"torch_iq_update_launches_{tag}"] = launches(torch_whole)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
