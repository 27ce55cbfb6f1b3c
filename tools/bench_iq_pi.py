#!/usr/bin/env python3
"""K27 measurements, one JSON line: one policy update of IQ-Learn (both Standardizers, no logging) at in = 32, A = 11 and
B = 64 and 512 rows: the oly_iq_pi_update call alone and one whole DeviceIQSAC.iq_update (the policy passes of K25, one
oly_iq_q_update, one oly_iq_pi_update), against the same lines in torch eager on the same GPU (the forwards with the
Standardizers' updates on the device, the losses, backward, torch.optim.Adam on the critic and on the actor, the soft
target update).  Every figure is the median of REPS timed windows of MANY host-driven updates after a warm-up.
launches_*: kernel launches per update, counted with torch.profiler.

    python tools/bench_iq_pi.py [--out FILE] [--kernel-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_iq_q import ACT_DIM, IN_DIM, MANY, REPS, D, Stand, launches, mlp, timed  # noqa: E402


class StandG(Stand):
    """Stand for a row that carries a gradient: the sums take the detached rows (the reference's are numpy), the
    standardised row keeps its graph."""

    def __call__(self, x):
        xd = x.detach().double()
        self.cs[0] += x.shape[0]
        self.cs[1] += xd.sum(0)
        self.cs[2] += (xd * xd).sum(0)
        cnt = self.cs[0] + 1e-2
        mean = self.cs[1] / cnt
        sd = torch.sqrt(torch.clamp((self.cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
        return ((x.double() - mean) / sd).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="time the device path alone")
    args = ap.parse_args()
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceIQSAC, DeviceSoftQCritic
    from olympic_hip.synthetic import il_synthetic_transitions
    eng = Engine(0)
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "in_dim": IN_DIM, "act_dim": ACT_DIM, "reps": REPS, "window": MANY}
    demo = il_synthetic_transitions(64, IN_DIM, ACT_DIM, seed=1)
    for B in (64, 512):
        t = {k: torch.as_tensor(v).cuda() for k, v in il_synthetic_transitions(B, IN_DIM, ACT_DIM, seed=2, absorbing_frac=0.2).items()}
        obs, act, nxt, ab = t["states"], t["actions"], t["next_states"], t["absorbing"]
        eps_q = {k: torch.randn((B if k != "expert" else B // 2, ACT_DIM), device="cuda") for k in ("next", "pi", "expert")}
        eps_pi = dict(pi=torch.randn((B, ACT_DIM), device="cuda"))
        tag = f"b{B}"
        p_lins = [torch.nn.Linear(IN_DIM, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * ACT_DIM)]
        with torch.no_grad():
            p_lins[2].weight.mul_(0.1)
        pol = DeviceSquashedGaussianPolicy(eng, p_lins, -np.ones(ACT_DIM), np.ones(ACT_DIM),
                                           standardizer=DeviceStandardizer(eng, IN_DIM))
        c_lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
        cr = DeviceSoftQCritic(eng, c_lins, standardizer=DeviceStandardizer(eng, D), lr=3e-4, tau=0.005)
        ag = DeviceIQSAC(eng, pol, cr, demo, gamma=0.99, batch_size=B // 2, use_target=True, logging_iter=10 ** 9,
                         max_replay_size=8, actor_optimizer=dict(lr=3e-4))
        ag.replay.add(demo)
        k27 = lambda: ag.update_policy(obs, B // 2, eps=eps_pi)
        res[f"k27_us_{tag}"] = timed(lambda: [k27() for _ in range(MANY)], REPS) * 1e3 / MANY
        res[f"k27_launches_{tag}"] = launches(k27)
        upd = lambda: ag.iq_update(obs, act, nxt, ab, B // 2, eps=dict(q=eps_q, pi=eps_pi))
        res[f"iq_update_us_{tag}"] = timed(lambda: [upd() for _ in range(MANY)], REPS) * 1e3 / MANY
        res[f"iq_update_launches_{tag}"] = launches(upd)
        if args.kernel_only:
            continue
        # torch eager: the reference's lines on the same GPU
        pnet, cnet, tnet = mlp(IN_DIM, 2 * ACT_DIM), mlp(D, 1), mlp(D, 1)
        tnet.load_state_dict(cnet.state_dict())
        ps, cs, ts = Stand(IN_DIM), StandG(D), Stand(D)
        copt = torch.optim.Adam(cnet.parameters(), lr=3e-4)
        popt = torch.optim.Adam(pnet.parameters(), lr=3e-4)
        alpha, gamma, tau, reg = 1e-3, 0.99, 0.005, 0.5
        is_exp = torch.arange(B, device="cuda") >= B // 2

        def act_logp(x, e):
            y = pnet(ps(x))
            mu, ls = y[:, :ACT_DIM], torch.clamp(y[:, ACT_DIM:], -20.0, 2.0)
            raw = mu + ls.exp() * e
            a = torch.tanh(raw)
            lp = torch.distributions.Normal(mu, ls.exp()).log_prob(raw).sum(1) - torch.log(1.0 - a.pow(2) + 1e-6).sum(1)
            return a, lp

        def torch_policy():
            a_new, lp = act_logp(obs, eps_pi["pi"])
            q = cnet(cs(torch.cat([obs, a_new], 1)))
            loss = (alpha * lp - q).mean()
            popt.zero_grad()
            loss.backward()
            popt.step()

        def torch_q():
            q = cnet(cs(torch.cat([obs, act], 1)))
            with torch.no_grad():
                a1, lp1 = act_logp(nxt, eps_q["next"])
                nv = tnet(ts(torch.cat([nxt, a1], 1))) - alpha * lp1.unsqueeze(1)
                a2, lp2 = act_logp(obs, eps_q["pi"])
            y = (1 - ab.unsqueeze(1)) * gamma * nv
            reward = q - y
            v = cnet(cs(torch.cat([obs, a2], 1))) - alpha * lp2.unsqueeze(1)
            loss = -reward[is_exp].mean() + (v - y).mean() + (reg * torch.square(reward)).mean()
            copt.zero_grad()
            loss.backward()
            copt.step()
            with torch.no_grad():
                for p, q_ in zip(cnet.parameters(), tnet.parameters()):
                    q_.copy_(tau * p + (1 - tau) * q_)

        def torch_update():
            torch_q()
            torch_policy()
        n_torch = 50
        res[f"torch_policy_us_{tag}"] = timed(lambda: [torch_policy() for _ in range(n_torch)], REPS, warmup=1) * 1e3 / n_torch
        res[f"torch_policy_launches_{tag}"] = launches(torch_policy)
        res[f"torch_iq_update_us_{tag}"] = timed(lambda: [torch_update() for _ in range(n_torch)], REPS, warmup=1) * 1e3 / n_torch
        res[f"torch_iq_update_launches_{tag}"] = launches(torch_update)
        res[f"speedup_policy_{tag}"] = res[f"torch_policy_us_{tag}"] / res[f"k27_us_{tag}"]
        res[f"speedup_iq_update_{tag}"] = res[f"torch_iq_update_us_{tag}"] / res[f"iq_update_us_{tag}"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
