#!/usr/bin/env python3
"""K26 measurements, one JSON line: one critic update of IQ-Learn (plcy_loss_mode value, regularizer exp_and_plcy, both
Standardizers) at in = 32, A = 11 and B = 64 and 512 rows, with and without a target: DeviceIQLearn.update_Q_function
(the policy passes of K25 and one oly_iq_q_update) and the oly_iq_q_update call alone, against the same lines in torch
eager on the same GPU (the policy's and the critic's forwards with the Standardizers' updates on the device, the loss,
backward, torch.optim.Adam, the soft target update).  Every figure is the median of REPS timed windows after a warm-up.
launches_*: kernel launches per update, counted with torch.profiler.

    python tools/bench_iq_q.py [--out FILE] [--kernel-only]

--kernel-only leaves the torch loop out (a kernel trace of the run then holds the device path's launches alone).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPS, MANY = 7, 100
IN_DIM, ACT_DIM = 32, 11
D = IN_DIM + ACT_DIM


def timed(fn, reps, warmup=2):
    """Median milliseconds of `reps` windows of one fn() each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def launches(fn):
    """Kernel launches of one fn()."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
               and "Memset" not in e.name)


class Stand:
    """The reference's Standardizer with its sums on the device."""

    def __init__(self, dim):
        self.cs = torch.zeros((3, dim), dtype=torch.float64, device="cuda")

    def __call__(self, x):
        xd = x.double()
        self.cs[0] += x.shape[0]
        self.cs[1] += xd.sum(0)
        self.cs[2] += (xd * xd).sum(0)
        cnt = self.cs[0] + 1e-2
        mean = self.cs[1] / cnt
        sd = torch.sqrt(torch.clamp((self.cs[2] + 1e-2) / cnt - mean * mean, min=1e-2))
        return ((xd - mean) / sd).float()


def mlp(i, o):
    return torch.nn.Sequential(torch.nn.Linear(i, 512), torch.nn.ReLU(), torch.nn.Linear(512, 256), torch.nn.ReLU(),
                               torch.nn.Linear(256, o)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="time the device path alone")
    args = ap.parse_args()
    from olympic_hip.bc import DeviceSquashedGaussianPolicy
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.iq import DeviceIQLearn, DeviceSoftQCritic
    from olympic_hip.synthetic import il_synthetic_transitions
    eng = Engine(0)
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "in_dim": IN_DIM, "act_dim": ACT_DIM, "reps": REPS}
    demo = il_synthetic_transitions(64, IN_DIM, ACT_DIM, seed=1)
    for B in (64, 512):
        t = {k: torch.as_tensor(v).cuda() for k, v in il_synthetic_transitions(B, IN_DIM, ACT_DIM, seed=2, absorbing_frac=0.2).items()}
        obs, act, nxt, ab = t["states"], t["actions"], t["next_states"], t["absorbing"]
        eps = {k: torch.randn((B if k != "expert" else B // 2, ACT_DIM), device="cuda") for k in ("next", "pi", "expert")}
        for use_target in (True, False):
            tag = f"b{B}_{'target' if use_target else 'notarget'}"
            p_lins = [torch.nn.Linear(IN_DIM, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * ACT_DIM)]
            pol = DeviceSquashedGaussianPolicy(eng, p_lins, -np.ones(ACT_DIM), np.ones(ACT_DIM),
                                               standardizer=DeviceStandardizer(eng, IN_DIM))
            c_lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 1)]
            cr = DeviceSoftQCritic(eng, c_lins, standardizer=DeviceStandardizer(eng, D), lr=3e-4, tau=0.005)
            ag = DeviceIQLearn(eng, pol, cr, demo, gamma=0.99, batch_size=B // 2, use_target=use_target, logging_iter=10 ** 9,
                               max_replay_size=8)
            upd = lambda: ag.update_Q_function(obs, act, nxt, ab, B // 2, eps=eps)
            res[f"update_us_{tag}"] = timed(lambda: [upd() for _ in range(MANY)], REPS) * 1e3 / MANY
            res[f"launches_{tag}"] = launches(upd)
            # the K26 call alone, on the actions of one policy pass
            a_n, lp_n = ag._policy_pass(nxt, eps["next"], None)
            a_p, lp_p = ag._policy_pass(obs, eps["pi"], None)
            ws = ag._workspace(B)

            def k26():
                eng.iq_q_update(obs, act, nxt, ab, a_n, lp_n, a_p, lp_p, B // 2, cr.stand.colstats, cr.target_stand.colstats,
                                cr.param, cr.exp_avg, cr.exp_avg_sq, cr.packed, cr.target_param, cr.target_packed, ws, cr.step,
                                cr.lr, use_target=use_target, alpha=ag.alpha, tau=cr.tau)
                cr.step += 1
            res[f"k26_us_{tag}"] = timed(lambda: [k26() for _ in range(MANY)], REPS) * 1e3 / MANY
            res[f"k26_launches_{tag}"] = launches(k26)
            if args.kernel_only:
                continue
            # torch eager: the reference's lines on the same GPU
            pnet, cnet, tnet = mlp(IN_DIM, 2 * ACT_DIM), mlp(D, 1), mlp(D, 1)
            tnet.load_state_dict(cnet.state_dict())
            ps, cs, ts = Stand(IN_DIM), Stand(D), Stand(D)
            opt = torch.optim.Adam(cnet.parameters(), lr=3e-4)
            alpha, gamma, tau, reg = 1e-3, 0.99, 0.005, 0.5
            is_exp = torch.arange(B, device="cuda") >= B // 2

            def act_logp(x, e):
                with torch.no_grad():
                    y = pnet(ps(x))
                    mu, ls = y[:, :ACT_DIM], torch.clamp(y[:, ACT_DIM:], -20.0, 2.0)
                    raw = mu + ls.exp() * e
                    a = torch.tanh(raw)
                    lp = torch.distributions.Normal(mu, ls.exp()).log_prob(raw).sum(1) - torch.log(1.0 - a.pow(2) + 1e-6).sum(1)
                return a, lp.unsqueeze(1)

            def torch_update():
                q = cnet(cs(torch.cat([obs, act], 1)))
                a1, lp1 = act_logp(nxt, eps["next"])
                if use_target:
                    with torch.no_grad():
                        nv = tnet(ts(torch.cat([nxt, a1], 1))) - alpha * lp1
                else:
                    nv = cnet(cs(torch.cat([nxt, a1], 1))) - alpha * lp1
                y = (1 - ab.unsqueeze(1)) * gamma * nv
                reward = q - y
                a2, lp2 = act_logp(obs, eps["pi"])
                v = cnet(cs(torch.cat([obs, a2], 1))) - alpha * lp2
                loss = -reward[is_exp].mean() + (v - y).mean() + (reg * torch.square(reward)).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
                with torch.no_grad():
                    for p, q_ in zip(cnet.parameters(), tnet.parameters()):
                        q_.copy_(tau * p + (1 - tau) * q_)
            n_torch = 50
            res[f"torch_us_{tag}"] = timed(lambda: [torch_update() for _ in range(n_torch)], REPS, warmup=1) * 1e3 / n_torch
            res[f"torch_launches_{tag}"] = launches(torch_update)
            res[f"speedup_{tag}"] = res[f"torch_us_{tag}"] / res[f"update_us_{tag}"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
