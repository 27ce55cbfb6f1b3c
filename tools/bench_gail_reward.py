#!/usr/bin/env python3
"""Config 4: the VAIL discriminator reward + GAE(0.97) + biased-std normalisation pipeline on
UnitreeH1-shaped observations (mask + running standardisation on the device, encoder / decoder
GEMMs in PyTorch-ROCm, reparameterisation and reward epilogue as HIP kernels, K6, K7).
Wall clock per call with a device sync on both sides.  Prints one JSON object.

With --algo / --in-dim / --pair only the discriminator reward is measured (statistics update + forward, one call), two
runs at [1, 4096] and [100, 4096]: VAIL's (K12) or GAIL's (K18), states only at --in-dim columns or the paired input
((s, s') at 32 + 32 with --pair next_state, (s, a) at 32 + 11 with --pair action):

    python tools/bench_gail_reward.py --algo gail --in-dim 64
    python tools/bench_gail_reward.py --algo gail --pair next_state"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "olympics-mujoco_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from olympic_hip.engine import Engine  # noqa: E402
from olympic_hip.gail import DiscriminatorReward, GAILAdvantage, VariationalDiscriminator  # noqa: E402
from olympic_hip.ppo import MLPCritic  # noqa: E402


def reward_only(eng, a):
    from olympic_hip.gail import GAILDiscriminator, GAILDiscriminatorReward
    ds, d2 = (32, 32 if a.pair == "next_state" else 11) if a.pair else (a.in_dim, 0)
    kw = dict(state_mask=np.arange(ds))
    if a.pair:
        kw.update(pair=a.pair, act_mask=None if a.pair == "next_state" else np.arange(d2))
    if a.algo == "gail":
        disc = GAILDiscriminatorReward(eng, GAILDiscriminator(ds + d2).cuda(), **kw)
    else:
        disc = DiscriminatorReward(eng, VariationalDiscriminator(ds + d2).cuda(), **kw)
    out = dict(algo=a.algo, in_dim=ds + d2, pair=a.pair)
    for T, N in ((1, 4096), (100, 4096)):
        x = torch.randn((T * N, ds), device="cuda")
        x2 = torch.randn((T * N, d2), device="cuda") if a.pair else None
        eps = torch.randn((T * N, 128), device="cuda")
        call = (lambda: disc(x, eps, x2=x2)) if a.pair else (lambda: disc(x, eps))
        runs = []
        for _ in range(2):
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            reps = 200 if T == 1 else 20
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / reps * 1e3)
        out[f"[{T},{N}]"] = dict(discriminator_reward_ms_runs=runs)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("vail", "gail"), default=None)
    ap.add_argument("--in-dim", type=int, default=None)
    ap.add_argument("--pair", choices=("next_state", "action"), default=None)
    a = ap.parse_args()
    eng = Engine(0)
    torch.manual_seed(0)
    if a.algo or a.in_dim or a.pair:
        a.algo, a.in_dim = a.algo or "vail", a.in_dim or 32
        return reward_only(eng, a)
    net = VariationalDiscriminator(32).cuda()
    disc = DiscriminatorReward(eng, net, state_mask=np.arange(32))
    critic = MLPCritic(32).cuda()
    out = {}
    for T, N in ((1, 4096), (400, 4096)):
        x = torch.randn((T, N, 32), device="cuda")
        xn = torch.randn((T, N, 32), device="cuda")
        r_env = torch.zeros((T, N), device="cuda")
        ab = torch.rand((T, N), device="cuda") < 0.003
        last = ab | (torch.rand((T, N), device="cuda") < 0.003)
        eps = torch.randn((T * N, 128), device="cuda")
        flat = x.reshape(T * N, 32).contiguous()

        def timeit(fn, reps):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3
        adv = GAILAdvantage(eng, disc, critic, gamma=0.99, lam=0.97)
        reps = 200 if T == 1 else 10
        out[f"[{T},{N}]"] = dict(discriminator_reward_ms=timeit(lambda: disc(flat, eps), reps),
                                 reward_gae_normalise_ms=timeit(lambda: adv(x, xn, r_env, ab, last, eps), reps),
                                 samples=T * N)
        out[f"[{T},{N}]"]["samples_per_s_full_pipeline"] = T * N / out[f"[{T},{N}]"]["reward_gae_normalise_ms"] * 1e3
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
