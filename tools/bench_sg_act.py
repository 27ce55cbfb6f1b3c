#!/usr/bin/env python3
"""K25 measurements, one JSON line, at UnitreeH1's shape (in = 32, A = 11), HIP events on the stream, every figure the
median of REPS timed windows after a warm-up:

    act    one acting step DeviceSquashedGaussianPolicy.act(ctrl=True) at N = 1 and N = 4096 with fused_act=True
           (torch.randn, oly_col_stats' launches, ONE sg_act_kernel) against fused_act=False (oly_col_stats,
           oly_ilmlp_forward, randn and about ten torch elementwise launches, oly_il_ctrl); a window is CALLS calls.
           Also compute_action_and_log_prob, both ways.
    fit    one step of fit_offline at batch 32 and 256 (20 000 rows, a Standardizer) as the mean over a 1000-step call,
           with empirical_entropy=True at logging_iter=1 (every step runs K25's kernel and the fold) against off.

    python tools/bench_sg_act.py [--out FILE]
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

REPS, CALLS = 7, 200
IN_DIM, ACT_DIM, N_ROWS = 32, 11, 20000


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", default="1,4096")
    args = ap.parse_args()
    from olympic_hip import specs
    from olympic_hip.bc import DeviceBehavioralCloning, DeviceSquashedGaussianPolicy
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    eng = Engine(0).il_configure(specs.unitree_h1("walk"))
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "in_dim": IN_DIM, "act_dim": ACT_DIM, "reps": REPS, "calls": CALLS}

    def policy(fused):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(1)
            lins = [torch.nn.Linear(IN_DIM, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, 2 * ACT_DIM)]
        return DeviceSquashedGaussianPolicy(eng, lins, -np.ones(ACT_DIM), np.ones(ACT_DIM),
                                            standardizer=DeviceStandardizer(eng, IN_DIM), fused_act=fused)
    for N in (int(v) for v in args.envs.split(",")):
        x = torch.as_tensor((rng.standard_normal((N, IN_DIM)) * 2 + 1).astype(np.float32)).cuda()
        for fused in (True, False):
            pol = policy(fused)
            pol.act(x, generator=gen)                   # the statistics are no longer fresh
            tag = "fused" if fused else "unfused"
            ms = timed(lambda: [pol.act(x, generator=gen, ctrl=True) for _ in range(CALLS)], REPS)
            res[f"act_us_N{N}_{tag}"] = ms * 1e3 / CALLS
            ms = timed(lambda: [pol.compute_action_and_log_prob(x, generator=gen) for _ in range(CALLS)], REPS)
            res[f"log_prob_us_N{N}_{tag}"] = ms * 1e3 / CALLS
        res[f"act_unfused_over_fused_N{N}"] = res[f"act_us_N{N}_unfused"] / res[f"act_us_N{N}_fused"]
        res[f"log_prob_unfused_over_fused_N{N}"] = res[f"log_prob_us_N{N}_unfused"] / res[f"log_prob_us_N{N}_fused"]

    states = torch.as_tensor((rng.standard_normal((N_ROWS, IN_DIM)) * rng.uniform(0.3, 3, IN_DIM)).astype(np.float32)).cuda()
    actions = torch.as_tensor(np.tanh(rng.standard_normal((N_ROWS, ACT_DIM))).astype(np.float32)).cuda()
    for batch in (32, 256):
        for logged in (True, False):
            bc = DeviceBehavioralCloning(eng, policy(False), dict(states=states, actions=actions), lr=1e-4, batch_size=batch,
                                         logging_iter=1, empirical_entropy=logged)
            idx = bc.draw_idx(1000, gen)
            eps = torch.randn((1000, batch, ACT_DIM), device="cuda", generator=gen) if logged else None
            ms = timed(lambda: bc.fit_offline(1000, idx=idx, eps=eps), REPS)
            res[f"fit_us_per_step_b{batch}_{'logged' if logged else 'plain'}"] = ms     # ms per 1000 steps = us per step
        res[f"fit_logging_extra_us_b{batch}"] = res[f"fit_us_per_step_b{batch}_logged"] - res[f"fit_us_per_step_b{batch}_plain"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
