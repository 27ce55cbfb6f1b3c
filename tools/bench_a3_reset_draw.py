#!/usr/bin/env python3
"""K23: the walking task's reset records drawn on the device (A3DeviceRollout(draw="device"), oly_a3_reset_draw) beside
the host draws (draw="host": numpy into pinned stashes, an upload and a scatter), at BASELINE config 3's rollout
[T, N] = [400, 4096] with the persistent kernel (K13).  Run the tool twice and compare the two JSON lines before quoting
a number.

    rollouts  one device_rollout per sample, host clock around it with a device synchronise at the end (the host's draws
              run behind the kernel and count only where the device waits for them); warm-up first, the median of the
              repetitions; every variant is measured twice, alternating (name, name_again), to show the run-to-run spread:
                host_4           draw="host", 4 records per environment (the default)
                device_32        draw="device", 32 records per environment (its default)
                device_rollout   draw="device", pool_depth="rollout": T + 1 records, none is ever used twice
              with the resets and the re-used records of the last rollout (last_info)
    launch    oly_a3_reset_draw alone at 4 / 32 / T + 1 records per environment, HIP events on the kernel's stream, with
              the bytes it writes (N * depth * 656) over that time

    python tools/bench_a3_reset_draw.py [--rollout 400x4096] [--max_traj_len 400] [--p_bad 0.03] [--reps 7] [--launch-reps 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "olympics-mujoco_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

VARIANTS = (("host_4", dict(reset_draw="host")), ("device_32", dict(reset_draw="device", reset_seed=1)),
            ("device_rollout", dict(reset_draw="device", reset_seed=1, reset_pool_depth="rollout")))


def rollouts(kw, blocks, pi, vf, T, N, max_len, reps, warmup):
    from olympic_hip import specs
    from olympic_hip.a3 import ReplayA3Physics, VecA3Env
    from olympic_hip.engine import Engine
    from olympic_hip.synthetic import A3_FLOOR_BODY, A3_GEOM_BODYID, A3_LFOOT_BODY, A3_RFOOT_BODY
    env = VecA3Env(specs.A3Spec(mass=41.5), N, Engine(0), ReplayA3Physics(dict(blocks)), A3_GEOM_BODYID, A3_FLOOR_BODY,
                   A3_RFOOT_BODY, A3_LFOOT_BODY, rs=np.random.RandomState(0), **kw)
    torch.manual_seed(0)
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.device_rollout(pi, vf, T, max_len, graph=False, persistent=True)
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    r = env._dev_rollout
    row = dict(rollout_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), pool_depth=r.depth,
               ring_mb=r.pool.numel() / 1e6, **r.last_info)
    r.close()
    env.eng.ctx.close()
    return row


def launch_alone(N, depths, reps, warmup):
    from olympic_hip._ffi import HipTimer
    from olympic_hip.engine import Engine
    eng, tm, res = Engine(0), HipTimer(), {}
    for depth in depths:
        pool = torch.empty(N * depth * 656, dtype=torch.uint8, device="cuda")
        base = torch.zeros(N, dtype=torch.int64, device="cuda")
        count = torch.ones(N, dtype=torch.int32, device="cuda")
        out = []
        for i in range(warmup + reps):
            count.fill_(3)                                   # a call that moves every ring on
            tm.start(eng._s())
            eng.a3_reset_draw(pool, base, count, depth, 1, 0.05, 88)
            tm.stop(eng._s())
            ms = tm.elapsed_ms()
            if i >= warmup:
                out.append(ms)
        med = statistics.median(out)
        res[f"depth_{depth}"] = dict(launch_us=1e3 * med, min_us=1e3 * min(out), max_us=1e3 * max(out),
                                     bytes=pool.numel(), gb_per_s=pool.numel() / (1e6 * med))
    eng.ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollout", default="400x4096")
    ap.add_argument("--max_traj_len", type=int, default=400)
    ap.add_argument("--K", type=int, default=32, help="readback rows of the synthetic physics")
    ap.add_argument("--p_bad", type=float, default=1.0 / 300,
                    help="probability per (step, environment) of a fall: 1/300 is config 3's, 0.03 an untrained policy's "
                         "(an episode of a few dozen steps, about 12 resets per environment and rollout)")
    ap.add_argument("--reps", type=int, default=7, help="rollouts per median")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launch-reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_a3_reset_draw needs the GPU: nothing is measured without one")
    from olympic_hip.ppo import MLPCritic, MLPGaussianActor
    from olympic_hip.synthetic import a3_synthetic_blocks
    T, N = (int(v) for v in args.rollout.split("x"))
    blocks = {k: torch.as_tensor(v).cuda() for k, v in a3_synthetic_blocks(N, args.K, seed=1, p_bad=args.p_bad).items()}
    torch.manual_seed(0)
    pi, vf = MLPGaussianActor(41, 12).cuda(), MLPCritic(41).cuda()
    res = dict(metric="a3_reset_draw", T=T, N=N, max_traj_len=args.max_traj_len, p_bad=args.p_bad, reps=args.reps, rollouts={})
    for suffix in ("", "_again"):
        for name, kw in VARIANTS:
            row = rollouts(kw, blocks, pi, vf, T, N, args.max_traj_len, args.reps, args.warmup)
            res["rollouts"][name + suffix] = row
            print(f"# rollout {name + suffix}: {row}", file=sys.stderr)
    best = {name: min(res["rollouts"][name]["rollout_ms"], res["rollouts"][name + "_again"]["rollout_ms"]) for name, _ in VARIANTS}
    res["host_over_device_32"] = best["host_4"] / best["device_32"]
    res["host_over_device_rollout"] = best["host_4"] / best["device_rollout"]
    res["launch"] = launch_alone(N, (4, 32, T + 1), args.launch_reps, 10)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
