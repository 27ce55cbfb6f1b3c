#!/usr/bin/env python3
"""K21: one acting step of the imitation-learning collection loop at UnitreeH1's shape (obs 32 -> 512 -> 256 -> act 11)
for N = 1, 1024 and 4096 environments, timed with HIP events on the kernels' stream (the host's enqueue time is inside the
interval whenever the device waits for it), warm-up first, the median of --reps repetitions:

    (a) act      DeviceGaussianPolicy.act(ctrl=True): torch.randn + ONE oly_il_act call (oly_col_stats' two launches and
                 the act launch)
    (b) parent   DeviceGaussianPolicy.draw_action + oly_il_ctrl, the path before K21: oly_col_stats, oly_ilmlp_forward,
                 randn, exp, mul, add, il_ctrl_kernel
    pieces       every call of (b) and of (a) on its own, for the per-launch breakdown

and the collection of one ILCore.learn fit ([100, 4096] on KinematicPhysics, a fit that does nothing) on the host clock
(the loop reads one flag per step), beside the examples' former stand-in loop (draw_action + step, no resets).  Prints
one JSON line.

    python tools/bench_il_act.py [--reps 300] [--envs 1,1024,4096] [--learn 100x4096]
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

D, A = 32, 11


def event_median(fn, reps, warmup, eng):
    """Median milliseconds of fn() between two HIP events on the engine's stream."""
    from olympic_hip._ffi import HipTimer
    tm = HipTimer()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        tm.start(eng._s())
        fn()
        tm.stop(eng._s())
        out.append(tm.elapsed_ms())
    return statistics.median(out)


def host_median(fn, reps, warmup):
    """Median milliseconds of the host's time inside fn() (the enqueue cost), nothing synchronised inside."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--envs", default="1,1024,4096")
    ap.add_argument("--learn", default="100x4096")
    args = ap.parse_args()
    if args.reps < 200:
        raise SystemExit("--reps: at least 200 repetitions per median")
    from olympic_hip import specs
    from olympic_hip.engine import Engine
    from olympic_hip.gail import DeviceStandardizer
    from olympic_hip.il_agent import DeviceGaussianPolicy
    eng = Engine(0).il_configure(specs.unitree_h1("walk"))
    torch.manual_seed(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = dict(metric="il_act", D=D, act=A, reps=args.reps)
    rng = np.random.default_rng(1)
    for N in (int(v) for v in args.envs.split(",")):
        lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, A)]
        pol = DeviceGaussianPolicy(eng, lins, DeviceStandardizer(eng, D), std_0=0.8)
        x = torch.as_tensor((rng.standard_normal((N, D)) * 2 + 1).astype(np.float32)).cuda()
        pol.act(x, generator=gen)                       # the statistics are no longer fresh: both paths accumulate
        cs, ls = pol.stand.colstats, pol.log_sigma
        mu = pol.predict(x)
        eps = torch.randn((N, A), device="cuda", generator=gen)
        action = mu + torch.exp(ls) * eps
        out = dict(action=torch.empty_like(mu), ctrl=torch.empty((N, A), device="cuda"))

        def parent():
            return eng.il_ctrl(pol.draw_action(x, generator=gen))
        calls = dict(
            act=lambda: pol.act(x, generator=gen, ctrl=True),
            parent=parent,
            # the pieces, each on its own
            il_act_call=lambda: eng.il_act(x, pol.packed, ls, cs, eps=eps, want_ctrl=True, out=out),
            il_act_no_stats=lambda: eng.il_act(x, pol.packed, ls, cs, eps=eps, update_stats=False, want_ctrl=True, out=out),
            col_stats=lambda: eng.col_stats(x, cs),
            ilmlp_forward=lambda: eng.ilmlp_forward(x, pol.packed, A, "identity", colstats=cs, y=mu),
            randn=lambda: torch.randn((N, A), dtype=torch.float32, device="cuda", generator=gen),
            exp_mul_add=lambda: mu + torch.exp(ls) * eps,
            il_ctrl=lambda: eng.il_ctrl(action, out=out["ctrl"]))
        row = {}
        for name, fn in calls.items():
            row[name + "_ms"] = event_median(fn, args.reps, args.warmup, eng)
        for name in ("act", "parent"):
            row[name + "_host_ms"] = host_median(calls[name], args.reps, args.warmup)
        row["launches"] = dict(act="randn + col_stats (2) + act_kernel (1) = 4",
                               parent="col_stats (2) + forward + randn + exp + mul + add + il_ctrl = 8")
        row["parent_over_act"] = row["parent_ms"] / row["act_ms"]
        res[f"N{N}"] = row
        print(f"# N={N}: {row}", file=sys.stderr)

    # ---- one fit's collection through ILCore.learn on the kinematic stand-in physics
    T, N = (int(v) for v in args.learn.split("x"))
    from olympic_hip.envs import LocoEnvBase
    from olympic_hip.il_core import ILCore

    class NoFit:
        def fit(self, dataset, generator=None):
            return None
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=N, seed=0)
    vec = env.vec
    lins = [torch.nn.Linear(D, 512), torch.nn.Linear(512, 256), torch.nn.Linear(256, A)]
    pol = DeviceGaussianPolicy(vec.eng, lins, DeviceStandardizer(vec.eng, D), std_0=0.8)
    core = ILCore(NoFit(), vec, pol, generator=gen)

    def wall(fn, reps=3):
        fn()
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    def stand_in():                                     # the examples' former loop: no resets, next_state = x[1:]
        xb = torch.empty((T + 1, N, D), device="cuda")
        ab = torch.empty((T, N, A), device="cuda")
        xb[0] = vec._obs.to(torch.float32)
        for t in range(T):
            ab[t] = pol.draw_action(xb[t], generator=gen)
            o, r, a, info = vec.step(ab[t])
            xb[t + 1] = o.to(torch.float32)
    learn_ms = wall(lambda: core.learn(T, T))
    resets = int(core.blocks["last"].any(1).sum())
    res[f"learn_{T}x{N}"] = dict(collection_ms=learn_ms, per_step_ms=learn_ms / T, steps_with_a_reset=resets,
                                 stand_in_loop_ms=wall(stand_in))
    print(f"# learn [{T}, {N}]: {res[f'learn_{T}x{N}']}", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
