"""K23 on the GPU: oly_a3_reset_draw against its numpy restatement (tests/a3_reset_draw_restate.py) byte for byte, and
A3DeviceRollout(draw="device") through the three rollout paths, a rollout that resets on every step, and a PPO resume.

Every comparison is of bytes or torch.equal: the kernel and the restatement do the same float64 operations in the same
order (the library is built with -ffp-contract=off), so there is no tolerance to choose."""
import ctypes as C

import numpy as np
import pytest
import torch

import a3_reset_draw_restate as R
from olympic_hip import _abi, specs
from olympic_hip._ffi import OlyError
from olympic_hip.synthetic import A3_FLOOR_BODY, A3_GEOM_BODYID, A3_LFOOT_BODY, A3_RFOOT_BODY, a3_synthetic_blocks
from olympic_hip.vecstep import REC

pytestmark = pytest.mark.gpu
CONTACT = (A3_GEOM_BODYID, A3_FLOOR_BODY, A3_RFOOT_BODY, A3_LFOOT_BODY)
SEED = 0xC0FFEE1234567891
PERIOD = 88
ISZ = REC.itemsize
BASES = np.array([0, 5, 2 ** 32 - 1, 2 ** 32 + 7], dtype=np.int64)      # the last two reach the counter's high word
ITERATIONS = (0, 3000, 7000, 20000)                                      # h = 0, 0, 0.05, 0.1
_BLOCKS = {}


@pytest.fixture(scope="module")
def eng():
    from olympic_hip.engine import Engine
    return Engine(0)


def make_env(n, rs_seed, **kw):
    from olympic_hip.a3 import ReplayA3Physics, VecA3Env
    from olympic_hip.engine import Engine
    if n not in _BLOCKS:                                    # the readback is data, the same for every run
        host = a3_synthetic_blocks(n, 5, seed=4, C=16, p_bad=0.03, p_low=0.01)
        _BLOCKS[n] = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    env = VecA3Env(specs.A3Spec(mass=41.5), n, Engine(0), ReplayA3Physics(dict(_BLOCKS[n])), *CONTACT,
                   rs=np.random.RandomState(rs_seed), **kw)
    env.device = env.eng.device
    return env


def networks(seed=5):
    from olympic_hip.ppo import MLPCritic, MLPGaussianActor
    torch.manual_seed(seed)
    return MLPGaussianActor(41, 12).cuda(), MLPCritic(41).cuda()


def ring_of(roll):
    return roll.pool.cpu().numpy().view(REC).reshape(roll.N, roll.depth)


# ------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("depth", [1, 4, 33])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_kernel_equals_the_restatement(eng, N, depth):
    size = N * depth * ISZ
    base0 = BASES[np.arange(N) % 4]
    consumed = ((np.arange(N) * 7) % 5 + (np.arange(N) == 0)).astype(np.int32)      # non-zero somewhere for every N
    for it in ITERATIONS:
        h = R.step_height(it)
        big = torch.full((size + 2 * ISZ,), 0xAB, dtype=torch.uint8, device="cuda")   # one guard record on either side
        pool = big[ISZ:ISZ + size]
        base = torch.as_tensor(base0).cuda()
        # pool_count NULL: base as it is
        eng.a3_reset_draw(pool, base, None, depth, SEED, h, PERIOD)
        assert np.array_equal(base.cpu().numpy(), base0)
        want = R.ring(SEED, base0, depth, PERIOD, h)
        assert pool.cpu().numpy().tobytes() == want.tobytes(), (it, "NULL pool_count")
        # consumed records: base advanced, the cursors rewound, the ring moved on
        count = torch.as_tensor(consumed).cuda()
        eng.a3_reset_draw(pool, base, count, depth, SEED, h, PERIOD)
        base1 = base0 + consumed
        assert np.array_equal(base.cpu().numpy(), base1) and not count.any()
        want = R.ring(SEED, base1, depth, PERIOD, h)
        assert pool.cpu().numpy().tobytes() == want.tobytes(), (it, "advanced")
        # nothing consumed: the same bytes again
        pool.fill_(0xCD)
        eng.a3_reset_draw(pool, base, count, depth, SEED, h, PERIOD)
        assert np.array_equal(base.cpu().numpy(), base1) and not count.any()
        assert pool.cpu().numpy().tobytes() == want.tobytes(), (it, "second call")
        assert bool((big[:ISZ] == 0xAB).all()) and bool((big[ISZ + size:] == 0xAB).all())
    rec = want.reshape(-1)
    assert N * depth < 33 or (len(np.unique(rec["mode"])) == 2 and rec["seq"][:, 19, 2].any())    # the case holds both modes


def test_argument_refusals(eng):
    N, depth = 4, 2
    pool = torch.zeros(N * depth * ISZ + 8, dtype=torch.uint8, device="cuda")
    base = torch.zeros(N, dtype=torch.int64, device="cuda")
    count = torch.zeros(N, dtype=torch.int32, device="cuda")
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(pool_p, n, d, base_p, h=0.0, period=PERIOD):
        eng.ctx.call("oly_a3_reset_draw", pool_p, n, d, SEED, base_p, vp(count), h, period, eng._s())
    call(vp(pool), N, depth, vp(base))                                   # the well-formed call is accepted
    for args in ((None, N, depth, vp(base)), (vp(pool), N, depth, None), (vp(pool), 0, depth, vp(base)),
                 (vp(pool), -1, depth, vp(base)), (vp(pool), N, 0, vp(base)), (vp(pool, 4), N, depth, vp(base)),
                 (vp(pool), N, depth, vp(base), -0.1), (vp(pool), N, depth, vp(base), float("nan"))):
        with pytest.raises(OlyError, match="oly_a3_reset_draw"):
            call(*args)
    # the typed front end refuses before the library is reached
    good = pool[:N * depth * ISZ]
    with pytest.raises(OlyError, match="pool"):
        eng.a3_reset_draw(pool, base, count, depth, SEED, 0.0, PERIOD)   # eight bytes too many
    with pytest.raises(OlyError, match="base"):
        eng.a3_reset_draw(good, base.to(torch.int32), count, depth, SEED, 0.0, PERIOD)
    with pytest.raises(OlyError, match="pool_count"):
        eng.a3_reset_draw(good, base, count.to(torch.int64), depth, SEED, 0.0, PERIOD)
    with pytest.raises(OlyError, match="seed"):
        eng.a3_reset_draw(good, base, count, depth, 2 ** 64, 0.0, PERIOD)
    torch.cuda.synchronize()
    assert not base.any() and not count.any()


# ------------------------------------------------------------------------------ no record is used twice
def test_a_rollout_sized_ring_never_reuses_a_record():
    """max_traj_len = 1: every step cuts, so every environment resets T = 12 times per rollout: env.reset() of all, then once
    per cut but the last step's (the next rollout opens with env.reset() again)."""
    N, T = 48, 12
    pi, vf = networks()
    host = make_env(N, 3)
    host.device_rollout(pi, vf, T, 1, graph=False)
    info = host._dev_rollout.last_info
    assert host._dev_rollout.depth == 4 and info["resets"] == N * T
    assert info["reused_records"] == N * (T - 4) > 0                 # the stated deviation of the host path
    env = make_env(N, 3, reset_draw="device", reset_seed=SEED, reset_pool_depth="rollout")
    env.iteration_count = 7000                                           # h = 0.05
    for nth in (1, 2):
        env.device_rollout(pi, vf, T, 1, graph=False)
        roll = env._dev_rollout
        assert roll.depth == T + 1 and roll.pool.numel() == N * (T + 1) * ISZ
        assert roll.last_info["resets"] == N * T and roll.last_info["reused_records"] == 0
        resets = nth * T                                                 # per environment, for the life of the run
        assert torch.equal(roll.base.cpu(), torch.full((N,), resets, dtype=torch.int64)) and not roll.pool_count.any()
        assert ring_of(roll).tobytes() == R.ring(SEED, np.full(N, resets), T + 1, PERIOD, 0.05).tobytes()
        # the task state is the last reset's record, stepped once since (the last step cuts without a reset)
        last = R.records(SEED, np.arange(N), np.full(N, resets - 1), PERIOD, 0.05)
        for k in ("mode", "seq_len"):
            assert np.array_equal(env.state[k].cpu().numpy(), last[k]), (nth, k)
        assert np.array_equal(env.state["phase"].cpu().numpy(), (last["phase"] + 1) % PERIOD), nth
    assert len(np.unique(last["mode"])) == 2 and len(np.unique(last["phase"])) == 2
    # a ring sized by the rollout belongs to the device mode alone
    with pytest.raises(OlyError, match="needs draw='device'"):
        make_env(N, 3, reset_pool_depth="rollout")._make_device_rollout()


def test_default_depths():
    dev_env, host_env = make_env(20, 3, reset_draw="device"), make_env(20, 3)
    dev_env._make_device_rollout(), host_env._make_device_rollout()
    d, h = dev_env._dev_rollout, host_env._dev_rollout
    assert (d.depth, d.draw, h.depth, h.draw) == (32, "device", 4, "host")
    assert not hasattr(d, "_stash_t") and 0 <= d.seed < 2 ** 63
    assert ring_of(d).tobytes() == R.ring(d.seed, np.zeros(20, np.int64), 32, PERIOD, 0.0).tobytes()


# ------------------------------------------------------------------------------ the three rollout paths
@pytest.mark.parametrize("N", [100, 1, 17])
def test_rollout_paths_agree_in_device_mode(N):
    T, max_len = 11, 4
    pi, vf = networks()
    out = []
    for graph, persistent in ((False, False), (True, False), (False, True)):
        env = make_env(N, 3, reset_draw="device", reset_seed=SEED, reset_pool_depth=5)
        env.iteration_count = 20000
        snaps = []
        for it in range(2):
            torch.manual_seed(11 + it)                                   # the action noise block
            env.device_rollout(pi, vf, T, max_len, anneal=0.7, graph=graph, persistent=persistent)
            r = env._dev_rollout
            named = dict(states=r.buf.states, actions=r.buf.actions, rewards=r.buf.rewards, values=r.buf.values,
                         next_values=r.buf.next_values, flags=r.buf.flags, state_obs=r.state_obs, traj_len=r.traj_len,
                         pool_count=r.pool_count, base=r.base, pool=r.pool)
            named.update({"st_" + k: v for k, v in env.state.items()})
            snaps.append(({k: v.clone() for k, v in named.items()}, dict(r.last_info)))
        out.append(snaps)
        env._dev_rollout.close()
    for other in out[1:]:
        for (a, ia), (b, ib) in zip(out[0], other):
            for name in a:
                assert a[name].dtype == b[name].dtype and torch.equal(a[name], b[name]), name
            assert ia == ib
    (first, info1), (second, info2) = out[0]
    assert info1["resets"] > N and info2["resets"] > N                    # env.reset() of all, then device-side resets
    assert int(first["base"].sum()) == info1["resets"] and int(second["base"].sum()) == info1["resets"] + info2["resets"]
    want = R.ring(SEED, second["base"].cpu().numpy(), 5, PERIOD, 0.1)
    assert second["pool"].cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------------------ checkpoints
def make_run(path, seed, n=32, **env_kw):
    from olympic_hip.ppo import PPO, MLPCritic, MLPGaussianActor
    args = dict(gamma=0.99, lam=0.95, lr=1e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=64, epochs=2,
                max_traj_len=8, use_gae=False, num_procs=n, max_grad_norm=0.05, mirror_coeff=0.0, eval_freq=2)
    ppo = PPO(args, str(path))
    torch.manual_seed(seed)
    pi, vf = MLPGaussianActor(41, 12).cuda(), MLPCritic(41).cuda()
    env = make_env(n, seed, **env_kw)
    torch.manual_seed(1000 + seed)
    return ppo, env, pi, vf


def end_state(ppo, env, hist):
    from olympic_hip import ppo_checkpoint as ck
    d = ck.to_host(dict(policy=ck.module_state(ppo.policy), critic=ck.module_state(ppo.critic),
                        optimiser=ck.optimiser_state(ppo), env=env.state_dict(), physics_k=int(env.physics.k),
                        ring=env._dev_rollout.pool.clone(),
                        history=[[h["itr"], h["losses"], h["ep_return"], h["ep_len"]] for h in hist]))
    torch.cuda.synchronize()
    return d


def test_resume_in_device_mode(tmp_path):
    from olympic_hip import ppo_checkpoint as ck
    from test_gpu_ppo_checkpoint import first_difference, leaves
    ends = []
    for name, kw in (("A", {}), ("A2", dict(checkpoint_every=2))):
        ppo, env, pi, vf = make_run(tmp_path / name, 4, reset_draw="device")      # the seed is one draw from the env's stream
        hist = ppo.train(lambda: env, pi, vf, n_itr=3, verbose=False, **kw)
        ends.append(end_state(ppo, env, hist))
    a, a2 = ends
    assert first_difference(a, a2) is None, "two runs from the same seeds differ: not a resume failure"
    assert [h[0] for h in a["history"]] == [0, 1, 2]
    roll = a["env"]["device_rollout"]
    assert roll["draw"] == "device" and roll["pool_depth"] == 32 and int(roll["tensors"]["base"].sum()) >= 3 * 32
    path = str(tmp_path / "A2" / "checkpoint.pt")
    mid = ck.read(path)
    assert mid["ppo"]["iteration"] == 1
    stored = mid["env"]["device_rollout"]
    assert stored["draw"] == "device" and stored["seed"] == roll["seed"] and not stored["tensors"]["pool_count"].any()
    names = [p for p, _ in leaves(mid)]
    assert not [p for p in names if p.split("/")[-1] in ("pool", "stash")] and any(p.endswith("/tensors/base") for p in names)
    # B: fresh objects from another seed (another reset seed too)
    ppo, env, pi, vf = make_run(tmp_path / "B", 11, reset_draw="device")
    env._make_device_rollout()
    assert env._dev_rollout.seed != roll["seed"]
    hist = ppo.train(lambda: env, pi, vf, n_itr=3, verbose=False, resume=path)
    assert [h["itr"] for h in hist] == [2]
    diff = first_difference(dict(a, history=a["history"][2:]), end_state(ppo, env, hist))
    assert diff is None, f"the resumed run first differs from the uninterrupted one in {diff}"
    r = env._dev_rollout
    assert r.seed == roll["seed"] and torch.equal(r.base.cpu(), roll["tensors"]["base"])
    assert ring_of(r).tobytes() == R.ring(r.seed, r.base.cpu().numpy(), 32, PERIOD, 0.0).tobytes()
    # one mode's file into the other mode: refused before the first write
    host_env = make_env(32, 5)
    before = {k: v.clone() for k, v in host_env.state.items()}
    with pytest.raises(OlyError, match="draw is 'device' in the stored state, 'host' in this object"):
        host_env.load_state_dict(mid["env"])
    assert all(torch.equal(before[k], v) for k, v in host_env.state.items()) and host_env.iteration_count == 0
    host_file = ck.to_host(host_env.state_dict())
    dev_env = make_env(32, 5, reset_draw="device")
    with pytest.raises(OlyError, match="draw is 'host' in the stored state, 'device' in this object"):
        dev_env.load_state_dict(host_file)
    assert not dev_env._dev_rollout.base.any()


def test_host_mode_state_dict_keeps_its_keys():
    env = make_env(20, 3)
    env._make_device_rollout()
    d = env._dev_rollout.state_dict()
    assert sorted(d) == sorted(["num_envs", "pool_depth", "tensors", "stash", "stash_n", "stash_i", "last_total", "physics_k",
                                "iteration_count", "rs"])
    task = [f"task.{k}" for k in _abi.A3_STATE_FIELDS]
    assert sorted(d["tensors"]) == sorted(task + ["state_obs", "traj_len", "pool_count", "ctr", "pd_target", "pool"])
    assert d["pool_depth"] == 4 and d["tensors"]["pool"].numel() == 20 * 4 * ISZ
    dev = make_env(20, 3, reset_draw="device", reset_pool_depth=2)
    dev._make_device_rollout()
    d = dev._dev_rollout.state_dict()
    assert sorted(d) == sorted(["num_envs", "pool_depth", "draw", "seed", "step_height_abs", "tensors", "physics_k",
                                "iteration_count"])
    assert sorted(d["tensors"]) == sorted(task + ["state_obs", "traj_len", "pool_count", "ctr", "pd_target", "base"])
