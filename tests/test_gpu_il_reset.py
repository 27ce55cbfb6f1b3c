"""K22 on the GPU: oly_il_reset_where / VecLocoEnv.reset_where against the host-driven reset(env_mask=), bit for bit, and
ILCore's device-reset path against its host path.

Everything here is a copy or a difference of two equal float64 numbers, so every comparison is torch.equal: there is no
tolerance to choose.  The physics is ReplayPhysics over a seeded synthetic block, so that the state a reset overwrites is
not itself a trajectory sample and a row that must stay untouched can be told from one that was reset."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from test_gpu_il_act import RecordingAgent, _policy

pytestmark = pytest.mark.gpu
F32, F64, I32 = torch.float32, torch.float64, torch.int32
ROBOTS = ("h1", "h1_ff", "atlas")
BUFS = ("_cur_traj", "_cur_step", "_origin", "_sample", "_prev", "episode_steps")


class Guarded:
    """A tensor that is the interior of a larger one whose margins hold a sentinel (il_shapes.Guarded for any dtype)."""
    MARGIN = 64

    def __init__(self, shape, dtype, init=None):
        self.sentinel = -7.0e33 if dtype.is_floating_point else -77777
        n = int(np.prod(shape))
        self.big = torch.full((n + 2 * self.MARGIN,), self.sentinel, dtype=dtype, device="cuda")
        self.t = self.big[self.MARGIN:self.MARGIN + n].view(shape)
        if init is None:
            self.t.zero_()
        else:
            self.t.copy_(torch.as_tensor(init).to(device="cuda", dtype=dtype).reshape(shape))

    def intact(self):
        edge = torch.cat([self.big[:self.MARGIN], self.big[-self.MARGIN:]])
        return bool((edge == self.sentinel).all())


def guarded(shape, dtype, init=None):
    return Guarded(shape, dtype, init)


def _close(*vecs):
    torch.cuda.synchronize()
    for v in vecs:
        v.eng.ctx.close()
    gc.collect()


def make_vec(robot, N, seed=0, replay=True, horizon=None, block_seed=3, **kw):
    """The environment's VecLocoEnv; with replay a ReplayPhysics over 4 rows of the synthetic block (it wraps)."""
    from helpers import h1_synthetic_block
    from olympic_hip import specs
    from olympic_hip.envs import LocoEnvBase, ReplayPhysics
    name = "Atlas" if robot == "atlas" else "UnitreeH1"
    if robot == "h1_ff":
        kw["use_foot_forces"] = True
    if replay:
        spec = specs.atlas("walk") if robot == "atlas" else specs.unitree_h1("walk")
        T = replay if isinstance(replay, int) and not isinstance(replay, bool) else 4
        qpos, qvel, _ = h1_synthetic_block(spec, T, N, seed=block_seed, fall_frac="bench")
        kw["physics"] = ReplayPhysics(spec, torch.as_tensor(qpos).cuda(), torch.as_tensor(qvel).cuda())
    vec = LocoEnvBase.make(f"{name}.walk.real", num_envs=N, seed=seed, **kw).vec
    if horizon is not None:
        vec.spec.horizon = vec.info.horizon = horizon
    return vec


def masks_for(N, seed):
    """The issue's five masks: none set, all set, a single environment, about a third (seeded), mask=None."""
    g = np.random.default_rng(seed)
    one = np.zeros(N, bool)
    one[int(g.integers(0, N))] = True
    return dict(none=np.zeros(N, bool), all=np.ones(N, bool), one=one, third=g.uniform(size=N) < 1 / 3, null=None)


def snapshot(vec, obs):
    d = {k: getattr(vec, k).clone() for k in BUFS}
    d.update(qpos=vec.physics.qpos.clone(), qvel=vec.physics.qvel.clone(), obs=obs.clone())
    return d


# ------------------------------------------------------------------------------ 1. against the host-driven path
@pytest.mark.parametrize("N", (1, 5, 64, 257))
@pytest.mark.parametrize("robot", ROBOTS)
def test_reset_where_is_the_host_reset_bit_for_bit(robot, N):
    A, B = make_vec(robot, N), make_vec(robot, N)           # A: host path, B: device path
    try:
        J, L = A.trajectories.number_of_trajectories, A.trajectories.trajectory_length
        n_grf = int(A.spec.n_grf)
        assert n_grf == (6 if robot == "h1_ff" else 0)
        gen = torch.Generator(device="cuda").manual_seed(11 + N)
        A.reset(), B.reset()
        case = 0
        for obs_f64 in (True, False):
            A.obs_f64 = B.obs_f64 = obs_f64
            for mname, m in masks_for(N, 5 + N).items():
                case += 1
                for _ in range(2):                          # prev, episode_steps and the observation are live values
                    a = torch.randn((N, A.spec.n_act), device="cuda", generator=gen)
                    A.step(a), B.step(a)
                if n_grf:
                    # the replayed physics reports no contacts; give the ground-force columns live values by hand
                    live = torch.arange(1, N * n_grf + 1, device="cuda", dtype=B._obs.dtype).reshape(N, n_grf) / 8
                    A._obs[:, -n_grf:] = live
                    B._obs[:, -n_grf:] = live
                stepped = B._obs                            # the tensor step returned last
                pre = snapshot(B, stepped)
                assert int(pre["episode_steps"].min()) >= 2 and torch.equal(A._obs, B._obs)
                seed = 100 * N + case
                rng = np.random.default_rng(seed)           # the order reset() draws them in
                tn, st = rng.integers(0, J, N), rng.integers(0, L, N)
                A._rng = np.random.default_rng(seed)
                md = None if m is None else torch.as_tensor(m).cuda()
                oa = A.reset(env_mask=md)
                ob = B.reset_where(md, torch.as_tensor(tn.astype(np.int32)).cuda(), torch.as_tensor(st.astype(np.int32)).cuda())
                torch.cuda.synchronize()
                tag = f"{robot} N={N} f64={obs_f64} mask={mname}"
                assert ob.dtype == (F64 if obs_f64 else F32) and tuple(ob.shape) == (N, A.spec.n_obs), tag
                assert ob.data_ptr() != stepped.data_ptr() and torch.equal(stepped, pre["obs"]), tag
                assert B._obs is ob, tag
                sel = torch.ones(N, dtype=torch.bool, device="cuda") if md is None else md
                post = snapshot(B, ob)
                host = snapshot(A, oa)
                for k in post:
                    assert torch.equal(post[k][sel], host[k][sel]), (tag, k)          # reset rows: the host path's bits
                    # rows that were not reset keep their bits.  The observation is compared with its value before the
                    # call, not with the host path: reset(env_mask=) recomputes every environment's observation with
                    # fresh=True, which zeroes the ground-force columns of environments that were NOT reset; the device
                    # path must not copy that
                    assert torch.equal(post[k][~sel], pre[k][~sel]), (tag, k)
                if n_grf and bool((~sel).any()):
                    assert bool((ob[~sel][:, -n_grf:] != 0).all()), tag
                    assert bool((ob[sel][:, -n_grf:] == 0).all()), tag
                if mname in ("all", "null"):
                    assert int(B.episode_steps.abs().sum()) == 0 and torch.equal(B._cur_step.cpu(), torch.as_tensor(st, dtype=I32))
    finally:
        _close(A, B)


# ------------------------------------------------------------------------------ 2. out-of-range indices
def test_out_of_range_indices_clamp_as_traj_reset_clamps():
    N = 9
    B = make_vec("h1", N)
    try:
        J, L = B.trajectories.number_of_trajectories, B.trajectories.trajectory_length
        B.reset()
        tn = torch.tensor([-3, J, 0, J + 5, -1, 0, J - 1, 2 ** 31 - 1, -2 ** 31], dtype=I32, device="cuda")
        st = torch.tensor([L + 7, -3, L, 0, L - 1, -1, L + 7, 2 ** 31 - 1, -2 ** 31], dtype=I32, device="cuda")
        ct, cs, org, smp = B.eng.traj_reset(tn, st)
        B.reset_where(None, tn, st)
        torch.cuda.synchronize()
        assert torch.equal(B._cur_traj, ct) and torch.equal(B._cur_step, cs)
        assert torch.equal(B._origin, org) and torch.equal(B._sample, smp)
        assert int(ct.min()) == 0 and int(ct.max()) == J - 1 and int(cs.min()) == 0 and int(cs.max()) == L - 1
        sp = B.spec
        assert torch.equal(B.physics.qpos[:, B._qadr], smp[:, :sp.n_pos])
        assert torch.equal(B.physics.qvel[:, B._vadr], smp[:, sp.n_pos:sp.n_pos + sp.n_vel])
    finally:
        _close(B)


# ------------------------------------------------------------------------------ 3. no trajectory
@pytest.mark.parametrize("robot", ("h1", "h1_ff"))
def test_without_a_trajectory_the_state_rows_are_zeroed(robot):
    from helpers import h1_synthetic_block
    from olympic_hip import specs
    from olympic_hip.envs import ReplayPhysics, VecLocoEnv
    N = 70
    spec = specs.unitree_h1("walk")
    if robot == "h1_ff":
        spec.with_foot_forces("UnitreeH1")
    qpos, qvel, _ = h1_synthetic_block(spec, 2, N, seed=8)
    vec = VecLocoEnv(spec, N, physics=ReplayPhysics(spec, torch.as_tensor(qpos).cuda(), torch.as_tensor(qvel).cuda()),
                     random_start=False)
    try:
        vec.reset()
        vec.step(torch.zeros((N, spec.n_act), device="cuda"))
        stepped = vec._obs
        pre = dict(qpos=vec.physics.qpos.clone(), qvel=vec.physics.qvel.clone(), prev=vec._prev.clone(),
                   steps=vec.episode_steps.clone(), obs=stepped.clone())
        assert bool((pre["obs"][:, :spec.n_obs - spec.n_grf] != 0).any(1).all()) and bool((pre["prev"] != 0).all())
        m = torch.as_tensor(np.random.default_rng(4).uniform(size=N) < 0.4).cuda()
        assert 0 < int(m.sum()) < N
        ob = vec.reset_where(m)
        torch.cuda.synchronize()
        assert torch.equal(stepped, pre["obs"])
        for k, t in (("qpos", vec.physics.qpos), ("qvel", vec.physics.qvel), ("prev", vec._prev), ("obs", ob)):
            assert int(t[m].count_nonzero()) == 0, k                  # the zero state and its observation
            assert torch.equal(t[~m], pre[k][~m]), k
        assert int(vec.episode_steps[m].abs().sum()) == 0 and torch.equal(vec.episode_steps[~m], pre["steps"][~m])
        with pytest.raises(Exception):
            vec.reset_where(m, traj_no=torch.zeros(N, dtype=I32, device="cuda"), step=torch.zeros(N, dtype=I32, device="cuda"))
        with pytest.raises(ValueError, match="Random start"):
            VecLocoEnv(spec, N, engine=vec.eng, random_start=True).reset_where(m)
    finally:
        _close(vec)


# ------------------------------------------------------------------------------ 4. / 5. the engine call
def engine_case(vec, N, seed=2):
    """Valid arguments of Engine.il_reset_where for the environment's configured engine, in guarded buffers."""
    sp = vec.spec
    K = vec.eng.traj_shape[0]
    J, L = vec.trajectories.number_of_trajectories, vec.trajectories.trajectory_length
    g = np.random.default_rng(seed)
    G = dict(qpos=guarded((N, sp.nq), F64, init=g.standard_normal((N, sp.nq))),
             qvel=guarded((N, sp.nv), F64, init=g.standard_normal((N, sp.nv))),
             obs_in=guarded((N, sp.n_obs), F32, init=g.standard_normal((N, sp.n_obs))),
             obs_out=guarded((N, sp.n_obs), F32),
             prev=guarded((N,), F64, init=g.standard_normal(N)),
             episode_steps=guarded((N,), I32, init=g.integers(1, 9, N)),
             cur_traj=guarded((N,), I32, init=np.full(N, -5)), cur_step=guarded((N,), I32, init=np.full(N, -5)),
             origin=guarded((N, 2), F64, init=g.standard_normal((N, 2))),
             sample=guarded((N, K), F64, init=g.standard_normal((N, K))))
    args = {k: v.t for k, v in G.items()}
    args["mask"] = torch.as_tensor(g.uniform(size=N) < 0.5).cuda()
    args["traj_no"] = torch.as_tensor(g.integers(0, J, N).astype(np.int32)).cuda()
    args["step"] = torch.as_tensor(g.integers(0, L, N).astype(np.int32)).cuda()
    return G, args


def test_obs_in_may_be_obs_out():
    N = 131
    vec = make_vec("h1", N, replay=False)
    try:
        G1, a1 = engine_case(vec, N)
        G2, a2 = engine_case(vec, N)
        a2["obs_out"] = a2["obs_in"]                                    # in place
        before = a1["obs_in"].clone()
        o1 = vec.eng.il_reset_where(**a1)
        o2 = vec.eng.il_reset_where(**a2)
        torch.cuda.synchronize()
        assert o2 is a2["obs_in"] and torch.equal(o1, o2)
        m = a1["mask"]
        assert 0 < int(m.sum()) < N and torch.equal(o1[~m], before[~m]) and not torch.equal(o1[m], before[m])
        assert torch.equal(a1["obs_in"], before)                        # the separate input is only read
        for k in G1:
            assert G1[k].intact() and G2[k].intact(), k                 # nothing written outside any buffer
            if k not in ("obs_in", "obs_out"):
                assert torch.equal(G1[k].t, G2[k].t), k
        # uint8 masks are the same bytes
        G3, a3 = engine_case(vec, N)
        a3["mask"] = a3["mask"].to(torch.uint8)
        assert torch.equal(vec.eng.il_reset_where(**a3), o1)
    finally:
        _close(vec)


def test_refusals_leave_the_context_usable():
    from olympic_hip import _abi, specs
    from olympic_hip._ffi import OlyError, ptr
    from olympic_hip.engine import Engine
    from olympic_hip.envs import KinematicPhysics, LocoEnvBase
    N = 6
    vec = make_vec("h1", N, replay=False)
    bare = Engine(0)
    try:
        eng = vec.eng
        G, args = engine_case(vec, N)
        want = eng.il_reset_where(**args).clone()

        def ok():
            """A valid call on the same context still runs and gives the same rows."""
            args["obs_out"].zero_()
            assert torch.equal(eng.il_reset_where(**args), want)
            torch.cuda.synchronize()
            assert all(g.intact() for g in G.values())

        def raw(e, **over):
            """Straight at the C entry point."""
            qs, vs = eng.il_reset_tables()
            p = dict(n=N, out_flags=0, qpos_slot=qs.data_ptr(), qvel_slot=vs.data_ptr(),
                     **{k: v.data_ptr() for k, v in args.items()})
            p.update(over)
            e.ctx.call("oly_il_reset_where", C.byref(_abi.ILReset(**p)), e._s())

        raw(eng)                                                        # the raw form itself is valid
        ok()
        # ---- no configured model; indices without a table
        with pytest.raises(OlyError, match="il_configure"):
            bare.il_reset_where(**args)
        with pytest.raises(OlyError, match="oly_il_configure"):
            raw(bare)
        bare.il_configure(specs.unitree_h1("walk"))
        with pytest.raises(OlyError, match="traj_upload"):
            bare.il_reset_where(**args)
        with pytest.raises(OlyError, match="oly_traj_upload"):
            raw(bare)
        no_traj = {k: v for k, v in args.items() if k not in ("traj_no", "step", "cur_traj", "cur_step", "origin", "sample")}
        bare.il_reset_where(**no_traj)                                  # without indices the same context runs
        torch.cuda.synchronize()
        assert int(args["qpos"][args["mask"]].count_nonzero()) == 0
        eng.il_reset_where(**args)
        ok()
        # ---- a table with fewer keys than n_pos + n_vel
        bare.traj_upload(np.zeros((5, 2, 3)))
        with pytest.raises(OlyError, match="keys"):
            raw(bare)
        with pytest.raises(OlyError, match="keys"):
            bare.il_reset_where(**dict(args, sample=torch.zeros((N, 5), dtype=F64, device="cuda")))
        # ---- n < 0; n == 0 launches nothing
        with pytest.raises(OlyError):
            raw(eng, n=-1)
        raw(eng, n=0)
        ok()
        # ---- a NULL among the required pointers, at the C entry point and through the engine
        required = ("step", "cur_traj", "cur_step", "origin", "sample", "qpos", "qvel", "qpos_slot", "qvel_slot", "obs_in",
                    "obs_out", "prev", "episode_steps")
        for k in required:
            with pytest.raises(OlyError, match="NULL|prev required"):
                raw(eng, **{k: None})
            ok()
            if k not in ("qpos_slot", "qvel_slot"):
                with pytest.raises(OlyError):
                    eng.il_reset_where(**dict(args, **{k: None}))
                ok()
        # ---- wrong dtype / shape / stride / device for each argument
        for k, t in args.items():
            wrong_dtype = t.to(F32 if t.dtype in (F64, I32, torch.bool) else F64)
            if k == "obs_in":
                wrong_dtype = t.to(torch.float16)
            wrong_shape = torch.zeros((N + 1,) + tuple(t.shape[1:]), dtype=t.dtype, device="cuda")
            wide = torch.zeros((N,) + ((2 * t.shape[1],) if t.dim() == 2 else (2,)), dtype=t.dtype, device="cuda")
            strided = wide[:, ::2] if t.dim() == 2 else wide[:, 0]
            assert tuple(strided.shape) == tuple(t.shape) and not strided.is_contiguous()
            for bad in (wrong_dtype, wrong_shape, strided, t.cpu()):
                with pytest.raises(OlyError):
                    eng.il_reset_where(**dict(args, **{k: bad}))
                ok()
        # ---- a physics whose state is not on the device
        class HostState(KinematicPhysics):
            device_state = False
        phys = HostState(specs.unitree_h1("walk"), N, torch.device("cuda", 0))
        env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=N, seed=1, physics=phys, device=0).vec
        try:
            env.reset()
            with pytest.raises(OlyError, match="device_state"):
                env.reset_where(None)
            from olympic_hip.il_core import ILCore
            with pytest.raises(OlyError, match="device_state"):
                ILCore(RecordingAgent(), env, None, device_reset=True)
            assert ILCore(RecordingAgent(), env, None).device_reset is False
        finally:
            _close(env)
        ok()
    finally:
        _close(vec)
        bare.ctx.close()


# ------------------------------------------------------------------------------ 6. no hidden synchronisation
def _sync_debug_mode_works():
    """Whether this torch build reports a synchronising call under set_sync_debug_mode("error")."""
    x = torch.ones(1, device="cuda")
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(old)
    return False


def test_no_hidden_synchronisation():
    from olympic_hip.il_core import ILCore
    if not _sync_debug_mode_works():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not report a synchronising call in this torch build")
    N = 64
    vec = make_vec("h1", N, horizon=1)
    try:
        pol = _policy(vec.eng, vec.spec.n_obs, vec.spec.n_act, 5)
        gen = torch.Generator(device="cuda").manual_seed(2)
        core = ILCore(RecordingAgent(), vec, pol, generator=gen, device_reset=True)
        obs = vec.reset()
        obs = core._step(obs, False)[-1]                                # warm-up: first launches, the policy's start
        mask = torch.as_tensor(np.arange(N) % 3 == 0).cuda()
        torch.cuda.synchronize()
        old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            obs = vec.reset_where(mask)                                 # drawn indices, the launch
            out = core._step(obs, False)                                # act, step, reset_where: horizon 1 ends every episode
        finally:
            torch.cuda.set_sync_debug_mode(old)
        torch.cuda.synchronize()
        assert bool(out[3].all()) and int(vec.episode_steps.abs().sum()) == 0
    finally:
        _close(vec)


# ------------------------------------------------------------------------------ 7. ILCore.learn, device against host
def test_learn_device_path_equals_host_path():
    from olympic_hip.il_core import ILCore
    N, H, T = 37, 5, 12
    runs = {}
    vecs = []
    try:
        for device_reset in (False, True):
            # init_step_no fixed and random_start off: neither path consumes random numbers for a reset
            vec = make_vec("h1", N, replay=T, horizon=H, block_seed=21, random_start=False, init_step_no=23)
            vecs.append(vec)
            pol = _policy(vec.eng, vec.spec.n_obs, vec.spec.n_act, 5)
            agent = RecordingAgent()
            core = ILCore(agent, vec, pol, generator=torch.Generator(device="cuda").manual_seed(2), device_reset=device_reset)
            assert core.device_reset is device_reset
            assert core.learn(T, T) == [1]
            torch.cuda.synchronize()
            runs[device_reset] = (agent.fits[0], core.blocks["last"].clone(), {k: getattr(vec, k).clone() for k in BUFS},
                                  vec.physics.qb.clone())
        (host, hl, hb, hq), (dev, dl, db, dq) = runs[False], runs[True]
        assert set(dev) == {"state", "action", "reward", "next_state", "absorbing", "last"}
        for k in dev:
            assert torch.equal(dev[k], host[k]), k
        assert torch.equal(dl, hl) and torch.equal(dq, hq)
        for k in BUFS:
            assert torch.equal(db[k], hb[k]), k
        last = dl
        for t in (H - 1, 2 * H - 1):                                    # steps 5 and 10
            assert int(last[t].sum()) >= 2, t
        assert bool(dev["absorbing"].any()) and bool((last & ~dev["absorbing"]).any())
        fixed = dev["state"][0]                                         # the full reset: every row is the fixed sample
        assert bool((fixed == fixed[0]).all()) and int(fixed[0].count_nonzero()) > 0
        s, nx, m = dev["state"], dev["next_state"], last[:-1]
        assert torch.equal(s[1:][m], fixed[None].expand(T - 1, N, -1)[m])      # state[t+1] of a reset environment
        assert torch.equal(s[1:][~m], nx[:-1][~m])
        assert not bool((nx[:-1][m] == fixed[None].expand(T - 1, N, -1)[m]).all(1).any())   # next_state[t]: pre-reset
        # the pre-reset observation is the replayed block's row, whichever path ran
        ref = vecs[1].eng.il_step(hq_rows(vecs[1], T, N, "q"), hq_rows(vecs[1], T, N, "v"), None,
                                  torch.zeros(N, dtype=F64, device="cuda"))["obs"]
        assert torch.equal(nx, ref)
    finally:
        _close(*vecs)


def hq_rows(vec, T, N, which):
    """The block the ReplayPhysics was built on (regenerated: the resets wrote into the live one)."""
    from helpers import h1_synthetic_block
    qpos, qvel, _ = h1_synthetic_block(vec.spec, T, N, seed=21, fall_frac="bench")
    return torch.as_tensor(qpos if which == "q" else qvel).cuda()


# ------------------------------------------------------------------------------ 8. ILCore.evaluate on the device path
def test_evaluate_on_the_device_path():
    from olympic_hip.il_core import ILCore
    N, H = 3, 4
    vec = make_vec("h1", N, replay=False, horizon=H, random_start=False, init_step_no=7)
    try:
        outs = {}
        for poll in (1, 32):
            pol = _policy(vec.eng, vec.spec.n_obs, vec.spec.n_act, 9)
            core = ILCore(RecordingAgent(), vec, pol, generator=torch.Generator(device="cuda").manual_seed(3))
            assert core.device_reset is True
            outs[poll], b = core.evaluate(7, poll=poll, return_blocks=True)
            assert b["last"].sum(0).tolist() == [3, 2, 2] and int(b["last"].sum()) == 7      # the completed count
        o = outs[1]
        assert o == outs[32]
        assert o["n_episodes"] == 7 and o["L"] == H and o["n_steps"] == 7 * H    # nothing falls on the held sample
    finally:
        _close(vec)


# ------------------------------------------------------------------------------ 9. random starts
def test_random_starts_are_in_range_and_seeded():
    N = 4096
    vec = make_vec("h1", N, replay=False)
    try:
        J, L = vec.trajectories.number_of_trajectories, vec.trajectories.trajectory_length
        vec.reset()
        draws = []
        for seed in (5, 5, 6):
            g = torch.Generator(device="cuda").manual_seed(seed)
            ob = vec.reset_where(torch.ones(N, dtype=torch.bool, device="cuda"), generator=g)
            ct, cs = vec._cur_traj.clone(), vec._cur_step.clone()
            assert 0 <= int(ct.min()) and int(ct.max()) < J and 0 <= int(cs.min()) and int(cs.max()) < L
            assert int(cs.max()) > L // 2 and (J == 1 or int(ct.max()) > 0)       # spread over the table
            _, _, org, smp = vec.eng.traj_reset(ct, cs)
            assert torch.equal(vec._sample, smp) and torch.equal(vec._origin, org)
            draws.append((ct, cs, ob.clone()))
        assert all(torch.equal(a, b) for a, b in zip(draws[0], draws[1]))
        assert not torch.equal(draws[0][1], draws[2][1])
        # the environment's own device generator: seeded by `seed`, so two environments built alike agree
        other = make_vec("h1", N, replay=False)
        try:
            other.reset()
            a, b = vec.reset_where(None), other.reset_where(None)
            assert torch.equal(vec._cur_step, other._cur_step) and torch.equal(vec._cur_traj, other._cur_traj)
            assert torch.equal(a, b)
        finally:
            _close(other)
    finally:
        _close(vec)
