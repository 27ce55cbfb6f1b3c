"""Checkpoint and resume of the imitation-learning loop on the GPU: every object's state_dict / load_state_dict, the file
format and BestAgentSaver's snapshot, held to the statement K15-K22 all make ("no atomics: two runs give identical bits").

Every comparison is torch.equal on the same computation run twice, so there is no tolerance to choose.  The agents are
built as examples/il_experiment.py:build_agent builds them, on UnitreeH1.walk with the kinematic stand-in: 64
environments, 8 vec steps per fit (512 rows: two critic minibatches of 256, one discriminator minibatch), the horizon cut
to 5 so that episodes end and are reset inside every window."""
import gc
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
N, T, H = 64, 8, 5


class Recorder:
    """The writer of an agent with diagnostics: what add_scalar was given, in order."""

    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


def build(algo, seed, device_reset=None, log=False, n=N):
    """(agent, core, vec) from one seed: the networks' initial weights (torch's global generator), the environment's
    two reset streams and the loop's generator all follow from it."""
    if EXAMPLES not in sys.path:
        sys.path.insert(0, EXAMPLES)
    from il_experiment import build_agent
    from olympic_hip.envs import LocoEnvBase
    from olympic_hip.il_core import ILCore
    torch.manual_seed(seed)
    env = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=n, seed=seed)
    vec = env.vec
    vec.spec.horizon = vec.info.horizon = H
    agent, policy = build_agent(algo, env, log, sw=Recorder() if log else None)
    gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
    core = ILCore(agent, vec, policy, generator=gen, device_reset=device_reset)
    return agent, core, vec


def close(*vecs):
    torch.cuda.synchronize()
    for v in vecs:
        v.eng.ctx.close()
    gc.collect()


def tensors(nest, prefix=""):
    """The (path, tensor) leaves of a nest, and the (path, value) of everything else."""
    if torch.is_tensor(nest):
        yield prefix, nest
    elif isinstance(nest, dict):
        for k, v in nest.items():
            yield from tensors(v, f"{prefix}/{k}")
    elif isinstance(nest, (list, tuple)):
        for i, v in enumerate(nest):
            yield from tensors(v, f"{prefix}/{i}")
    else:
        yield prefix, nest


def assert_same(a, b, what):
    """Two nests agree: the same paths, tensors bit-equal (NaN equal to NaN: EpLenMean may be one), the rest ==."""
    la, lb = list(tensors(a)), list(tensors(b))
    assert [p for p, _ in la] == [p for p, _ in lb], what
    n = 0
    for (p, x), (_, y) in zip(la, lb):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape, (what, p)
            assert torch.equal(x.cpu().reshape(-1).view(torch.uint8), y.cpu().reshape(-1).view(torch.uint8)), (what, p)
            n += 1
        elif isinstance(x, float) and x != x:
            assert y != y, (what, p)
        else:
            assert type(x) is type(y) and x == y, (what, p, x, y)
    return n


def fit_tensors(out):
    return {k: out[k] for k in ("reward", "v_target", "adv", "critic_loss", "disc_loss", "disc_trained", "disc_log", "iter_log")
            if k in out}


def pointers(agent):
    pol = agent.policy_step.policy
    d = dict(param=agent.critic.param, critic_packed=agent.critic.packed, theta=pol.theta, policy_packed=pol.packed,
             colstats=agent.critic.stand.colstats, disc_colstats=agent.disc.stand.colstats,
             disc_packed=agent.disc._packed, exp_avg=agent.disc_trainer.exp_avg)
    d.update({f"disc_param{i}": p for i, p in enumerate(agent.disc._params())})
    return {k: v.data_ptr() for k, v in d.items()}


# ------------------------------------------------------------------------------ a. component round trip
@pytest.mark.parametrize("algo", ("gail", "vail"))
def test_component_round_trip(algo, tmp_path):
    from olympic_hip import il_checkpoint as ck
    a1, c1, v1 = build(algo, 0)
    a2, c2, v2 = build(algo, 7)
    try:
        assert len(c1.learn(3 * T, T)) == 3 and a1.iter == 4
        c2.learn(T, T)                                       # the second agent has a past of its own, and live buffers
        path = ck.save(str(tmp_path / "a.pt"), a1, c1, epoch=0)
        before = pointers(a2)
        assert all(before.values())
        with pytest.raises(Exception):                       # the two really differ before the load
            assert_same(a1.state_dict(), a2.state_dict(), "agents")
        assert ck.load(path, a2, c2) == dict(epoch=0)
        sa, sb = a1.state_dict(), a2.state_dict()
        assert assert_same(sa, sb, "agent state") >= 12
        assert assert_same(c1.state_dict(), c2.state_dict(), "core state") >= 10
        assert sb["iter"] == 4 and sb["header"]["kind"] == algo and sb["critic"]["step"] == 3 * 3 * 2
        assert sb["disc_trainer"]["step"] == 1               # fit 3 trained the discriminator: one minibatch
        assert pointers(a2) == before                        # written in place
        with pytest.raises(Exception, match="no step has run"):
            a2.policy_step.old_distribution()
        g = torch.Generator(device="cuda").manual_seed(5)
        probe = v1.reset().to(torch.float32) + 0.01 * torch.randn((N, v1.spec.n_obs), device="cuda", generator=g)
        eps = torch.randn((N, 128), device="cuda", generator=g)
        for name, f in (("policy", lambda a: a.policy_step.policy.predict(probe)),
                        ("critic", lambda a: a.critic.predict(probe)),
                        ("reward", lambda a: a.disc(probe, eps))):
            x, y = f(a1), f(a2)
            assert x.shape[0] == N and torch.equal(x, y), name
            assert bool(torch.isfinite(x).all()) and float(x.std()) > 0, name
        # the thin methods; an agent-only file
        a1.save(str(tmp_path / "b.pt"), note="x")
        assert a2.load(str(tmp_path / "b.pt")) == dict(note="x")
        assert_same(a1.state_dict(), a2.state_dict(), "agent state, thin methods")
        # the other kind of agent refuses the file, naming the field
        from olympic_hip._ffi import OlyError
        a3, _, v3 = build("vail" if algo == "gail" else "gail", 3, n=8)
        try:
            with pytest.raises(OlyError, match="kind is"):
                a3.load(path)
        finally:
            close(v3)
    finally:
        close(v1, v2)


# ------------------------------------------------------------------------------ b. exact resume
def run_fits(core, n):
    outs = [fit_tensors(o) for o in core.learn(n * T, T)]
    assert len(outs) == n
    return outs


@pytest.mark.parametrize("algo,device_reset,log", [("gail", True, False), ("gail", False, False), ("vail", True, False),
                                                   ("vail", False, False), ("vail", True, True)])
def test_exact_resume(algo, device_reset, log, tmp_path):
    from olympic_hip import il_checkpoint as ck
    vecs = []
    try:
        runs = {}
        for name in ("A", "A2"):                             # uninterrupted, and the same again: the control
            agent, core, vec = build(algo, 0, device_reset, log)
            vecs.append(vec)
            assert core.device_reset is device_reset and agent.iter == 1
            outs = run_fits(core, 6)
            runs[name] = (outs, agent.state_dict(), core.state_dict(), core.evaluate(8),
                          list(agent.sw.rows) if log else None)
        outs = runs["A"][0]
        assert [o["disc_trained"] for o in outs] == [False, False, True, False, False, True]
        assert ("iter_log" in outs[5]) == log and ("disc_log" in outs[5]) == log
        # episodes end, and are reset, inside the windows; some of them by falling
        last = core.blocks["last"]
        assert int(last[:-1].sum()) >= N
        # the precondition: the existing path is deterministic
        assert_same(runs["A"], runs["A2"], "A against A'")
        # B: three fits, a file, fresh objects from other seeds, three more fits
        agent, core, vec = build(algo, 0, device_reset, log)
        vecs.append(vec)
        first = run_fits(core, 3)
        assert_same(first, outs[:3], "B's first three fits")
        path = ck.save(str(tmp_path / "mid.pt"), agent, core, epoch=1)
        close(vecs.pop())
        del agent, core, vec
        agent, core, vec = build(algo, 11, device_reset, log)
        vecs.append(vec)
        run_fits(core, 1)                                    # a past of its own, to be overwritten
        assert ck.load(path, agent, core) == dict(epoch=1)
        rest = run_fits(core, 3)
        n = assert_same(rest, outs[3:], "fits 4-6 after the resume")
        assert n >= 3 * 4 + 1
        assert_same(agent.state_dict(), runs["A"][1], "the final agent state")
        assert_same(core.state_dict(), runs["A"][2], "the final core state")
        assert_same(core.evaluate(8), runs["A"][3], "evaluate after the resume")
        if log:                                              # the writer got fit 6's scalars (iter 6 // 3 = 2), the same ones
            want = [(t, repr(v), s) for t, v, s in runs["A"][4] if s == 2]
            assert len(want) >= 12 + 6 and [(t, repr(v), s) for t, v, s in agent.sw.rows] == want
    finally:
        close(*vecs)


# ------------------------------------------------------------------------------ c. the environment's reset stream
def test_vec_env_resumes_reset_where_inside_a_block():
    from olympic_hip.envs import LocoEnvBase
    A = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=N, seed=0).vec
    B = LocoEnvBase.make("UnitreeH1.walk.real", num_envs=N, seed=9).vec
    try:
        g = torch.Generator(device="cuda").manual_seed(1)
        A.reset(), B.reset()
        B.reset_where(None)                                  # B's own stream has started too, from another seed
        act = lambda: torch.randn((N, A.spec.n_act), device="cuda", generator=g)      # noqa: E731
        for i in range(3):
            A.step(act())
            A.reset_where(torch.rand(N, device="cuda", generator=g) < 0.4)
        assert {k: c for k, (_, c) in A._drawn.items()} == dict(traj=3, step=3)       # inside the block of 64
        d = A.state_dict()
        assert d["drawn"]["step"]["cursor"] == 3 and tuple(d["drawn"]["step"]["block"].shape) == (A._DRAW_AHEAD, N)
        assert d["dev_gen"] is not None
        B.load_state_dict(d)
        assert {k: c for k, (_, c) in B._drawn.items()} == dict(traj=3, step=3)
        for k in ("_origin", "_cur_traj", "_cur_step", "_sample", "_prev", "episode_steps", "_obs"):
            assert torch.equal(getattr(A, k), getattr(B, k)), k
        draws = set()
        for i in range(10):                                  # the next ten resets draw the same indices
            a = act()
            oa, ob = A.step(a)[0], B.step(a)[0]
            assert torch.equal(oa, ob), i
            m = torch.rand(N, device="cuda", generator=g) < 0.5
            ra, rb = A.reset_where(m), B.reset_where(m)
            assert torch.equal(A._cur_step, B._cur_step) and torch.equal(A._cur_traj, B._cur_traj), i
            assert torch.equal(A._origin, B._origin) and torch.equal(ra, rb), i
            assert A._drawn["step"][1] == B._drawn["step"][1] == 4 + i
            draws.add(tuple(A._cur_step[m].tolist()))
        assert len(draws) == 10                              # the resets did draw
        # past the end of the block both draw the next one from the restored generator
        A._drawn = {k: (b, A._DRAW_AHEAD) for k, (b, _) in A._drawn.items()}
        B._drawn = {k: (b, B._DRAW_AHEAD) for k, (b, _) in B._drawn.items()}
        A.reset_where(None), B.reset_where(None)
        assert torch.equal(A._cur_step, B._cur_step) and torch.equal(A._drawn["step"][0], B._drawn["step"][0])
        # a dict from before the environment had a stream of its own leaves the stream alone
        old = {k: v for k, v in A.state_dict().items() if k not in ("dev_gen", "drawn", "physics")}
        keep = B._drawn["step"][0].clone(), B._drawn["step"][1], B._dev_gen.get_state().clone()
        B.load_state_dict(old)
        assert torch.equal(B._drawn["step"][0], keep[0]) and B._drawn["step"][1] == keep[1]
        assert torch.equal(B._dev_gen.get_state(), keep[2])
    finally:
        close(A, B)


# ------------------------------------------------------------------------------ d. the saver's snapshot
def test_snapshot_is_independent_of_the_agent(tmp_path):
    from olympic_hip import il_checkpoint as ck
    a1, c1, v1 = build("vail", 0)
    a2, c2, v2 = build("vail", 4)
    try:
        saver = ck.BestAgentSaver(str(tmp_path), n_epochs_save=3)
        c1.learn(T, T)
        want_agent, want_core = a1.state_dict(), c1.state_dict()
        assert saver.save(a1, 1.5, core=c1) is None and os.listdir(tmp_path) == []     # held on the device, not written
        held = saver.best_curr_agent[0]
        assert all(t.is_cuda for _, t in tensors(held) if torch.is_tensor(t) and t.numel() > 16)
        c1.learn(2 * T, T)                                   # two more fits move every tensor of the agent
        assert saver.save(a1, 1.0, core=c1) is None          # no improvement: the snapshot stays
        path = saver.save_curr_best_agent()
        assert os.path.basename(path) == "agent_epoch_0_J_1.500000.pt" and os.listdir(tmp_path) == [os.path.basename(path)]
        assert ck.load(path, a2, c2) == dict(epoch=0, J=1.5)
        assert_same(a2.state_dict(), want_agent, "the file against the snapshot")
        assert_same(c2.state_dict(), want_core, "the file's core against the snapshot")
        now = a1.state_dict()
        assert now["iter"] == 4 and a2.iter == 2
        for key in ("critic/param", "policy/theta", "standardizer/colstats", "disc/params/0"):
            x = dict(("/".join(p.split("/")[1:]), t) for p, t in tensors(now))[key]
            y = dict(("/".join(p.split("/")[1:]), t) for p, t in tensors(want_agent))[key]
            assert not torch.equal(x, y), key                # the agent did move on
    finally:
        close(v1, v2)
