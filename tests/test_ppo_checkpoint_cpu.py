"""ppo_checkpoint without a GPU: the container's round trip and refusals, the stored form of the numpy stream and of Adam,
load_policy, the header comparison and the restored logs.  The run here is a PPO object set up by hand around CPU modules
(train() itself needs the engine); the device runs are in tests/test_gpu_ppo_checkpoint.py."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

from olympic_hip import ppo_checkpoint as ck
from olympic_hip._ffi import OlyError
from olympic_hip.ppo import PPO, MLPCritic, MLPGaussianActor

ARGS = dict(gamma=0.99, lam=0.95, lr=1e-3, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=8, epochs=1,
            max_traj_len=16, use_gae=False, num_procs=4, max_grad_norm=0.05, mirror_coeff=0.0, eval_freq=2)


class HostEnv:
    """The least an environment gives a checkpoint: its size and a state_dict of its own."""

    def __init__(self, n=4, seed=0):
        self.num_envs = n
        self.x = torch.full((n, 3), float(seed))
        self.rs = np.random.RandomState(seed)

    def state_dict(self):
        return dict(x=self.x.clone(), rs=ck.numpy_stream_state(self.rs))

    def load_state_dict(self, d):
        self.x.copy_(d["x"])
        ck.set_numpy_stream(self.rs, d["rs"])


def make_run(path, seed, hidden=(16, 16), n=4, update="torch", tables=True):
    """A PPO object as train() leaves it on the torch path: modules, their two optimisers, the run's description."""
    torch.manual_seed(seed)
    ppo = PPO(ARGS, str(path))
    pi, vf = MLPGaussianActor(5, 3, layers=hidden), MLPCritic(5, layers=hidden)
    if tables:
        pi.obs_mean, pi.obs_std = torch.randn(5), torch.rand(5) + 0.5
    ppo.policy, ppo.critic, ppo.old_policy = pi, vf, deepcopy(pi)
    ppo.actor_optimizer = torch.optim.Adam(pi.parameters(), lr=ppo.lr, eps=ppo.eps)
    ppo.critic_optimizer = torch.optim.Adam(vf.parameters(), lr=ppo.lr, eps=ppo.eps)
    ppo._run = dict(update=update, T=16, mirror=False, device_permutation=False, rollout="host")
    return ppo, HostEnv(n, seed)


def step(ppo, x):
    for opt in (ppo.actor_optimizer, ppo.critic_optimizer):
        opt.zero_grad()
    (ppo.policy(x).square().mean() + ppo.critic(x).square().mean()).backward()
    ppo.actor_optimizer.step()
    ppo.critic_optimizer.step()


def params(ppo):
    return [p.detach().clone() for m in (ppo.policy, ppo.critic) for p in m.parameters()]


# ------------------------------------------------------------------------------ the container
def test_container_round_trips_a_nested_state(tmp_path):
    state = dict(header=dict(num_envs=4, actor_hidden=[16, 16], update="kernel", mirror=True),
                 ppo=dict(iteration=3, total_steps=12, highest_reward=-1, curr_anneal=0.81, next_perm=torch.randperm(7)),
                 policy=dict(params=dict(w=torch.randn(3, 2)), obs_mean=0.0, fixed_std=torch.tensor(0.25)),
                 critic=None, optimiser=dict(kind="kernel", steps=5, actor=dict(exp_avg=torch.randn(9, dtype=torch.float32))),
                 env=dict(pool=torch.arange(656, dtype=torch.int64).to(torch.uint8), nest=[1, "a", None, [2.5, True]]),
                 rng=dict(torch_cpu=torch.get_rng_state()), logs=dict(train="ep_returns,ep_lens\n1.0,2.0\n", eval=None))
    path = ck.write(str(tmp_path / "sub" / "c.pt"), state, note="x", n=2)
    assert os.listdir(tmp_path / "sub") == ["c.pt"]          # no .part left behind
    obj = ck.read(path)
    assert obj["format"] == "olympic_hip.ppo_checkpoint" and obj["version"] == 1 and obj["meta"] == dict(note="x", n=2)
    assert set(obj) == {"format", "version", "header", "ppo", "policy", "critic", "optimiser", "env", "rng", "logs", "meta"}

    def same(a, b, where):
        if torch.is_tensor(a):
            assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b), where
        elif isinstance(a, dict):
            assert list(a) == list(b), where
            for k in a:
                same(a[k], b[k], f"{where}/{k}")
        elif isinstance(a, list):
            assert len(a) == len(b), where
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, f"{where}/{i}")
        else:
            assert type(a) is type(b) and a == b, where
    for k, v in state.items():
        same(v, obj[k], k)
    # written again under the same name: the file is replaced
    ck.write(path, dict(state, ppo=dict(iteration=4)))
    assert ck.read(path)["ppo"] == dict(iteration=4) and os.listdir(tmp_path / "sub") == ["c.pt"]


def test_refusals_of_the_reader(tmp_path):
    pickled = str(tmp_path / "module.pt")
    torch.save(MLPCritic(5, layers=(4, 4)), pickled)         # what PPO.save writes: a pickled module
    with pytest.raises(OlyError, match="would unpickle an object, which is refused"):
        ck.read(pickled)
    with pytest.raises(OlyError, match="would unpickle an object, which is refused"):
        ck.load_policy(pickled, MLPGaussianActor(5, 3, layers=(4, 4)), MLPCritic(5, layers=(4, 4)))
    other = str(tmp_path / "il.pt")
    torch.save(dict(format="olympic_hip.il_checkpoint", version=1, agent={}, core=None, meta={}), other)
    with pytest.raises(OlyError, match=r"ppo_checkpoint.load: .*format is 'olympic_hip.il_checkpoint', expected "
                                       r"'olympic_hip.ppo_checkpoint'"):
        ck.read(other)
    torch.save([1, 2], other)
    with pytest.raises(OlyError, match="format is 'list'"):
        ck.read(other)
    newer = str(tmp_path / "v2.pt")
    torch.save(dict(format=ck.FORMAT, version=2), newer)
    with pytest.raises(OlyError, match="version is 2, this reader takes 1"):
        ck.read(newer)
    with pytest.raises(OlyError, match="not int|not .*ndarray|holds tensors, numbers"):
        ck.write(str(tmp_path / "bad.pt"), dict(env=dict(a=np.zeros(3))))
    assert not os.path.exists(tmp_path / "bad.pt")


# ------------------------------------------------------------------------------ the numpy stream
@pytest.mark.parametrize("source", ["own", "global"])
def test_numpy_stream_round_trips_through_the_file(source, tmp_path):
    from olympic_hip.specs import A3Spec
    from olympic_hip.vecstep import draw_reset_records
    keep = np.random.get_state()
    try:
        rs = np.random.RandomState(5) if source == "own" else np.random
        if source == "global":
            np.random.seed(5)
        draw_reset_records(rs, 37, A3Spec())                 # somewhere inside the stream, not at a seed
        rs.normal()                                          # a cached Gaussian is part of the state
        d = ck.numpy_stream_state(rs)
        assert d["source"] == source and tuple(d["keys"].shape) == (624,) and d["has_gauss"] == 1
        path = ck.write(str(tmp_path / "rs.pt"), dict(env=dict(rs=d)))
        want = draw_reset_records(rs, 1000, A3Spec()).tobytes()
        want_normal = rs.normal()
        other = np.random.RandomState(99)
        other.uniform(size=11)
        assert draw_reset_records(deepcopy(other), 1000, A3Spec()).tobytes() != want
        ck.set_numpy_stream(other, ck.read(path)["env"]["rs"])
        assert draw_reset_records(other, 1000, A3Spec()).tobytes() == want
        assert other.normal() == want_normal
    finally:
        np.random.set_state(keep)


# ------------------------------------------------------------------------------ Adam
def test_adam_state_round_trips_through_the_file(tmp_path):
    a, _ = make_run(tmp_path / "a", 0)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(8, 5, generator=g) for _ in range(4)]
    for x in xs[:3]:
        step(a, x)
    path = ck.write(str(tmp_path / "adam.pt"), dict(policy=ck.module_state(a.policy), critic=ck.module_state(a.critic),
                                                     optimiser=ck.optimiser_state(a)))
    obj = ck.read(path)
    assert obj["optimiser"]["kind"] == "torch" and len(obj["optimiser"]["actor"]["state"]) == 6
    assert float(obj["optimiser"]["actor"]["state"]["0"]["step"]) == 3.0
    # into optimisers that have not stepped, and into ones with a past of their own (in place)
    for past in (0, 2):
        b, _ = make_run(tmp_path / f"b{past}", 7)
        for _ in range(past):
            step(b, torch.randn(8, 5))
        held = [st["exp_avg"].data_ptr() for st in b.actor_optimizer.state.values()]
        assert not all(torch.equal(p, q) for p, q in zip(params(a), params(b)))
        ck.check_module(b.policy, obj["policy"], "policy")
        ck.load_module(b.policy, obj["policy"])
        ck.load_module(b.critic, obj["critic"])
        ck.load_adam(b.actor_optimizer, obj["optimiser"]["actor"])
        ck.load_adam(b.critic_optimizer, obj["optimiser"]["critic"])
        if past:
            assert held == [st["exp_avg"].data_ptr() for st in b.actor_optimizer.state.values()]
        a2 = deepcopy(a)
        step(a2, xs[3])
        step(b, xs[3])
        assert all(torch.equal(p, q) for p, q in zip(params(a2), params(b))), past
        for oa, ob in ((a2.actor_optimizer, b.actor_optimizer), (a2.critic_optimizer, b.critic_optimizer)):
            for sa, sb in zip(oa.state.values(), ob.state.values()):
                assert float(sa["step"]) == float(sb["step"]) == 4.0
                assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    # weights alone do not give that step: the moments matter
    c, _ = make_run(tmp_path / "c", 7)
    ck.load_module(c.policy, obj["policy"])
    ck.load_module(c.critic, obj["critic"])
    a2 = deepcopy(a)
    step(a2, xs[3])
    step(c, xs[3])
    assert not all(torch.equal(p, q) for p, q in zip(params(a2), params(c)))


# ------------------------------------------------------------------------------ save / load / load_policy
def test_save_load_restores_the_run_and_the_logs_in_a_fresh_directory(tmp_path):
    a, env_a = make_run(tmp_path / "a", 0)
    step(a, torch.randn(8, 5))
    a.iteration_count, a.total_steps, a.highest_reward, a.curr_anneal = 5, 384, 12.5, 0.729
    a._next_perm = torch.randperm(64)
    with open(a.train_fn, "a") as f:
        f.write("1.5,16.0\n2.5,15.0\n")
    with open(a.eval_fn, "a") as f:
        f.write("3.25,16.0\n")
    env_a.x.normal_()
    path = ck.save(os.path.join(a.save_path, ck.FILE), a, env_a, iteration=5)
    want_cpu, want_np = torch.rand(3), env_a.rs.uniform(size=3)

    b, env_b = make_run(tmp_path / "elsewhere", 9)
    assert open(b.train_fn).read() == "ep_returns,ep_lens\n"
    ptrs = [p.data_ptr() for p in b.policy.parameters()] + [b.policy.obs_mean.data_ptr(), env_b.x.data_ptr()]
    assert ck.load(path, b, env_b) == dict(iteration=5)
    assert ptrs == [p.data_ptr() for p in b.policy.parameters()] + [b.policy.obs_mean.data_ptr(), env_b.x.data_ptr()]
    assert (b.iteration_count, b.total_steps, b.highest_reward, b.curr_anneal) == (5, 384, 12.5, 0.729)
    assert torch.equal(b._next_perm, a._next_perm) and torch.equal(env_b.x, env_a.x)
    assert all(torch.equal(p, q) for p, q in zip(params(a), params(b)))
    for m in (b.policy, b.old_policy):                       # the old policy's tables follow the policy's
        assert torch.equal(m.obs_mean, a.policy.obs_mean) and torch.equal(m.obs_std, a.policy.obs_std)
        assert torch.equal(m.fixed_std, a.policy.fixed_std)
    assert torch.equal(torch.rand(3), want_cpu) and np.array_equal(env_b.rs.uniform(size=3), want_np)
    assert open(b.train_fn).read() == "ep_returns,ep_lens\n1.5,16.0\n2.5,15.0\n"
    assert open(b.eval_fn).read() == "test_ep_returns,test_ep_lens\n3.25,16.0\n"
    assert len(b.actor_optimizer.state) == 6


def test_load_policy_takes_weights_and_tables_only(tmp_path):
    a, env_a = make_run(tmp_path / "a", 0)
    step(a, torch.randn(8, 5))
    ck.save(os.path.join(a.save_path, ck.FILE), a, env_a)
    x = torch.randn(6, 5)
    for where in (a.save_path, os.path.join(a.save_path, ck.FILE)):       # DIR/checkpoint.pt, or the file
        b, _ = make_run(tmp_path / "b", 4, tables=False)
        assert b.policy.obs_mean == 0.0 and not torch.equal(a.policy(x), b.policy(x))
        rng = torch.get_rng_state()
        assert ck.load_policy(where, b.policy, b.critic) == {}
        assert torch.equal(a.policy(x), b.policy(x)) and torch.equal(a.critic(x), b.critic(x))
        assert torch.equal(b.policy.obs_mean, a.policy.obs_mean) and torch.equal(b.policy.fixed_std, a.policy.fixed_std)
        assert len(b.actor_optimizer.state) == 0 and len(b.critic_optimizer.state) == 0
        assert b.iteration_count == 0 and torch.equal(torch.get_rng_state(), rng)
    with pytest.raises(OlyError, match=r"policy.actor_layers.0.weight's shape is \[16, 5\] in the file, \[8, 5\]"):
        ck.load_policy(a.save_path, MLPGaussianActor(5, 3, layers=(8, 8)), MLPCritic(5, layers=(8, 8)))


@pytest.mark.parametrize("field,kw,stored,own", [
    ("num_envs", dict(n=8), 4, 8),
    ("actor_hidden", dict(hidden=(8, 16)), [16, 16], [8, 16]),
    ("update", dict(update="kernel"), "torch", "kernel"),
])
def test_header_mismatch_names_the_field_and_writes_nothing(field, kw, stored, own, tmp_path):
    a, env_a = make_run(tmp_path / "a", 0)
    step(a, torch.randn(8, 5))
    with open(a.train_fn, "a") as f:
        f.write("1.5,16.0\n")
    path = ck.save(os.path.join(a.save_path, ck.FILE), a, env_a)
    b, env_b = make_run(tmp_path / "b", 3, **kw)
    before, x, rng = params(b), env_b.x.clone(), torch.get_rng_state()
    with pytest.raises(OlyError) as e:
        ck.load(path, b, env_b)
    assert f"{field} is {stored!r} in the file, {own!r} in this run" in str(e.value)
    assert all(torch.equal(p, q) for p, q in zip(before, params(b))) and torch.equal(env_b.x, x)
    assert b.iteration_count == 0 and torch.equal(torch.get_rng_state(), rng)
    assert open(b.train_fn).read() == "ep_returns,ep_lens\n"


def test_header_of_a_run_and_of_an_object_train_has_not_set_up(tmp_path):
    a, env_a = make_run(tmp_path / "a", 0)
    assert ck.header(a, env_a) == dict(obs_dim=5, act_dim=3, actor_hidden=[16, 16], critic_in=5, critic_hidden=[16, 16],
                                       num_envs=4, T=16, max_traj_len=16, update="torch", mirror=False,
                                       device_permutation=False, rollout="host")
    with pytest.raises(OlyError, match="PPO.train has not set this object up"):
        ck.save(str(tmp_path / "x.pt"), PPO(ARGS, str(tmp_path / "p")), env_a)
