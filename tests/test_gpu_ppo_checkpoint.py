"""Checkpoint and resume of PPO.train on the GPU: a run stopped after iteration 1 and continued in fresh objects from
other seeds must end in the very bits the uninterrupted run ends in.

Every comparison is torch.equal / == on the same computation run again, so there is no tolerance to choose.  The set-up is
tests/test_gpu_vecstep.py::test_ppo_train_on_the_device_rollout's: 256 environments on the synthetic readback
a3_synthetic_blocks(256, 9, seed=4), max_traj_len = 16 (T = 16, 4096 rows), four minibatches of 1024, two epochs, an
evaluation every second iteration, four iterations.  Per case three runs: A uninterrupted; A' the same with
checkpoint_every=2 (A' == A: the path is reproducible and a checkpoint disturbs nothing; a failure there says "not
reproducible" and is no resume failure); B fresh objects seeded differently, train(resume=A's file of iteration 1).
A' keeps its periodic files (checkpoint_keep): checkpoint.pt itself is replaced by iteration 3's before A' returns."""
import os

import numpy as np
import pytest
import torch

from olympic_hip import specs
from olympic_hip.synthetic import A3_FLOOR_BODY, A3_GEOM_BODYID, A3_LFOOT_BODY, A3_RFOOT_BODY, a3_synthetic_blocks

pytestmark = pytest.mark.gpu
CONTACT = (A3_GEOM_BODYID, A3_FLOOR_BODY, A3_RFOOT_BODY, A3_LFOOT_BODY)
N, N_ITR, SEED_A = 256, 4, 4
CASES = {                                                   # attributes set on the PPO object, mirror_coeff, symmetric env
    "default": (dict(), 0.0, False),                        # K13 rollout, K14 one-call epoch, device permutation
    "host_perm": (dict(device_permutation=False), 0.0, False),      # the draw-ahead _next_perm
    "torch_optim": (dict(update_kernel=False), 0.0, False),         # two torch Adam optimisers
    "mirror": (dict(), 0.4, True),                          # SymmetricEnv, mirror loss inside K14
}
PARAMS = [("default", False), ("default", True), ("host_perm", True), ("host_perm", False), ("torch_optim", False),
          ("torch_optim", True), ("mirror", True)]
_BLOCKS = {}


def make_env(n, rs_seed, symmetric=False):
    from olympic_hip.a3 import ReplayA3Physics, VecA3Env
    from olympic_hip.engine import Engine
    from olympic_hip.wrappers import SymmetricEnv
    if n not in _BLOCKS:                                    # the readback is data, the same for every run
        host = a3_synthetic_blocks(n, 9, seed=4, C=16, p_bad=0.02, p_low=0.01)
        _BLOCKS[n] = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    spec = specs.A3Spec(mass=41.5)
    env = VecA3Env(spec, n, Engine(0), ReplayA3Physics(dict(_BLOCKS[n])), *CONTACT, rs=np.random.RandomState(rs_seed))
    env.device = env.eng.device
    if symmetric:
        return SymmetricEnv(lambda: env, mirrored_obs=list(spec.mirrored_obs), mirrored_act=list(spec.mirrored_acts),
                            clock_inds=list(spec.clock_inds))
    return env


def make_run(case, anneal, path, seed, n=N):
    """(ppo, env, policy, critic) from one seed: the weights, the input tables, the environment's reset stream and
    torch's two generators all follow from it."""
    from olympic_hip.ppo import PPO, MLPCritic, MLPGaussianActor
    attrs, mirror_coeff, symmetric = CASES[case]
    args = dict(gamma=0.99, lam=0.95, lr=1e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=1024, epochs=2,
                max_traj_len=16, use_gae=False, num_procs=n, max_grad_norm=0.05, mirror_coeff=mirror_coeff, eval_freq=2)
    ppo = PPO(args, str(path))
    for k, v in attrs.items():
        setattr(ppo, k, v)
    if anneal and seed == SEED_A:                           # a resumed run gets these from the file
        ppo.highest_reward = 100.0                          # > 2/3 max_traj_len: the exploration anneal moves
    torch.manual_seed(seed)
    pi = MLPGaussianActor(41, 12, fixed_std=None if seed == SEED_A else torch.tensor(0.3)).cuda()
    vf = MLPCritic(41).cuda()
    pi.obs_mean = torch.randn(41, device="cuda") * 0.1
    pi.obs_std = torch.rand(41, device="cuda") + 0.75
    env = make_env(n, seed, symmetric)
    torch.manual_seed(1000 + seed)                          # where training starts in both of torch's streams
    return ppo, env, pi, vf


def end_state(ppo, env, hist):
    """Everything the issue lists, as one nest; the three streams' next draws come last (they move the streams)."""
    from olympic_hip import ppo_checkpoint as ck
    inner = env                                             # a SymmetricEnv hands every attribute through
    d = ck.to_host(dict(policy=ck.module_state(ppo.policy), critic=ck.module_state(ppo.critic), optimiser=ck.optimiser_state(ppo),
             env=env.state_dict(), physics_k=int(inner.physics.k),
             numbers=[int(ppo.total_steps), float(ppo.highest_reward), float(ppo.curr_anneal), int(ppo.iteration_count)],
             next_perm=getattr(ppo, "_next_perm", None),
             logs=[open(ppo.train_fn).read(), open(ppo.eval_fn).read()],
             history=[[h["itr"], h["losses"], h["ep_return"], h["ep_len"], h.get("eval_return")] for h in hist]))
    d["draws"] = [torch.rand(5), torch.rand(5, device="cuda"), torch.randperm(9, device="cuda"),
                  torch.from_numpy(inner._reset_one.rs.uniform(size=5))]
    torch.cuda.synchronize()
    return d


def leaves(nest, prefix=""):
    if isinstance(nest, dict):
        for k, v in nest.items():
            yield from leaves(v, f"{prefix}/{k}")
    elif isinstance(nest, (list, tuple)):
        for i, v in enumerate(nest):
            yield from leaves(v, f"{prefix}/{i}")
    else:
        yield prefix, nest


def first_difference(a, b):
    """The path of the first leaf that differs (tensors bit for bit, NaN equal to NaN), or None."""
    la, lb = list(leaves(a)), list(leaves(b))
    if [p for p, _ in la] != [p for p, _ in lb]:
        return "the two nests' paths"
    for (p, x), (_, y) in zip(la, lb):
        if torch.is_tensor(x):
            if not (torch.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape and
                    torch.equal(x.cpu().contiguous().reshape(-1).view(torch.uint8), y.cpu().contiguous().reshape(-1).view(torch.uint8))):
                return p
        elif isinstance(x, float) and x != x:
            if y == y:
                return p
        elif not (x == y):
            return p
    return None


_RUNS = {}


def reference_runs(case, anneal, tmp_root):
    """Run A and run A' of a case, made once: (A's end state, A''s end state, A''s directory)."""
    key = (case, anneal)
    if key not in _RUNS:
        out = []
        for name, kw in (("A", {}), ("A2", dict(checkpoint_every=2, checkpoint_keep=True))):
            path = tmp_root / f"{case}-{int(anneal)}-{name}"
            ppo, env, pi, vf = make_run(case, anneal, path, SEED_A)
            hist = ppo.train(lambda: env, pi, vf, n_itr=N_ITR, anneal_rate=0.9, verbose=False, **kw)
            out.append(end_state(ppo, env, hist))
        _RUNS[key] = (out[0], out[1], str(tmp_root / f"{case}-{int(anneal)}-A2"))
    return _RUNS[key]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("ppo_ckpt")


def check_run_a(a, case, anneal):
    """Run A is the run the case means."""
    assert len(a["history"]) == N_ITR and a["numbers"][0] == N_ITR * 16 * N and a["numbers"][3] == N_ITR - 1
    assert all(np.isfinite(h[1]).all() for h in a["history"]) and a["history"][1][4] is not None
    want_anneal = 1.0
    for _ in range(N_ITR if anneal else 0):
        want_anneal *= 0.9                                   # highest_reward stays above 2/3 max_traj_len, the std above 0.5
    assert a["numbers"][2] == want_anneal
    assert a["optimiser"]["kind"] == ("torch" if case == "torch_optim" else "kernel")
    if case == "torch_optim":
        assert float(a["optimiser"]["actor"]["state"]["0"]["step"]) == N_ITR * 2 * 4
    else:
        assert a["optimiser"]["steps"] == N_ITR * 2 * 4 and float(a["optimiser"]["actor"]["exp_avg"].abs().sum()) > 0
    assert (a["history"][0][1][4] > 0) == (case == "mirror")             # the mirror loss is on only there
    assert a["logs"][0].count("\n") == 1 + N_ITR and a["logs"][1].count("\n") == 1 + N_ITR // 2
    roll = a["env"]["device_rollout"]
    assert roll is not None and roll["tensors"]["pool"].numel() == N * 4 * 656 and roll["last_total"] >= N


# ------------------------------------------------------------------------------ a. exact resume
@pytest.mark.parametrize("case,anneal", PARAMS, ids=[f"{c}-{'anneal' if a else 'plain'}" for c, a in PARAMS])
def test_resume_continues_bit_for_bit(case, anneal, tmp_root):
    from olympic_hip import ppo_checkpoint as ck
    a, a2, dir_a2 = reference_runs(case, anneal, tmp_root)
    check_run_a(a, case, anneal)
    diff = first_difference(a, a2)
    if diff is not None:
        pytest.fail(f"not reproducible: two runs of the {case} path from the same seeds (the second taking checkpoints) "
                    f"first differ in {diff}")
    assert sorted(f for f in os.listdir(dir_a2) if f.startswith("checkpoint")) == \
        ["checkpoint.pt", "checkpoint_1.pt", "checkpoint_3.pt"]                  # and no .part
    assert ck.read(os.path.join(dir_a2, "checkpoint.pt"))["ppo"]["iteration"] == 3
    mid = ck.read(os.path.join(dir_a2, "checkpoint_1.pt"))
    assert mid["ppo"]["iteration"] == 1 and mid["meta"] == dict(iteration=1)
    assert (mid["ppo"]["next_perm"] is not None) == (case == "host_perm")       # drawn ahead behind the last epoch
    # B: other seeds everywhere, a new directory
    ppo, env, pi, vf = make_run(case, anneal, tmp_root / f"{case}-{int(anneal)}-B", 11)
    assert first_difference(ck.module_state(pi), mid["policy"]) is not None      # B really starts elsewhere
    hist = ppo.train(lambda: env, pi, vf, n_itr=N_ITR, anneal_rate=0.9, verbose=False,
                     resume=os.path.join(dir_a2, "checkpoint_1.pt"))
    assert [h["itr"] for h in hist] == [2, 3]
    b = end_state(ppo, env, hist)
    want = dict(a, history=a["history"][2:])
    diff = first_difference(want, b)
    assert diff is None, f"the resumed run first differs from the uninterrupted one in {diff}"
    assert torch.equal(ppo.old_policy.obs_mean, pi.obs_mean) and torch.equal(ppo.old_policy.fixed_std, pi.fixed_std)
    assert os.path.exists(os.path.join(ppo.save_path, "actor_3.pt"))             # the module files are written as before


# ------------------------------------------------------------------------------ b. extending a finished run
def test_a_finished_run_is_extended(tmp_root):
    a, _, _ = reference_runs("host_perm", True, tmp_root)
    ppo, env, pi, vf = make_run("host_perm", True, tmp_root / "short", SEED_A)
    hist = ppo.train(lambda: env, pi, vf, n_itr=2, anneal_rate=0.9, verbose=False, checkpoint_every=2)
    assert [h["itr"] for h in hist] == [0, 1] and getattr(ppo, "_next_perm", None) is None    # nothing drawn ahead at the end
    assert first_difference([h["losses"] for h in hist], [h[1] for h in a["history"][:2]]) is None
    ppo, env, pi, vf = make_run("host_perm", True, tmp_root / "extended", 12)
    hist = ppo.train(lambda: env, pi, vf, n_itr=N_ITR, anneal_rate=0.9, verbose=False, resume=str(tmp_root / "short"))
    diff = first_difference(dict(a, history=a["history"][2:]), end_state(ppo, env, hist))
    assert diff is None, f"the extended run first differs from the uninterrupted one in {diff}"


# ------------------------------------------------------------------------------ c. load is in place
def test_load_is_in_place(tmp_root):
    from olympic_hip import ppo_checkpoint as ck
    _, _, dir_a2 = reference_runs("default", False, tmp_root)
    path = os.path.join(dir_a2, "checkpoint_1.pt")
    ppo, env, pi, vf = make_run("default", False, tmp_root / "in_place", 13)
    ppo.train(lambda: env, pi, vf, n_itr=1, verbose=False)                       # live buffers and a past of its own
    roll = env._dev_rollout

    def pointers():
        d = {f"param{i}": p for i, p in enumerate(list(pi.parameters()) + list(vf.parameters()))}
        for i, nt in enumerate(ppo.kupd.nets):
            d.update({f"flat{i}": nt["param"], f"exp_avg{i}": nt["exp_avg"], f"exp_avg_sq{i}": nt["exp_avg_sq"]})
        d.update(pool=roll.pool, pool_count=roll.pool_count, ctr=roll.ctr, obs_mean=pi.obs_mean, fixed_std=pi.fixed_std,
                 phase=env.state["phase"], packed_a=ppo.kupd.fw.packed_a, stash0=roll._stash_t[0], stash1=roll._stash_t[1])
        return {k: v.data_ptr() for k, v in d.items()}
    before = pointers()
    assert all(before.values()) and ppo.kupd.steps == 8
    assert ck.load(path, ppo, env) == dict(iteration=1)
    assert pointers() == before
    mid = ck.read(path)
    assert ppo.kupd.steps == 16 and ppo.iteration_count == 1 and ppo.total_steps == 2 * 16 * N
    assert torch.equal(ppo.kupd.nets[0]["exp_avg"].cpu(), mid["optimiser"]["actor"]["exp_avg"])
    assert torch.equal(pi.means.weight.detach().cpu(), mid["policy"]["params"]["means.weight"])
    assert pi.means.weight.data_ptr() >= ppo.kupd.nets[0]["param"].data_ptr()    # still a view of the flat buffer
    assert torch.equal(roll.pool.cpu(), mid["env"]["device_rollout"]["tensors"]["pool"])
    assert first_difference(ck.to_host(ck.state_dict(ppo, env)["env"]), mid["env"]) is None


# ------------------------------------------------------------------------------ d. refusals
def test_refusals(tmp_root, monkeypatch):
    from olympic_hip._ffi import OlyError
    _, _, dir_a2 = reference_runs("default", False, tmp_root)
    path = os.path.join(dir_a2, "checkpoint_1.pt")
    # another number of environments
    ppo, env, pi, vf = make_run("default", False, tmp_root / "r1", 5, n=128)
    w0 = pi.means.weight.detach().clone()
    with pytest.raises(OlyError, match="num_envs is 256 in the file, 128 in this run"):
        ppo.train(lambda: env, pi, vf, n_itr=N_ITR, verbose=False, resume=path)
    assert torch.equal(w0, pi.means.weight) and ppo.total_steps == 0             # nothing was written
    # a kernel-path file into the torch path
    ppo, env, pi, vf = make_run("torch_optim", False, tmp_root / "r2", 5)
    with pytest.raises(OlyError, match="update is 'kernel' in the file, 'fused' in this run"):
        ppo.train(lambda: env, pi, vf, n_itr=N_ITR, verbose=False, resume=path)
    assert len(ppo.actor_optimizer.state) == 0
    # more than one rank
    import torch.distributed as tdist
    from olympic_hip import dist as odist
    monkeypatch.setattr(odist, "is_dist", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **k: 2)
    ppo, env, pi, vf = make_run("default", False, tmp_root / "r3", 5)
    for kw in (dict(resume=path), dict(checkpoint_every=2)):
        with pytest.raises(OlyError, match="single-rank only; this process group has 2 ranks"):
            ppo.train(lambda: env, pi, vf, n_itr=N_ITR, verbose=False, **kw)
    assert ppo.total_steps == 0


# ------------------------------------------------------------------------------ e. the launcher
def test_launcher_resume_and_continued(tmp_root, monkeypatch):
    """examples/train_a3_walk.py (StickFigureA3 inside a SymmetricEnv, the K14 path with the mirror loss): a run of four
    iterations against two + --resume; --continued takes the weights and tables alone; neither runs the pre-pass."""
    import sys
    from argparse import Namespace
    from olympic_hip import ppo_checkpoint as ck
    examples = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    monkeypatch.syspath_prepend(examples)
    import train_a3_walk as launcher

    def args(logdir, **kw):
        d = dict(seed=0, logdir=str(tmp_root / logdir), input_norm_steps=0, n_itr=4, lr=1e-4, eps=1e-5, lam=0.95, gamma=0.99,
                 anneal=1.0, std_dev=-1.5, entropy_coeff=0.0, clip=0.2, minibatch_size=256, epochs=2, use_gae=True,
                 num_procs=64, max_grad_norm=0.05, max_traj_len=8, no_mirror=False, mirror_coeff=0.4, eval_freq=2,
                 no_graph=False, continued=None, resume=None, checkpoint_every=None)
        d.update(kw)
        return Namespace(**d)
    keep = np.random.get_state()
    try:
        whole = launcher.run_experiment(args("whole", checkpoint_every=4))
        assert [h["itr"] for h in whole] == [0, 1, 2, 3]
        launcher.run_experiment(args("half", n_itr=2, checkpoint_every=2))

        def no_pre_pass(*a, **k):
            raise AssertionError("the normalisation pre-pass ran")
        monkeypatch.setattr(launcher, "get_normalization_params", no_pre_pass)
        np.random.seed(123)                                  # a resumed run brings its streams with it
        rest = launcher.run_experiment(args("half", input_norm_steps=1000, resume=str(tmp_root / "half"), checkpoint_every=2))
        assert [h["itr"] for h in rest] == [2, 3]
        assert [h["losses"] for h in rest] == [h["losses"] for h in whole[2:]]
        a, b = ck.read(str(tmp_root / "whole" / "checkpoint.pt")), ck.read(str(tmp_root / "half" / "checkpoint.pt"))
        assert a["header"]["update"] == "kernel" and a["header"]["mirror"] and a["env"]["vec"]["device_rollout"] is not None
        for part in ("ppo", "policy", "critic", "optimiser", "env", "rng", "logs"):
            assert first_difference(a[part], b[part]) is None, part
        # --continued: iteration 0 again, from the stored weights, with a fresh optimiser
        again = launcher.run_experiment(args("again", n_itr=1, input_norm_steps=1000, continued=str(tmp_root / "whole"),
                                             checkpoint_every=1))
        c = ck.read(str(tmp_root / "again" / "checkpoint.pt"))
        assert [h["itr"] for h in again] == [0] and c["optimiser"]["steps"] == 2 * 2 and a["optimiser"]["steps"] == 4 * 2 * 2
        assert c["logs"]["train"].count("\n") == 2
    finally:
        np.random.set_state(keep)
        sys.modules.pop("train_a3_walk", None)
