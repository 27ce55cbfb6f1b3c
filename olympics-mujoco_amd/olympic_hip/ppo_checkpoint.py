"""Checkpoints of a PPO run (rl/algos/ppo.py:284-477; the launcher's --continued,
examples/reinforcement_learning_ppo/a3/train_a3_walk.py:54-64).

    ppo.train(..., checkpoint_every=k)       -> save(path, ppo, env) after every k-th iteration
    ppo.train(..., resume=path)              -> load(path, ppo, env), then the remaining iterations, bit for bit
    --continued PATH of the launcher         -> load_policy(path, policy, critic)

A checkpoint is ONE file written by torch.save, a nested dict of host tensors, Python numbers, strings, lists and None,

    dict(format="olympic_hip.ppo_checkpoint", version=1, header=..., ppo=..., policy=..., critic=..., optimiser=...,
         env=..., rng=..., logs=..., meta=...)

read with torch.load(path, map_location="cpu", weights_only=True) and nothing else (il_checkpoint.read_file): no object is
ever unpickled from a file.  Everything is written IN PLACE on load: the parameters (on the K14 path views of
KernelUpdate's flat buffers), Adam's moments, the environment's tensors and the reset-record pool keep their addresses,
so prepared launches, captured graphs and pointer-keyed caches stay valid.  The header is compared first; on a mismatch
nothing is written.

Stated differences from the reference: its --continued unpickles the two modules (torch.load of actor.pt / critic.pt),
restores no optimiser state and starts at iteration 0 with fresh random streams; here the weights are tensors in a
checked container, and --resume additionally restores Adam, the environment, the random streams and the logs.  The
reference's files are actor.pt / critic.pt (+ _<itr>); those are still written, the checkpoint is checkpoint.pt
(+ checkpoint_<itr>.pt).

Nothing here runs per step and nothing here launches a kernel of its own; the module imports without the shared library.
"""
import os

import numpy as np
import torch

from ._ffi import OlyError
from .il_checkpoint import read_file, to_host, write_file

FORMAT, VERSION = "olympic_hip.ppo_checkpoint", 1
FILE = "checkpoint.pt"
_TABLES = ("obs_mean", "obs_std", "fixed_std")


# ---------------------------------------------------------------------------------- the container
def write(path, state, **meta):
    """Write a state taken earlier by state_dict (tensors may still be on the device)."""
    obj = dict(format=FORMAT, version=VERSION, meta=to_host(meta))
    for k in ("header", "ppo", "policy", "critic", "optimiser", "env", "rng", "logs"):
        obj[k] = to_host(state.get(k))
    return write_file(path, obj)


def read(path):
    """The checked content of a checkpoint file, tensors on the host."""
    return read_file(path, FORMAT, VERSION, who="ppo_checkpoint.load")


def resolve(path):
    """`path`, or DIR/checkpoint.pt when it names a directory."""
    path = os.fspath(path)
    return os.path.join(path, FILE) if os.path.isdir(path) else path


def _mismatch(field, stored, own):
    raise OlyError(f"ppo_checkpoint.load: {field} is {stored!r} in the file, {own!r} in this run")


def check_header(stored, own):
    """Every field of this run's header must be the file's; the first that is not is named with both values."""
    for k in own:
        if k not in stored:
            _mismatch(k, None, own[k])
        if stored[k] != own[k]:
            _mismatch(k, stored[k], own[k])
    for k in stored:
        if k not in own:
            _mismatch(k, stored[k], None)


# ---------------------------------------------------------------------------------- random streams
def numpy_stream_state(rs):
    """A numpy RandomState (or the numpy.random module: the global stream) as its 624 words plus three numbers."""
    if not hasattr(rs, "get_state"):
        raise OlyError(f"ppo_checkpoint: the reset stream is a {type(rs).__name__}: a numpy RandomState or numpy.random "
                       "is needed to store it")
    kind, keys, pos, has_gauss, cached = rs.get_state()
    if kind != "MT19937":
        raise OlyError(f"ppo_checkpoint: the numpy stream is {kind!r}, expected 'MT19937'")
    return dict(source="global" if rs is np.random else "own", keys=torch.from_numpy(np.asarray(keys).astype(np.int64)),
                pos=int(pos), has_gauss=int(has_gauss), cached_gaussian=float(cached))


def set_numpy_stream(rs, d):
    keys = np.asarray(d["keys"].cpu().numpy() if torch.is_tensor(d["keys"]) else d["keys"])
    if keys.shape != (624,):
        raise OlyError(f"ppo_checkpoint.load: the numpy stream holds {keys.shape} words, expected (624,)")
    rs.set_state(("MT19937", keys.astype(np.uint32), int(d["pos"]), int(d["has_gauss"]), float(d["cached_gaussian"])))


def _cuda_device(env):
    dev = getattr(env, "device", None)
    if dev is None and hasattr(env, "eng"):
        dev = env.eng.device
    if dev is None:
        return None
    dev = torch.device(dev) if not isinstance(dev, int) else torch.device("cuda", dev)
    return dev if dev.type == "cuda" else None


def rng_state(env=None):
    """torch's CPU generator (the host permutation) and the CUDA generator of the env's device (action noise, the device
    randperm).  Reading a generator's state draws nothing."""
    dev = _cuda_device(env) if env is not None else None
    return dict(torch_cpu=torch.get_rng_state().clone(),
                torch_cuda=None if dev is None else torch.cuda.get_rng_state(dev).clone(),
                cuda_device=None if dev is None else str(dev))


def set_rng_state(d, env=None):
    torch.set_rng_state(d["torch_cpu"].cpu())
    dev = _cuda_device(env) if env is not None else None
    if d.get("torch_cuda") is not None and dev is not None:
        torch.cuda.set_rng_state(d["torch_cuda"].cpu(), dev)


# ---------------------------------------------------------------------------------- modules
def _number(x):
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    return float(x)


def _table(v):
    if v is None:
        return None
    if torch.is_tensor(v):
        return v.detach().clone()
    if isinstance(v, np.ndarray):
        return torch.from_numpy(np.array(v))
    return _number(v)


def module_state(module):
    """Every entry of the module's state_dict (clones), and the input-normalisation tables / fixed std it carries as
    plain attributes (rl/policies/actor.py:152-158, 189)."""
    d = dict(params={k: v.detach().clone() for k, v in module.state_dict().items()})
    for name in _TABLES:
        if hasattr(module, name):
            d[name] = _table(getattr(module, name))
    return d


def check_module(module, rec, who):
    own = module.state_dict()
    if list(own) != list(rec["params"]):
        _mismatch(f"{who}'s parameter names", list(rec["params"]), list(own))
    for k, v in own.items():
        if tuple(v.shape) != tuple(rec["params"][k].shape):
            _mismatch(f"{who}.{k}'s shape", list(rec["params"][k].shape), list(v.shape))


@torch.no_grad()
def load_module(module, rec):
    """Parameters and buffers by copy_ into the module's own tensors; a table that is a tensor of the stored shape
    likewise, else the attribute takes the stored value (a module built with obs_mean = 0.0 gets the stored vector)."""
    own = module.state_dict()                               # detached views of the module's own storage
    for k, v in own.items():
        v.copy_(rec["params"][k])
    ref = next(iter(own.values()), None)
    for name in _TABLES:
        if name not in rec:
            continue
        v, cur = rec[name], getattr(module, name, None)
        if torch.is_tensor(v) and torch.is_tensor(cur) and cur.shape == v.shape:
            cur.copy_(v)
        elif torch.is_tensor(v):
            v = v.to(ref.device) if ref is not None else v.clone()
            if name in getattr(module, "_buffers", {}):
                module._buffers[name] = v
            else:
                setattr(module, name, v)
        else:
            setattr(module, name, v)


def _dims(module):
    """(input width, [output width of every 2-D weight]) in the module's parameter order."""
    w = [p for p in module.parameters() if p.dim() == 2]
    return (int(w[0].shape[1]), [int(p.shape[0]) for p in w]) if w else (0, [])


# ---------------------------------------------------------------------------------- optimiser
def adam_state(opt):
    sd = opt.state_dict()
    return dict(state={str(k): {n: (v.detach().clone() if torch.is_tensor(v) else v) for n, v in st.items()}
                       for k, st in sd["state"].items()},
                param_groups=[{n: (list(v) if isinstance(v, tuple) else v) for n, v in g.items()}
                              for g in sd["param_groups"]])


def check_adam(opt, rec, who):
    params = [p for g in opt.param_groups for p in g["params"]]
    n = sum(len(g["params"]) for g in rec["param_groups"])
    if n != len(params):
        _mismatch(f"{who} optimiser's parameter count", n, len(params))
    for k, st in rec["state"].items():
        p = params[int(k)]
        for name in ("exp_avg", "exp_avg_sq"):
            if name in st and tuple(st[name].shape) != tuple(p.shape):
                _mismatch(f"{who} optimiser's {name}[{k}] shape", list(st[name].shape), list(p.shape))


@torch.no_grad()
def load_adam(opt, rec):
    """Into tensors the optimiser already holds: copy_.  An optimiser that has not stepped yet holds none, and takes the
    stored ones through its own load_state_dict (which moves them to the parameters' device: the capturable `step`
    included)."""
    params = [p for g in opt.param_groups for p in g["params"]]
    fresh = {}
    for k, st in rec["state"].items():
        own = opt.state.get(params[int(k)])
        if own:
            for name, v in st.items():
                if torch.is_tensor(own.get(name)) and torch.is_tensor(v):
                    own[name].copy_(v)
                else:
                    own[name] = v
        else:
            fresh[int(k)] = {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()}   # never the caller's
    if fresh:
        sd = opt.state_dict()
        keep = {k: v for k, v in sd["state"].items() if k not in fresh}
        opt.load_state_dict(dict(state={**keep, **fresh}, param_groups=sd["param_groups"]))


def optimiser_state(ppo):
    path = ppo._run["update"]
    if path == "kernel":
        kupd = getattr(ppo, "kupd", None)
        if kupd is None:
            return dict(kind="kernel", steps=0, actor=None, critic=None)
        nets = [dict(exp_avg=nt["exp_avg"].clone(), exp_avg_sq=nt["exp_avg_sq"].clone()) for nt in kupd.nets]
        return dict(kind="kernel", steps=int(kupd.steps), actor=nets[0], critic=nets[1])
    return dict(kind="torch", actor=adam_state(ppo.actor_optimizer), critic=adam_state(ppo.critic_optimizer))


def _check_optimiser(ppo, rec):
    if rec["kind"] == "kernel":
        kupd = ppo._ensure_kernel_update()
        for nt, who in zip(kupd.nets, ("actor", "critic")):
            for name in ("exp_avg", "exp_avg_sq"):
                if rec[who] is not None and tuple(rec[who][name].shape) != tuple(nt[name].shape):
                    _mismatch(f"{who}'s {name} length", list(rec[who][name].shape), list(nt[name].shape))
    else:
        check_adam(ppo.actor_optimizer, rec["actor"], "actor")
        check_adam(ppo.critic_optimizer, rec["critic"], "critic")


@torch.no_grad()
def _load_optimiser(ppo, rec):
    if rec["kind"] == "kernel":
        kupd = ppo._ensure_kernel_update()
        for nt, who in zip(kupd.nets, ("actor", "critic")):
            for name in ("exp_avg", "exp_avg_sq"):
                if rec[who] is None:
                    nt[name].zero_()
                else:
                    nt[name].copy_(rec[who][name])
        kupd.steps = int(rec["steps"])
        kupd._norm_ready = False
        kupd.fw.refresh()                                   # the packed weight streams follow the loaded parameters
        kupd.nets[0]["packed"], kupd.nets[1]["packed"] = kupd.fw.packed_a, kupd.fw.packed_c
    else:
        load_adam(ppo.actor_optimizer, rec["actor"])
        load_adam(ppo.critic_optimizer, rec["critic"])


# ---------------------------------------------------------------------------------- the whole run
def header(ppo, env):
    """What must agree between the run that wrote a file and the run that reads it."""
    run = getattr(ppo, "_run", None)
    if run is None or getattr(ppo, "policy", None) is None:
        raise OlyError("ppo_checkpoint: PPO.train has not set this object up (its update path and rollout are chosen "
                       "there): take checkpoints with train(checkpoint_every=) and resume with train(resume=)")
    a_in, a_out = _dims(ppo.policy)
    c_in, c_out = _dims(ppo.critic)
    return dict(obs_dim=a_in, act_dim=a_out[-1] if a_out else 0, actor_hidden=a_out[:-1], critic_in=c_in,
                critic_hidden=c_out[:-1], num_envs=int(env.num_envs), T=int(run["T"]), max_traj_len=int(ppo.max_traj_len),
                update=run["update"], mirror=bool(run["mirror"]), device_permutation=bool(run["device_permutation"]),
                rollout=run["rollout"])


def _log_text(fn):
    try:
        with open(fn) as f:
            return f.read()
    except OSError:
        return None


def state_dict(ppo, env):
    """The run as it is now: clones on the device, nothing goes to the host until write().  Draws no random number and
    changes no tensor."""
    perm = getattr(ppo, "_next_perm", None)
    return dict(header=header(ppo, env),
                ppo=dict(iteration=int(ppo.iteration_count), total_steps=int(ppo.total_steps),
                         highest_reward=_number(ppo.highest_reward), curr_anneal=float(ppo.curr_anneal),
                         next_perm=None if perm is None else perm.clone()),
                policy=module_state(ppo.policy), critic=module_state(ppo.critic), optimiser=optimiser_state(ppo),
                env=env.state_dict() if hasattr(env, "state_dict") else None, rng=rng_state(env),
                logs=dict(train=_log_text(ppo.train_fn), eval=_log_text(ppo.eval_fn)))


def save(path, ppo, env, **meta):
    """Write the run (`ppo` inside or after train(), and the env it trains on); `meta` (numbers, strings, ...) is
    stored beside it and handed back by load."""
    return write(path, state_dict(ppo, env), **meta)


def load(path, ppo, env):
    """Read `path` into a run built like the saved one; returns the file's meta.  The header and every shape are compared
    before the first write."""
    obj = read(path)
    check_header(obj["header"], header(ppo, env))
    check_module(ppo.policy, obj["policy"], "policy")
    check_module(ppo.critic, obj["critic"], "critic")
    _check_optimiser(ppo, obj["optimiser"])
    dev = _cuda_device(env)
    if dev is not None:
        torch.cuda.synchronize(dev)                         # no queued work reads what is overwritten below
    if obj["env"] is not None:
        if not hasattr(env, "load_state_dict"):
            raise OlyError(f"ppo_checkpoint.load: the file holds an environment state, {type(env).__name__} has no "
                           "load_state_dict")
        env.load_state_dict(obj["env"])                     # checks its own sizes before it writes
    for m in (ppo.policy, getattr(ppo, "old_policy", None)):
        if m is not None:
            load_module(m, obj["policy"])
    load_module(ppo.critic, obj["critic"])
    _load_optimiser(ppo, obj["optimiser"])
    st = obj["ppo"]
    ppo.iteration_count, ppo.total_steps = int(st["iteration"]), int(st["total_steps"])
    ppo.highest_reward, ppo.curr_anneal = st["highest_reward"], float(st["curr_anneal"])
    ppo._next_perm = None if st["next_perm"] is None else st["next_perm"]
    restore_logs(ppo, obj["logs"])
    set_rng_state(obj["rng"], env)
    return obj["meta"]


def restore_logs(ppo, logs):
    """train.txt / eval.txt as they were at the save, so the curves continue (in a new directory too)."""
    for fn, text in ((ppo.train_fn, logs.get("train")), (ppo.eval_fn, logs.get("eval"))):
        if text is not None:
            os.makedirs(os.path.dirname(os.path.abspath(fn)), exist_ok=True)
            with open(fn, "w") as out:
                out.write(text)


def load_policy(path, policy, critic):
    """Weights and input-normalisation tables only (the reference's --continued): no optimiser state, no iteration, no
    random stream.  `path` may be a directory holding checkpoint.pt.  Returns the file's meta."""
    obj = read(resolve(path))
    check_module(policy, obj["policy"], "policy")
    check_module(critic, obj["critic"], "critic")
    load_module(policy, obj["policy"])
    load_module(critic, obj["critic"])
    return obj["meta"]
