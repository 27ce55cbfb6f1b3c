"""Checkpoints of the imitation-learning agent and the launcher's BestAgentSaver
(examples/imitation_learning/experiment.py:39,65,67; imitation_lib/utils/training.py:8-52).

    agent_saver = BestAgentSaver(save_path, n_epochs_save)        -> BestAgentSaver
    agent_saver.save(core.agent, J_mean)                          -> BestAgentSaver.save(agent, J, core=None)
    agent_saver.save_curr_best_agent()                            -> BestAgentSaver.save_curr_best_agent()
    Agent.load(path) of the evaluation scripts                    -> load(path, agent, core=None) / agent.load(path)

A checkpoint is ONE file written by torch.save: a nested dict of host tensors, Python numbers, strings, lists and None,

    dict(format="olympic_hip.il_checkpoint", version=1, agent=agent.state_dict(), core=core.state_dict() or None, meta=meta)

and is read with torch.load(path, map_location="cpu", weights_only=True) and nothing else: no object is ever unpickled from
a file (the reference's Agent.load unpickles the whole agent).  A file that would need one is refused.

Stated differences from the reference: the demonstrations are NOT stored (the reference pickles them under full_save=True,
gail_TRPO.py:91): an agent is built with its demonstrations like any other and then loaded into; what the saver holds
between the epoch of the best J and the write is agent.state_dict() (clones on the device), where the reference holds a
deepcopy of the agent; the file names end in .pt, not .msh.

Nothing here runs per step and nothing here launches a kernel of its own; the module imports without the shared library.
"""
import os
import pickle

import torch

from ._ffi import OlyError

FORMAT, VERSION = "olympic_hip.il_checkpoint", 1


def to_host(state):
    """A state_dict's nest with every tensor moved to the host (a copy; the rest as it is)."""
    if torch.is_tensor(state):
        return state.detach().cpu()
    if isinstance(state, dict):
        return {k: to_host(v) for k, v in state.items()}
    if isinstance(state, (list, tuple)):
        return [to_host(v) for v in state]
    if state is None or isinstance(state, (bool, int, float, str)):
        return state
    raise OlyError(f"il_checkpoint: a state_dict holds tensors, numbers, strings, lists, dicts and None, not "
                   f"{type(state).__name__}")


def write_file(path, obj):
    """torch.save of a nest of host values (to_host's output) under `path`: written beside it as .part and renamed, so
    the name never shows a half-written file and a previous file of that name is replaced in one step."""
    path = os.fspath(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".part"
    torch.save(obj, tmp)
    os.replace(tmp, path)
    return path


def read_file(path, fmt, version, who="il_checkpoint.load"):
    """The content of a file written by write_file, read with weights_only=True and checked for its format name and
    version (`who` opens the messages: ppo_checkpoint reads its files through here as well)."""
    try:
        obj = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        raise OlyError(f"{who}: {path} is not a checkpoint of tensors, numbers and strings: reading it "
                       f"would unpickle an object, which is refused ({str(e).splitlines()[0]})") from None
    if not isinstance(obj, dict) or obj.get("format") != fmt:
        got = obj.get("format") if isinstance(obj, dict) else type(obj).__name__
        raise OlyError(f"{who}: {path}: format is {got!r}, expected {fmt!r}")
    if obj.get("version") != version:
        raise OlyError(f"{who}: {path}: version is {obj.get('version')!r}, this reader takes {version!r}")
    return obj


def save_state(path, agent_state, core_state=None, **meta):
    """Write state_dicts that were taken earlier (BestAgentSaver's snapshot).  The file appears under its name only once
    it is complete."""
    obj = dict(format=FORMAT, version=VERSION, agent=to_host(agent_state),
               core=None if core_state is None else to_host(core_state), meta=to_host(meta))
    return write_file(path, obj)


def save(path, agent, core=None, **meta):
    """Write the agent (and, to resume a run, its ILCore: the environment, the observation and the random stream) as
    they are now; `meta` (numbers, strings, ...) is stored beside them and handed back by load."""
    return save_state(path, agent.state_dict(), None if core is None else core.state_dict(), **meta)


def read(path):
    """The checked content of a checkpoint file: dict(format, version, agent, core, meta), tensors on the host."""
    return read_file(path, FORMAT, VERSION)


def load(path, agent, core=None):
    """Read `path` into an agent (and core) built like the saved ones; returns the file's meta.  Everything is written
    in place by the objects' load_state_dict; a structural mismatch raises OlyError naming the field and both values."""
    obj = read(path)
    if core is not None and obj["core"] is None:
        raise OlyError(f"il_checkpoint.load: {path} holds no core state (it was saved without core=), so a run cannot "
                       "be resumed from it; load the agent alone")
    agent.load_state_dict(obj["agent"])
    if core is not None:
        core.load_state_dict(obj["core"])
    return obj["meta"]


class BestAgentSaver:
    """The reference's BestAgentSaver (imitation_lib/utils/training.py:8-52), its schedule kept as it is:

    save(agent, J): unless n_epochs_save == -1, a snapshot is taken when J exceeds the best since the last write (a tie
    does not), the held snapshot is written when last_save + n_epochs_save <= epoch_counter, and then the epoch counter
    advances.  The test runs before the counter advances, so with n_epochs_save = 1 the first call writes nothing and a
    write lags its snapshot by one call; a write also forgets the best J, AFTER that call's own J was compared, so
    the J of a call that writes an older snapshot is never kept (J = 1, .5: epoch 0 is written in the second call and
    epoch 1 is lost).

    A snapshot is agent.state_dict() (and core.state_dict() when a core is given, which makes the file resumable):
    clones on the device, nothing goes to the host until the write.  The file therefore holds the agent of the epoch of
    its J, not the agent at the time of the write (the reference's deepcopy).  J is the host number ILCore.evaluate
    returns, so the comparison synchronises nothing."""

    def __init__(self, save_path, n_epochs_save=10):
        self.best_curr_agent = None
        self.save_path = save_path
        self.n_epochs_save = n_epochs_save
        self.last_save = 0
        self.epoch_counter = 0
        self.best_J_since_last_save = -float("inf")

    def save(self, agent, J, core=None):
        if self.n_epochs_save != -1:
            if J > self.best_J_since_last_save:
                self.best_J_since_last_save = J
                self.best_curr_agent = (agent.state_dict(), None if core is None else core.state_dict(), J,
                                        self.epoch_counter)
            written = None
            if self.last_save + self.n_epochs_save <= self.epoch_counter:
                written = self.save_curr_best_agent()
            self.epoch_counter += 1
            return written
        return None

    def save_curr_best_agent(self):
        """Write the held snapshot to agent_epoch_%d_J_%f.pt and forget it; returns the path, or None without one."""
        if self.best_curr_agent is None:
            return None
        agent_state, core_state, J, epoch = self.best_curr_agent
        path = os.path.join(self.save_path, "agent_epoch_%d_J_%f.pt" % (epoch, J))
        save_state(path, agent_state, core_state, epoch=int(epoch), J=float(J))
        self.best_curr_agent = None
        self.best_J_since_last_save = -float("inf")
        self.last_save = self.epoch_counter
        return path

    def save_agent(self, agent, J, core=None):
        """Write the agent as it is now to agent_J_%f.pt."""
        path = os.path.join(self.save_path, "agent_J_%f.pt" % J)
        return save(path, agent, core, J=float(J))
