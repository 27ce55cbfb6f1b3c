"""K22 and ILCore's device-reset path without a GPU: the C ABI of oly_il_reset_where, and ILCore driven by CPU fakes.

The fake environments are test_il_core_cpu.py's closed form: the observation is (environment id, episode number, step
in episode), environment e ends an episode every 2 + e steps.  DeviceFakeEnv adds reset_where(mask), written with
torch.where only, and reports `last` as a tensor subclass that raises when it is converted to a Python bool or reduced
with any(): the device path may not ask the host whether an episode ended."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import iter_log_restate as rs
from olympic_hip import _abi
from olympic_hip._ffi import OlyError
from olympic_hip.il_core import ILCore
from test_il_core_cpu import FakeAgent, FakeEnv, FakePolicy, expected_learn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ C ABI
def test_header_abi_and_names_agree():
    raw = open(os.path.join(ROOT, "include", "olympic_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\boly_il_reset_where\s*\(", txt)
    assert "oly_il_reset_where" in _abi.SIGNATURES
    assert re.search(r"\}\s*oly_il_reset_args\s*;", txt)
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    # the header comment cites the reference lines the entry point replaces
    block = raw[raw.index("K22 :"):raw.index("typedef struct oly_il_reset_args")]
    for cite in ("loco_env_base.py:568-657", "loco_env_base.py:659-684", "utils/trajectory.py:289-323",
                 "loco_env_base.py:584"):
        assert cite in block, cite


def test_struct_layout_matches_the_header(tmp_path):
    cls, ctype = _abi.ILReset, "oly_il_reset_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             f'printf("size %zu\\n", sizeof({ctype}));']
    lines += [f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 8 + 15 * 8
    assert len(out) == len(cls._fields_) + 1
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f
    # every member of the C struct is mirrored: the header's member names, in order
    raw = open(os.path.join(ROOT, "include", "olympic_hip.h")).read()
    body = raw[raw.index("typedef struct oly_il_reset_args"):raw.index("} oly_il_reset_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [f for f, _ in cls._fields_]


def test_library_exports_the_entry_and_refuses_a_null_context():
    """The argument refusals need a context, hence a device: they are in tests/test_gpu_il_reset.py."""
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    assert int(L.oly_abi_version()) == 8
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH], text=True)
    assert re.search(r" T oly_il_reset_where\b", out)
    assert L.oly_il_reset_where(None, None, None) == _abi.OLY_EINVAL
    f = _abi.ILReset(n=4)
    assert L.oly_il_reset_where(None, ctypes.byref(f), None) == _abi.OLY_EINVAL


# ------------------------------------------------------------------------------ fakes
class NoHostRead(torch.Tensor):
    """`last` as the device path may use it: element-wise operations pass, asking the host for its truth does not."""

    @staticmethod
    def wrap(t):
        return t.as_subclass(NoHostRead)

    def __bool__(self):
        raise AssertionError("the device path converted `last` to a Python bool")

    def any(self, *a, **k):
        raise AssertionError("the device path reduced `last` with any()")

    def item(self):
        raise AssertionError("the device path read `last` back")


class DeviceFakeEnv(FakeEnv):
    """FakeEnv with reset_where.  reset(env_mask=) is refused: the device path may not call it."""

    def __init__(self, N, device_state=True, guard_last=True, **kw):
        super().__init__(N, **kw)
        self.guard_last = guard_last
        self.physics = SimpleNamespace(needs_ctrl=False, device_state=device_state)
        self.where_calls = []

    def reset(self, env_mask=None):
        assert env_mask is None, "reset(env_mask=) called on the device path"
        return super().reset()

    def step(self, actions, ctrl=None):
        obs, r, ab, info = super().step(actions, ctrl)
        return obs, r, ab, dict(last=NoHostRead.wrap(info["last"]) if self.guard_last else info["last"])

    def reset_where(self, mask, traj_no=None, step=None, generator=None):
        assert isinstance(mask, NoHostRead) or not self.guard_last
        m = torch.Tensor.as_subclass(mask, torch.Tensor)
        self.where_calls.append(m.clone())
        before = self._obs()
        self.ep = torch.where(m, self.ep + 1, self.ep)
        self.k = torch.where(m, torch.zeros_like(self.k), self.k)
        out = self._obs()
        assert torch.equal(out[~m], before[~m])
        return out


def test_no_host_read_really_raises():
    t = NoHostRead.wrap(torch.tensor([True, False]))
    for f in (bool, lambda x: x.any(), lambda x: x.item()):
        with pytest.raises(AssertionError):
            f(t)
    assert isinstance(t.clone(), torch.Tensor) and t.to(torch.int64).tolist() == [1, 0]


def check_fit_blocks(agent, N, T):
    for i, d in enumerate(agent.fits):
        st, nx, last, ab = expected_learn(N, T * i, T)
        assert np.array_equal(d["state"].numpy(), st)
        assert np.array_equal(d["next_state"].numpy(), nx)         # the pre-reset observation at every last
        assert np.array_equal(d["absorbing"].numpy(), ab)
        handed = last.copy()
        handed[-1] = True
        assert np.array_equal(d["last"].numpy(), handed)
        s, n = d["state"].numpy(), d["next_state"].numpy()
        m = last[:-1]
        assert m.any() and (~m).any()
        assert np.array_equal(s[1:][~m], n[:-1][~m])               # no reset: state[t+1] is next_state[t]
        assert np.all(s[1:][m][:, 2] == 0) and np.array_equal(s[1:][m][:, 1], n[:-1][m][:, 1] + 1)   # post-reset
        assert d["state"].data_ptr() != d["next_state"].data_ptr()


@pytest.mark.parametrize("device_reset", [None, True])
def test_device_path_never_asks_the_host(device_reset):
    env, pol, agent = DeviceFakeEnv(3), FakePolicy(), FakeAgent()
    core = ILCore(agent, env, pol, episode_stats=rs.episode_stats, device_reset=device_reset)
    assert core.device_reset is True
    assert core.learn(n_steps=12, n_steps_per_fit=6) == [1, 2]
    assert env.n_steps == 12 and env.full_resets == 1 and env.masked_resets == 0
    assert len(env.where_calls) == 12                              # every vec step, whether or not anything ended
    want_last = np.concatenate([expected_learn(3, 0, 6)[2], expected_learn(3, 6, 6)[2]])
    assert np.array_equal(torch.stack(env.where_calls).numpy(), want_last)
    assert not want_last[0].any()                                  # a step on which nothing ended was passed on too
    check_fit_blocks(agent, 3, 6)
    assert np.array_equal(core.blocks["last"].numpy(), expected_learn(3, 6, 6)[2])


def test_device_path_evaluate_matches_the_host_path():
    """evaluate keeps its completion poll, which reads a count derived from `last`: a plain tensor here."""
    outs = {}
    for name, env in (("host", FakeEnv(3, horizon=10, gamma=0.5)),
                      ("device", DeviceFakeEnv(3, horizon=10, gamma=0.5, guard_last=False))):
        core = ILCore(FakeAgent(), env, FakePolicy(), episode_stats=rs.episode_stats)
        assert core.device_reset is (name == "device")
        outs[name] = core.evaluate(5, poll=1)
        assert env.masked_resets == 0 or name == "host"
    assert outs["host"] == outs["device"] and outs["device"]["n_episodes"] == 5


def test_device_reset_true_needs_the_method_and_the_attribute():
    with pytest.raises(OlyError, match="reset_where"):
        ILCore(FakeAgent(), FakeEnv(3), FakePolicy(), episode_stats=rs.episode_stats, device_reset=True)
    with pytest.raises(OlyError, match="device_state"):
        ILCore(FakeAgent(), DeviceFakeEnv(3, device_state=False), FakePolicy(), episode_stats=rs.episode_stats,
               device_reset=True)
    # None falls back to the host path for both
    assert ILCore(FakeAgent(), FakeEnv(3), FakePolicy(), episode_stats=rs.episode_stats).device_reset is False
    env = DeviceFakeEnv(3, device_state=False)
    assert ILCore(FakeAgent(), env, FakePolicy(), episode_stats=rs.episode_stats).device_reset is False


def test_device_reset_false_reproduces_the_old_call_sequence():
    """On an environment that has both methods, device_reset=False is the host path: reset(env_mask=) exactly on the
    steps with an ended episode, never reset_where, and the same blocks."""

    class Both(FakeEnv):
        def __init__(self, N):
            super().__init__(N)
            self.physics = SimpleNamespace(needs_ctrl=False, device_state=True)
            self.log = []

        def reset(self, env_mask=None):
            self.log.append("reset" if env_mask is None else ("masked", env_mask.tolist()))
            return super().reset(env_mask)

        def step(self, actions, ctrl=None):
            self.log.append("step")
            return super().step(actions, ctrl)

        def reset_where(self, mask, **kw):
            raise AssertionError("reset_where called with device_reset=False")

    env, agent = Both(3), FakeAgent()
    ILCore(agent, env, FakePolicy(), episode_stats=rs.episode_stats, device_reset=False).learn(12, 6)
    last = np.concatenate([expected_learn(3, 0, 6)[2], expected_learn(3, 6, 6)[2]])
    want = ["reset"]
    for t in range(12):
        want.append("step")
        if last[t].any():
            want.append(("masked", last[t].tolist()))
    assert env.log == want and env.masked_resets == int(last.any(1).sum())
    check_fit_blocks(agent, 3, 6)
