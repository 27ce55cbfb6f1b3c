"""K21 and the launcher's loop without a GPU: the C ABI of oly_il_act, and ILCore.learn / ILCore.evaluate driven by CPU
fakes (a deterministic environment, a policy that echoes a column, an agent that records what fit gets).

The fake environment's observation is (environment id, episode number, step in episode); environment e ends an episode
every 2 + e steps, the odd-numbered episodes in an absorbing state, and pays 1 + e per step.  Every expected value below
follows from that in closed form."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ C ABI
def test_header_abi_and_names_agree():
    raw = open(os.path.join(ROOT, "include", "olympic_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\boly_il_act\s*\(", txt)
    assert "oly_il_act" in _abi.SIGNATURES
    assert re.search(r"\}\s*oly_il_act_args\s*;", txt)
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8


def test_struct_layout_matches_the_header(tmp_path):
    cls, ctype = _abi.ILAct, "oly_il_act_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             f'printf("size %zu\\n", sizeof({ctype}));']
    lines += [f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    assert len(out) == len(cls._fields_) + 1
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_library_exports_the_entry_and_refuses_a_null_context():
    """The argument refusals need a context, hence a device: they are in tests/test_gpu_il_act.py."""
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    assert int(L.oly_abi_version()) == 8
    assert L.oly_il_act(None, None, None) == _abi.OLY_EINVAL
    f = _abi.ILAct(n=4, in_dim=32, act_dim=11)
    assert L.oly_il_act(None, ctypes.byref(f), None) == _abi.OLY_EINVAL


# ------------------------------------------------------------------------------ fakes
class FakeEnv:
    def __init__(self, N, horizon=10, gamma=0.5, needs_ctrl=False):
        self.num_envs = N
        self.info = SimpleNamespace(horizon=horizon, gamma=gamma)
        self.physics = SimpleNamespace(needs_ctrl=needs_ctrl)
        self.ids = torch.arange(N)
        self.ep, self.k = torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
        self.n_steps, self.full_resets, self.masked_resets, self.ctrls = 0, 0, 0, []

    def _obs(self):
        return torch.stack([self.ids, self.ep, self.k], 1).to(torch.float64)

    def reset(self, env_mask=None):
        if env_mask is None:
            self.full_resets += 1
            self.ep.zero_()
            self.k.zero_()
        else:
            assert env_mask.dtype == torch.bool and bool(env_mask.any())
            self.masked_resets += 1
            self.ep[env_mask] += 1
            self.k[env_mask] = 0
        return self._obs()

    def step(self, actions, ctrl=None):
        assert tuple(actions.shape) == (self.num_envs, 1)
        self.ctrls.append(ctrl)
        self.n_steps += 1
        self.k += 1
        last = self.k >= 2 + self.ids
        absorbing = last & (self.ep % 2 == 1)
        return self._obs(), (1.0 + self.ids).to(torch.float32), absorbing, dict(last=last)


class FakePolicy:
    def __init__(self):
        self.calls = []

    def act(self, obs, generator=None, eps=None, deterministic=False, ctrl=False):
        self.calls.append(bool(ctrl))
        a = obs[:, :1].to(torch.float32)
        return a, (a * 2 if ctrl else None)


class FakeAgent:
    def __init__(self):
        self.fits = []

    def fit(self, dataset, generator=None):
        self.fits.append({k: v.clone() for k, v in dataset.items()})
        return len(self.fits)


def expected_learn(N, T0, T):
    """The six blocks of vec steps T0 .. T0 + T - 1 from the closed form."""
    st, nx = np.zeros((T, N, 3)), np.zeros((T, N, 3))
    last, ab = np.zeros((T, N), bool), np.zeros((T, N), bool)
    for e in range(N):
        L = 2 + e
        for t in range(T):
            g = T0 + t
            ep, k = g // L, g % L
            st[t, e], nx[t, e] = (e, ep, k), (e, ep, k + 1)
            last[t, e] = k + 1 == L
            ab[t, e] = last[t, e] and ep % 2 == 1
    return st, nx, last, ab


def test_learn_blocks_resets_and_hand_over():
    env, pol, agent = FakeEnv(3), FakePolicy(), FakeAgent()
    core = ILCore(agent, env, pol, episode_stats=rs.episode_stats)
    assert core.learn(n_steps=12, n_steps_per_fit=6) == [1, 2]
    assert len(agent.fits) == 2 and env.n_steps == 12 and env.full_resets == 1
    for i, d in enumerate(agent.fits):
        st, nx, last, ab = expected_learn(3, 6 * i, 6)          # the second fit continues the first one's episodes
        assert set(d) == {"state", "action", "reward", "next_state", "absorbing", "last"}
        assert tuple(d["state"].shape) == tuple(d["next_state"].shape) == (6, 3, 3)
        assert tuple(d["action"].shape) == (6, 3, 1) and tuple(d["reward"].shape) == (6, 3)
        assert np.array_equal(d["state"].numpy(), st)
        assert np.array_equal(d["next_state"].numpy(), nx)         # the pre-reset observation at every last
        assert np.array_equal(d["absorbing"].numpy(), ab) and ab.any() and (last & ~ab).any()
        assert np.array_equal(d["action"].numpy()[..., 0], st[..., 0])
        assert np.array_equal(d["reward"].numpy(), np.broadcast_to(1.0 + np.arange(3), (6, 3)))
        handed = last.copy()
        handed[-1] = True
        assert np.array_equal(d["last"].numpy(), handed) and (i == 1 or not last[-1].all())
        # state[t+1] is the post-reset observation where last[t], next_state[t] elsewhere
        s, n = d["state"].numpy(), d["next_state"].numpy()
        m = last[:-1]
        assert np.array_equal(s[1:][~m], n[:-1][~m])
        assert np.all(s[1:][m][:, 2] == 0) and np.array_equal(s[1:][m][:, 1], n[:-1][m][:, 1] + 1)
        assert d["state"].data_ptr() != d["next_state"].data_ptr()
    # the core's own copy keeps `last` as the environment reported it
    assert np.array_equal(core.blocks["last"].numpy(), expected_learn(3, 6, 6)[2])
    # a later call continues the running episodes
    core.learn(6, 6)
    assert env.full_resets == 1 and np.array_equal(agent.fits[2]["state"].numpy(), expected_learn(3, 12, 6)[0])
    assert pol.calls == [False] * 18 and all(c is None for c in env.ctrls)


def test_learn_refuses_a_ragged_step_count():
    env, agent = FakeEnv(3), FakeAgent()
    core = ILCore(agent, env, FakePolicy(), episode_stats=rs.episode_stats)
    with pytest.raises(OlyError):
        core.learn(n_steps=7, n_steps_per_fit=6)
    assert env.n_steps == 0 and not agent.fits


def test_learn_hands_the_controls_to_a_physics_that_needs_them():
    env, pol = FakeEnv(2, needs_ctrl=True), FakePolicy()
    ILCore(FakeAgent(), env, pol, episode_stats=rs.episode_stats).learn(3, 3)
    assert pol.calls == [True] * 3
    assert all(c is not None and tuple(c.shape) == (2, 1) for c in env.ctrls)


def geo(r, n, g):
    return sum(r * g ** k for k in range(n))


@pytest.mark.parametrize("n_episodes,N", [(5, 3), (2, 4)])
def test_evaluate_quotas_and_means(n_episodes, N):
    quota = [n_episodes // N + (e < n_episodes % N) for e in range(N)]
    assert quota == ([2, 2, 1] if N == 3 else [1, 1, 0, 0])
    R = sum(q * (1 + e) * (2 + e) for e, q in enumerate(quota)) / n_episodes
    J = sum(q * geo(1 + e, 2 + e, 0.5) for e, q in enumerate(quota)) / n_episodes
    steps = sum(q * (2 + e) for e, q in enumerate(quota))
    out = {}
    for poll in (1, 32):
        env = FakeEnv(N, horizon=10, gamma=0.5)
        core = ILCore(FakeAgent(), env, FakePolicy(), episode_stats=rs.episode_stats)
        out[poll] = core.evaluate(n_episodes, poll=poll)
        assert env.full_resets == 1
        assert env.n_steps <= max(quota) * 10                         # the step bound
        if poll == 1:
            assert env.n_steps == max(q * (2 + e) for e, q in enumerate(quota))
    o = out[1]
    assert out[1] == out[32]
    assert set(o) == {"R_mean", "J_mean", "L", "n_episodes", "n_steps"}
    assert o["n_episodes"] == n_episodes and o["n_steps"] == steps
    assert o["R_mean"] == pytest.approx(R, rel=1e-15)
    assert o["J_mean"] == pytest.approx(J, rel=1e-15)
    assert o["L"] == pytest.approx(steps / n_episodes, rel=1e-15)
    assert (R, J, steps / n_episodes) == ((5.6, 3.125, 2.8) if N == 3 else (4.0, 2.5, 2.5))   # by hand


def test_evaluate_blocks_zero_the_rows_past_the_quota():
    env = FakeEnv(3, horizon=10, gamma=0.5)
    core = ILCore(FakeAgent(), env, FakePolicy(), episode_stats=rs.episode_stats)
    o, b = core.evaluate(5, poll=32, return_blocks=True)
    r, last = b["reward"].numpy(), b["last"].numpy()
    assert r.shape == last.shape == (6, 3)                            # cut where the slowest quota was met
    assert b["reward_raw"].shape[0] == 20                             # poll 32 ran to the bound
    assert last.sum(0).tolist() == [2, 2, 1]
    assert np.all(r[4:, 0] == 0) and np.all(r[:4, 0] == 1) and np.all(r[:, 1] == 2) and np.all(r[4:, 2] == 0)
