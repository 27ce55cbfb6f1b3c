"""K24 without a GPU: the case table of tests/bc_restate.py held to its purpose (float32 against float64, the fit moves
every tensor, the saturated cases have teeth), the clip bounds, the argument checks of olympic_hip.bc and the C ABI
entries of oly_bc_*."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import bc_restate as br
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = br.TOL
K24_ENTRIES = ("oly_bc_fit_ws", "oly_bc_targets", "oly_bc_fit_steps")
IDS = [br.case_id(c) for c in br.CASES]


def test_the_table_is_the_issues():
    assert TOL == 2e-5
    got = [(c.in_dim, c.A, c.batch, c.n_rows, c.steps, c.standardizer, c.saturated) for c in br.CASES]
    assert got == [(1, 1, 1, 5, 4, True, False), (17, 6, 32, 100, 3, True, False), (17, 1, 7, 20, 4, True, True),
                   (33, 11, 33, 40, 3, True, True), (45, 12, 100, 250, 3, True, True), (64, 16, 256, 300, 3, False, True),
                   (32, 8, 40, 30, 3, True, False)]
    assert all(c.lr == 1e-3 for c in br.CASES)
    for c in br.CASES:
        k = br.build(c)
        assert k["idx"].shape == (c.steps, min(c.batch, c.n_rows)) and k["idx"].dtype == np.int32
        assert all(len(set(r.tolist())) == len(r) for r in k["idx"]), "rows within a step are distinct"
        assert 0 <= k["idx"].min() and k["idx"].max() < c.n_rows
        width = k["max_a"] - k["min_a"]
        assert c.A == 1 or np.ptp(width) > 0.1, "action bounds of unequal width"
        if c.saturated:
            t = k["targets"]
            on_hi, on_lo = np.mean(t == np.float32(np.arctanh(np.float64(br.CLIP)))), np.mean(t == -np.float32(np.arctanh(np.float64(br.CLIP))))
            assert 0.03 < on_hi < 0.25 and 0.03 < on_lo < 0.25, (on_lo, on_hi)
            assert k["params"][5][c.A] == -9.0
            assert c.A <= 1 or k["params"][5][c.A + 1] == 3.0
            assert c.A <= 2 or k["params"][5][c.A + 2] == -25.0


@pytest.mark.parametrize("c", br.CASES, ids=IDS)
def test_float32_restatement_lies_within_a_quarter_of_the_tolerance(c):
    k, ref = br.yardstick(c)
    f32 = br.restate(c, torch.float32, case=k)
    worst = 0.0
    for name, a, b in zip(("w1", "b1", "w2", "b2", "w3", "b3"), f32["params"][-1], ref["params"][-1]):
        d = float(np.abs(a - b).max())
        worst = max(worst, d)
        print(f"{br.case_id(c)} {name}: |f32 - f64| max {d:.3e}")
        assert d <= TOL / 4, (name, d)
    rel = float(np.abs(f32["out"][:, 0] - ref["out"][:, 0]).max() / np.abs(ref["out"][:, 0]).max())
    print(f"{br.case_id(c)} loss: relative {rel:.3e} (losses {ref['out'][:, 0]})")
    assert rel <= TOL / 4


@pytest.mark.parametrize("c", br.CASES, ids=IDS)
def test_the_fit_moves_every_tensor(c):
    k, ref = br.yardstick(c)
    for name, p0, p1 in zip(("w1", "b1", "w2", "b2", "w3", "b3"), k["params"], ref["params"][-1]):
        assert float(np.abs(p1 - p0.astype(np.float64)).max()) >= 10 * TOL, name
    assert np.all(np.isfinite(ref["out"]))


@pytest.mark.parametrize("c", [c for c in br.CASES if c.saturated], ids=[br.case_id(c) for c in br.CASES if c.saturated])
def test_saturated_cases_tell_the_gradient_under_the_variance_floor(c):
    """A reading that zeroes the log_sigma gradient where the variance lies under GaussianNLLLoss's floor misses the
    yardstick by 10 TOL on some tensor; and the case does reach the floor and both ends of the clamp."""
    k, ref = br.yardstick(c)
    wrong = br.restate(c, torch.float64, case=k, wrong=True)
    worst = max(float(np.abs(a - b).max()) for a, b in zip(wrong["params"][-1], ref["params"][-1]))
    assert worst >= 10 * TOL, worst
    # the raw log_sigma of the first minibatch at the initial parameters
    w1, b1, w2, b2, w3, b3 = (np.asarray(p, np.float64) for p in k["params"])
    x = k["states"][k["idx"][0]].astype(np.float64)
    if c.standardizer:
        x = br.Standardizer(c.in_dim)(x).astype(np.float64)
    h = np.maximum(np.maximum(x @ w1.T + b1, 0) @ w2.T + b2, 0)
    raw = (h @ w3.T + b3)[:, c.A:]
    assert np.any(np.exp(2 * raw) < br.NLL_EPS) and (c.A <= 1 or np.any(raw > br.LOG_STD_MAX))
    assert c.A <= 2 or np.any(raw < br.LOG_STD_MIN)


def test_clip_bounds_in_float32():
    hi = torch.clip(torch.tensor([2.0, -2.0, 0.25], dtype=torch.float32), -1.0 + 1e-7, 1.0 - 1e-7)
    assert hi[0].item() == float(np.float32(0.99999988)) == br.CLIP and hi[1].item() == -br.CLIP and hi[2].item() == 0.25
    assert br.CLIP == 1.0 - 2.0 ** -23
    t = br.targets_of(np.array([[3.0, -3.0]], np.float32), np.zeros(2, np.float32), np.ones(2, np.float32))
    assert abs(float(t[0, 0]) - 8.3177662) < 1e-6 and t[0, 1] == -t[0, 0]


# ------------------------------------------------------------------------------ the module's argument checks
def _fake_engine():
    return types.SimpleNamespace(device=torch.device("cpu"))


def _lins(in_dim=8, h1=512, h2=256, out=4):
    return [torch.nn.Linear(in_dim, h1), torch.nn.Linear(h1, h2), torch.nn.Linear(h2, out)]


def test_policy_argument_checks():
    from olympic_hip._ffi import OlyError
    from olympic_hip.bc import DeviceSquashedGaussianPolicy as P
    eng = _fake_engine()
    with pytest.raises(OlyError, match="three Linear"):
        P(eng, _lins()[:2], [-1, -1], [1, 1])
    with pytest.raises(OlyError, match="512 -> 256"):
        P(eng, _lins(h1=256), [-1, -1], [1, 1])
    with pytest.raises(OlyError, match="512 -> 256"):
        P(eng, _lins(in_dim=65), [-1, -1], [1, 1])
    with pytest.raises(OlyError, match="2A"):
        P(eng, _lins(out=5), [-1, -1], [1, 1])
    with pytest.raises(OlyError, match="2A"):
        P(eng, _lins(out=34), [-1] * 17, [1] * 17)           # A = 17 > 16
    with pytest.raises(OlyError, match="min_a / max_a"):
        P(eng, _lins(out=4), [-1, -1, -1], [1, 1, 1])
    with pytest.raises(OlyError, match="log_std_min"):
        P(eng, _lins(out=4), [-1, -1], [1, 1], log_std_min=3, log_std_max=2)


def test_trainer_argument_checks():
    from olympic_hip._ffi import OlyError
    from olympic_hip.bc import DeviceBehavioralCloning as BC, DeviceSquashedGaussianPolicy as P
    eng = _fake_engine()
    pol = object.__new__(P)
    pol.in_dim, pol.act_dim = 8, 2
    with pytest.raises(OlyError, match="must be a DeviceSquashedGaussianPolicy"):
        BC(eng, object(), dict(states=np.zeros((4, 8)), actions=np.zeros((4, 2))), 1e-3)
    with pytest.raises(OlyError, match="no 'actions'"):
        BC(eng, pol, dict(states=np.zeros((4, 8))), 1e-3)
    with pytest.raises(OlyError, match="actions"):
        BC(eng, pol, dict(states=np.zeros((4, 8)), actions=np.zeros((4, 3))), 1e-3)          # the wrong width
    with pytest.raises(OlyError, match="states"):
        BC(eng, pol, dict(states=np.zeros((4, 7)), actions=np.zeros((4, 2))), 1e-3)
    with pytest.raises(OlyError, match="action rows"):
        BC(eng, pol, dict(states=np.zeros((4, 8)), actions=np.zeros((5, 2))), 1e-3)
    with pytest.raises(OlyError, match="batch_size"):
        BC(eng, pol, dict(states=np.zeros((4, 8)), actions=np.zeros((4, 2))), 1e-3, batch_size=0)
    with pytest.raises(AttributeError, match="fit_offline"):
        object.__new__(BC).fit(None)
    import olympic_hip
    assert olympic_hip.DeviceBehavioralCloning is BC and olympic_hip.DeviceSquashedGaussianPolicy is P


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_declares_the_k24_entry_points():
    raw = _header()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in K24_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    assert int(re.search(r"#define OLY_BC_MAX_BATCH (\d+)", txt).group(1)) == _abi.OLY_BC_MAX_BATCH >= 1024
    assert int(re.search(r"#define OLY_BC_MAX_ACT (\d+)", txt).group(1)) == _abi.OLY_BC_MAX_ACT == 16
    k24 = raw[raw.index("K24 :"):]
    assert "behavioral_cloning.py:46-80" in k24 and "iq_sac.py" in k24 and "behavioral_cloning.py:63-66" in k24


def test_fit_struct_layout_matches_the_header(tmp_path):
    cls = _abi.BCFit
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             'printf("size %zu\\n", sizeof(oly_bc_fit));']
    lines += [f'printf("{f} %zu\\n", offsetof(oly_bc_fit, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    assert len(out) == len(cls._fields_) + 1
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_workspace_sizes_and_refusals():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    small, big = int(L.oly_bc_fit_ws(1, 32, 11)), int(L.oly_bc_fit_ws(4096, 64, 16))
    assert 0 < small < big and big == int(L.oly_bc_fit_ws(4096, 1, 1))
    # per row: 64 + 512 + 256 activations, 512 + 256 + 32 deltas; plus the transposed W2 and W3
    assert small >= 16 * 1632 + 256 * 512 + 32 * 256
    assert int(L.oly_bc_fit_ws(1024, 32, 11)) >= 1024 * 1632 + 256 * 512 + 32 * 256
    for bad in ((4097, 32, 11), (0, 32, 11), (-1, 32, 11), (32, 65, 11), (32, 0, 11), (32, 32, 17), (32, 32, 0)):
        assert int(L.oly_bc_fit_ws(*bad)) == -1, bad
    # a NULL context is refused before anything is read
    assert L.oly_bc_fit_steps(None, None, 1, None) == _abi.OLY_EINVAL
    assert L.oly_bc_targets(None, 0, 1, None, None, None, None, None) == _abi.OLY_EINVAL
