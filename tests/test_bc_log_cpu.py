"""The logged fit and K25 without a GPU: the float64 restatement of tests/bc_log_restate.py against the reference-run
fixture tests/golden/bc_log/bc_log.npz (statistics, parameters, the four scalars; the two wrong readings miss it by the
margins the generator asserted), and the C ABI entries of oly_sg_act / oly_bc_fit_steps_log."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bc_log_restate as blr
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = blr.TOL
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
K25_ENTRIES = ("oly_sg_act", "oly_bc_fit_log_ws", "oly_bc_fit_steps_log")
_CACHE = {}


def fixture_runs(golden):
    """(fixture, case, generator module, {(logging_iter, reading): restatement}), computed once and shared."""
    if not _CACHE:
        g = golden("bc_log/bc_log.npz")
        k, gen = blr.fixture_case(g)
        runs = {}
        for li in (1, 2):
            for reading in ("true", "once", "prestep"):
                runs[li, reading] = blr.restate(gen.IN_DIM, gen.ACT_DIM, k, gen.N_STEPS, gen.LR, True, g[f"eps_li{li}"], li,
                                                once=reading == "once", prestep=reading == "prestep")
        _CACHE.update(g=g, k=k, gen=gen, runs=runs)
    return _CACHE["g"], _CACHE["k"], _CACHE["gen"], _CACHE["runs"]


def param_miss(run, g, li):
    return max(float(np.abs(a - g[f"{n}_li{li}"]).max()) for n, a in zip(NAMES, run["params"][-1]) if n != "w2")


def test_the_fixture_is_the_issues(golden):
    g, k, gen, _ = fixture_runs(golden)
    assert TOL == 2e-5 and (gen.N_ROWS, gen.IN_DIM, gen.ACT_DIM, gen.BATCH, gen.N_STEPS) == (200, 32, 11, 32, 6)
    assert list(g["logging_iters"]) == [1, 2] and g["idx"].shape == (6, 32)
    assert g["eps_li1"].shape == (6, 32, 11) and g["eps_li2"].shape == (3, 32, 11) and g["eps_li1"].dtype == np.float32
    assert g["st_count_li1"][0] == 0.01 + 2 * 6 * 32 and g["st_count_li2"][0] == 0.01 + 32 * (6 + 3)
    for li in (1, 2):
        s = g[f"scalars_li{li}"]
        logged = blr.logged_steps(6, li)
        assert s.shape == (6, 4) and np.all(np.isfinite(s[:, :3])) and np.all(np.isfinite(s[logged, 3]))
        assert np.all(np.isnan(np.delete(s[:, 3], logged)))
        assert float(g[f"sep_params_li{li}"]) >= 10 * TOL
    assert 0 < float(g["ent_spread"]) < 1e-5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "bc_log", "bc_log.npz")) < 1 << 20


@pytest.mark.parametrize("li", (1, 2))
def test_restatement_reproduces_the_reference_run(golden, li):
    g, k, gen, runs = fixture_runs(golden)
    r = runs[li, "true"]
    cs = r["colstats"]
    # the statistics, as tests/test_gpu_bc_fit.py compares them: the count exactly, the sums within TOL of their own size
    # (the reference sums the float32 minibatch in float32 before it adds to its float64 totals)
    assert np.all(cs[0] + 1e-2 == g[f"st_count_li{li}"][0])
    assert float(cs[0, 0]) + 1e-2 == (0.01 + 2 * 6 * 32 if li == 1 else 0.01 + 32 * (6 + 3))
    st_sum, st_sumsq = g[f"st_sum_li{li}"], g[f"st_sumsq_li{li}"]
    assert np.all(np.abs(cs[1] - st_sum) <= TOL * np.maximum(1, np.abs(st_sum)))
    assert np.all(np.abs(cs[2] + 1e-2 - st_sumsq) <= TOL * np.maximum(1, np.abs(st_sumsq)))
    miss = param_miss(r, g, li)
    print(f"logging_iter {li}: parameters |f64 - fixture| max {miss:.3e}")
    assert miss <= TOL
    s = g[f"scalars_li{li}"]
    rel = np.abs(r["out"][:, :3] - s[:, :3]) / np.abs(s[:, :3])
    assert rel.max() <= TOL, rel
    for step in range(gen.N_STEPS):
        if step in blr.logged_steps(gen.N_STEPS, li):
            err, tol = abs(r["out"][step, 3] - s[step, 3]), blr.ent_tol(s[step, 3], g["ent_spread"])
            print(f"logging_iter {li} step {step}: entropy {s[step, 3]:.6f}, |f64 - fixture| {err:.3e}, tolerance {tol:.3e}")
            assert err <= tol
        else:
            assert np.isnan(r["out"][step, 3])


@pytest.mark.parametrize("li", (1, 2))
def test_the_wrong_readings_miss_the_fixture(golden, li):
    """Rows added to the Standardizer once: the final parameters miss by 10 TOL and the count is short.  The logged
    forward with the weights before the step: a logged entropy misses by 10 tolerances."""
    g, k, gen, runs = fixture_runs(golden)
    once, pre = runs[li, "once"], runs[li, "prestep"]
    assert once["colstats"][0, 0] == 6 * 32 and once["colstats"][0, 0] + 1e-2 != g[f"st_count_li{li}"][0]
    miss = param_miss(once, g, li)
    print(f"logging_iter {li}: once-only reading misses the parameters by {miss / TOL:.1f} TOL")
    assert miss >= 10 * TOL
    s = g[f"scalars_li{li}"]
    logged = blr.logged_steps(gen.N_STEPS, li)
    ratio = max(abs(pre["out"][t, 3] - s[t, 3]) / blr.ent_tol(s[t, 3], g["ent_spread"]) for t in logged)
    print(f"logging_iter {li}: pre-step reading misses an entropy by {ratio:.1f} tolerances")
    assert ratio >= 10
    # ... and feeds the statistics as the true one does, so the parameters agree with the fixture
    assert param_miss(pre, g, li) <= TOL


@pytest.mark.parametrize("c", blr.PLAIN, ids=[__import__("bc_restate").case_id(c) for c in blr.PLAIN])
def test_plain_cases_are_well_conditioned(c):
    """The cases the device's entropy is held to float64 on: torch's float32 restatement lies within TOL / 4 of float64
    on every parameter and within a quarter of the entropy tolerance."""
    import bc_restate as br
    k = br.build(c)
    li = blr.logging_iter_of(c)
    eps = blr.noise(c, li)
    r64 = blr.restate(c.in_dim, c.A, k, c.steps, c.lr, c.standardizer, eps, li)
    r32 = blr.restate(c.in_dim, c.A, k, c.steps, c.lr, c.standardizer, eps, li, dtype=torch.float32)
    for name, a, b in zip(NAMES, r32["params"][-1], r64["params"][-1]):
        d = float(np.abs(a - b).max())
        print(f"{br.case_id(c)} {name}: |f32 - f64| max {d:.3e}")
        assert d <= TOL / 4, (name, d)
    g_spread = 6.6e-7      # the fixture's ent_spread to two digits; any value under TOL / 4 leaves the tolerance at TOL |v|
    for t in blr.logged_steps(c.steps, li):
        err, tol = abs(r32["out"][t, 3] - r64["out"][t, 3]), blr.ent_tol(r64["out"][t, 3], g_spread)
        assert err <= tol / 4, (t, err, tol)
    assert not c.saturated and np.abs(eps).max() <= 2.5
    assert [(c.in_dim, c.A, c.batch, c.standardizer) for c in blr.PLAIN] == [(c.in_dim, c.A, c.batch, c.standardizer) for c in blr.TABLED]


def test_logged_steps_and_noise():
    assert blr.logged_steps(6, 1) == list(range(6)) and blr.logged_steps(6, 2) == [0, 2, 4]
    assert blr.logged_steps(4, 2, iter0=1) == [1, 3] and blr.logged_steps(3, 5, iter0=1) == []
    from olympic_hip.engine import Engine
    assert Engine.bc_logged_steps(4, 2, 1) == [1, 3] and Engine.bc_logged_steps(6, 3, 0) == [0, 3]
    import bc_restate as br
    e = blr.noise(br.CASES[3], 2)
    assert e.shape == (2, 33, 11) and e.dtype == np.float32 and float(np.abs(e).max()) <= 2.5


def test_log_prob_is_torchs():
    rng = np.random.default_rng(0)
    mu, ls, eps = (torch.as_tensor(rng.standard_normal((9, 5))) for _ in range(3))
    ls = 0.3 * ls
    a_raw = mu + ls.exp() * eps
    want = torch.distributions.Normal(mu, ls.exp()).log_prob(a_raw).sum(1) - torch.log(1 - torch.tanh(a_raw) ** 2 + 1e-6).sum(1)
    assert torch.allclose(blr.log_prob(mu, ls, a_raw), want, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_declares_the_k25_entry_points():
    raw = _header()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in K25_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8, "additive: no bump"
    k25 = raw[raw.index("K25 :"):]
    assert "iq_sac.py:102-151" in k25 and "behavioral_cloning.py:82-94" in k25
    assert _abi.BC_LOG_TAG_EMPIRICAL == "Squashed Gaussian Entropy (Empirical)"


@pytest.mark.parametrize("cname,cls", (("oly_sg_act_args", _abi.SGAct), ("oly_bc_fit_log", _abi.BCFitLog)))
def test_struct_layouts_match_the_header(tmp_path, cname, cls):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             f'printf("size %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_workspace_sizes_and_null_refusals():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    for b in (1, 32, 33, 4096):
        assert int(L.oly_bc_fit_log_ws(b, 32, 11)) == int(L.oly_bc_fit_ws(b, 32, 11)) + (b + 15) // 16 * 16
    for bad in ((4097, 32, 11), (0, 32, 11), (32, 65, 11), (32, 32, 17), (32, 32, 0)):
        assert int(L.oly_bc_fit_log_ws(*bad)) == -1, bad
    assert L.oly_sg_act(None, None, None) == _abi.OLY_EINVAL
    assert L.oly_bc_fit_steps_log(None, None, 1, None) == _abi.OLY_EINVAL


def test_host_flags_default_off():
    import inspect
    from olympic_hip.bc import DeviceBehavioralCloning, DeviceSquashedGaussianPolicy
    assert inspect.signature(DeviceSquashedGaussianPolicy.__init__).parameters["fused_act"].default is False
    assert inspect.signature(DeviceBehavioralCloning.__init__).parameters["empirical_entropy"].default is False
    assert inspect.signature(DeviceBehavioralCloning.fit_offline).parameters["eps"].default is None
