"""K20 without a GPU: the reference-run fixtures of _logging_sw (tests/golden/iter_log/, made by
tests/golden/gen_iter_log.py), the float64 restatement of tests/iter_log_restate.py held to them, and the C ABI of
oly_episode_stats / oly_iter_log / oly_trpo_old_offsets.

Tolerances (rs.tolerances): vf_loss, entropy and kl each four times the measured float32-fixture-versus-float64 spread,
relative to the value itself, with DESIGN section 13's floor of 1e-6; the episode means 1e-12 relative (float64 on both
sides); EpLenMean exact."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import iter_log_restate as rs
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K20_ENTRIES = ("oly_episode_stats", "oly_iter_log_ws_floats", "oly_iter_log", "oly_trpo_old_offsets")
_cache = {}


def restated(case, **kw):
    key = (case, tuple(sorted(kw.items())))
    if key not in _cache:
        args, g = rs.load_case(case)
        _cache[key] = (rs.restate_iter_log(**dict(args, **kw)), g, args)
    return _cache[key]


def spread_of(case):
    out, g, _ = restated(case)
    return rs.rel_err(out["scalars"][:6], g["values"])


@pytest.mark.parametrize("case", rs.CASES)
def test_fixture_is_the_reference_s_call(case):
    args, g = rs.load_case(case)
    import gen_iter_log as gen
    c = gen.CASES[case]
    assert os.path.getsize(rs.fixture(case)) < 16 << 10
    assert tuple(g["tags"]) == rs.NAMES == _abi.ITER_LOG_TAGS                      # the reference's tags in its order
    assert np.all(g["steps"] == int(g["iter"]) // 3) and int(g["iter"]) % 3 == 0
    n = c["T"] * c["N"]
    # the Standardizer took the batch twice; the old distribution was taken four batches earlier, on the copy
    assert float(g["st_count"][0]) - float(g["st0_count"][0]) == pytest.approx(2 * n, abs=1e-9)
    assert float(g["st0_count"][0]) - float(g["st_old_count"][0]) == pytest.approx(3 * n, abs=1e-9)
    assert float(g["st_old_count"][0]) == pytest.approx(c["prior_rows"] + 1e-2, abs=1e-9)
    assert int(g["episodes"]) >= 3
    assert abs(float(g["mean_length"]) % 1.0 - 0.5) > 0.01
    assert g["values"][2] == np.round(float(g["mean_length"]))
    assert 1e-3 <= g["values"][5] <= 1e-2                                            # kl of max_kl's order
    assert bool(args["last"][-1].all()) == c["close"]
    assert args["r_env"].dtype == (np.float64 if c["r64"] else np.float32)
    # the rebuilt old means are the reference's float32 tensor up to the float32 rounding of a forward
    assert np.abs(args["mu_old"][0] - g["mu_old_head"]).max() < 1e-5
    assert abs(float(args["mu_old"].sum(dtype=np.float64)) - float(g["mu_old_sum"])) < 1e-5 * n


@pytest.mark.parametrize("case", rs.CASES)
def test_restatement_reproduces_every_scalar(case):
    """The float32 fixture against float64: the spread per scalar is printed (DESIGN section 17 lists it) and sets the
    device tolerance."""
    out, g, _ = restated(case)
    spread = spread_of(case)
    tol = rs.tolerances(spread)
    for name, s, a, b, t in zip(rs.NAMES, spread, out["scalars"], g["values"], tol):
        print(f"{case} {name:14s} fixture {b:+.12e} restated {a:+.12e} spread {s:.2e} tolerance {t:.1e}")
    assert out["scalars"][2] == g["values"][2]
    assert np.all(spread[list(rs.EPISODE)] <= rs.EP_TOL)
    assert np.all(spread[3:] < 1e-3)                 # float32 against float64, not another formula
    assert out["scalars"][6] == pytest.approx(float(g["mean_length"]), rel=1e-15)
    assert out["scalars"][7] == int(g["episodes"])


@pytest.mark.parametrize("case", rs.CASES)
def test_restatement_reproduces_the_final_statistics(case):
    """The live statistics end two batches later; the float64 sums the device keeps are within the float32 rounding of the
    reference's float32 running sums."""
    out, g, args = restated(case)
    cs = out["colstats"]
    n = args["x"].shape[0]
    assert cs[0, 0] + 1e-2 == pytest.approx(float(g["st_count"][0]), rel=1e-12)
    assert cs[0, 0] - args["colstats"][0, 0] == 2 * n
    assert np.all(np.abs(cs[1] - g["st_sum"]) <= 2e-5 * np.maximum(1, np.abs(g["st_sum"])))
    assert np.all(np.abs(cs[2] + 1e-2 - g["st_sumsq"]) <= 2e-5 * np.abs(g["st_sumsq"]))


@pytest.mark.parametrize("reading", ("live", "policy_s1"))
@pytest.mark.parametrize("case", rs.CASES)
def test_wrong_readings_of_the_statistics_miss(case, reading):
    """Both forwards under S misses vf_loss and kl, the policy's forward under S + c misses kl: each by ten tolerances or
    more on both fixtures."""
    out, g, _ = restated(case, reading=reading)
    tol = rs.tolerances(spread_of(case))
    miss = rs.rel_err(out["scalars"][:6], g["values"]) / np.where(tol > 0, tol, 1.0)
    print(f"{case} {reading}: vf_loss misses by {miss[3]:.0f} tolerances, kl by {miss[5]:.0f}")
    assert miss[5] >= 10
    if reading == "live":
        assert miss[3] >= 10
    else:
        assert miss[3] <= 1


def test_counting_the_open_episode_among_the_lengths_misses():
    """Case b ends in an open episode: compute_J counts it, compute_episodes_length does not."""
    out, g, args = restated("b", count_open_length=True)
    assert out["scalars"][2] != g["values"][2]
    good = restated("b")[0]["scalars"]
    assert good[2] == g["values"][2] and out["scalars"][7] == good[7] + 1
    ep = rs.episode_stats(args["r_env"], args["last"])
    assert ep[3] == ep[4] + 1                                                      # one more return than lengths
    ea = rs.episode_stats(restated("a")[2]["r_env"], restated("a")[2]["last"])
    assert ea[3] == ea[4]


def test_episode_restatement_edge_cases():
    r = np.arange(1.0, 7.0).reshape(6, 1)
    none = np.zeros((6, 1), bool)
    e = rs.episode_stats(r, none)
    assert e[0] == 21.0 and e[3] == 1 and e[4] == 0 and np.isnan(e[2])           # one open episode: a return, no length
    e = rs.episode_stats(r, ~none)
    assert e[3] == e[4] == 6 and e[2] == 1.0 and e[0] == 3.5
    e = rs.episode_stats(r, none, gamma=0.5)
    assert e[0] == pytest.approx(sum(0.5 ** k * (k + 1) for k in range(6)), rel=1e-15)
    last = np.array([1, 0, 0, 1, 0, 1], bool).reshape(6, 1)
    e = rs.episode_stats(r, last, reward2=2 * r)
    assert e[3] == e[4] == 3 and e[7] == 6 and e[5] == 21.0 and e[6] == 42.0


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_abi_and_names_agree():
    from olympic_hip import il_agent
    raw = _header()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in K20_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    assert int(re.search(r"#define OLY_ITER_LOG_SCALARS (\d+)", txt).group(1)) == _abi.OLY_ITER_LOG_SCALARS == 8
    assert int(re.search(r"#define OLY_EPISODE_STATS (\d+)", txt).group(1)) == _abi.OLY_EPISODE_STATS == 8
    assert _abi.ITER_LOG_TAGS == rs.NAMES == il_agent.ITER_LOG_NAMES
    # the header documents the slots in the same order
    doc = dict((int(i), name) for i, name in re.findall(r"^ \*\s+\[(\d)\] (Ep[A-Za-z]+|vf_loss|entropy|kl)\b", raw, flags=re.M))
    assert [doc[i] for i in range(6)] == list(rs.NAMES)


def test_struct_layout_matches_the_header(tmp_path):
    cls, ctype = _abi.IterLog, "oly_iter_log_args"
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


def test_workspace_sizes_offsets_and_refusals():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    sizes = [int(L.oly_iter_log_ws_floats(n)) for n in (1, 300, 4096, 16384, 16385, 409600)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    # values and means are held for one chunk, not for n: beyond a chunk only the partial slots grow
    assert sizes[5] - sizes[3] < (409600 - 16384) // 16 and sizes[3] - sizes[0] >= (16384 - 4) * 32
    for bad in (0, -5):
        assert int(L.oly_iter_log_ws_floats(bad)) == -1
    # a NULL context is refused before anything is read
    assert L.oly_iter_log(None, None, None) == _abi.OLY_EINVAL
    assert L.oly_episode_stats(None, 1, 1, 0, 1.0, None, None, None, None, None) == _abi.OLY_EINVAL
    # the old distribution lies inside the step's workspace, 16-byte aligned, mu_old before theta_0
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    for n, D, A in ((1000, 32, 11), (1, 1, 1), (320, 64, 32)):
        assert L.oly_trpo_old_offsets(n, D, 512, 256, A, ctypes.byref(a), ctypes.byref(b)) == _abi.OLY_OK
        total, n_par = int(L.oly_trpo_ws_floats(n, D, 512, 256, A)), int(L.oly_trpo_param_count(D, 512, 256, A))
        assert 0 <= a.value and a.value % 4 == 0 and a.value + n * A <= b.value - (n_par - A)
        assert b.value + A <= total
    for bad in ((0, 32, 512, 256, 11), (10, 65, 512, 256, 11), (10, 32, 512, 256, 33), (10, 32, 256, 256, 11)):
        assert L.oly_trpo_old_offsets(*bad, ctypes.byref(a), ctypes.byref(b)) == _abi.OLY_EINVAL
    assert L.oly_trpo_old_offsets(10, 32, 512, 256, 11, None, ctypes.byref(b)) == _abi.OLY_EINVAL
