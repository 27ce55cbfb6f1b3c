"""K19 without a GPU: the reference-run fixtures of _discriminator_logging (tests/golden/disc_log/, made by
tests/golden/gen_disc_log.py), the float64 restatement of tests/disc_log_restate.py held to them, and the C ABI of
oly_gail_disc_log / oly_disc_log."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import disc_log_restate as rs
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K19_ENTRIES = ("oly_gail_disc_log_ws_floats", "oly_disc_log_ws_floats", "oly_gail_disc_log", "oly_disc_log")
_cache = {}


def restated(case, chain="sequence", stats="f64"):
    key = (case, chain, stats)
    if key not in _cache:
        args, g = rs.load_case(case)
        _cache[key] = (rs.restate_log(chain=chain, stats=stats, **args), g, args)
    return _cache[key]


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))


def fixture_scalars(g):
    """The recorded values in DISC_LOG_NAMES' order, zeros where the case has none."""
    v = np.zeros(12)
    v[:len(g["values"])] = g["values"]
    return v


@pytest.mark.parametrize("case", rs.CASES)
def test_fixture_is_the_reference_s_call(case):
    g = np.load(rs.fixture(case))
    vail = case.startswith("vail")
    assert os.path.getsize(rs.fixture(case)) < 1 << 20
    assert tuple(g["tags"]) == rs.NAMES[:12 if vail else 9]                     # the reference's tags in its order
    assert np.all(g["steps"] == int(g["iter"]) // 3)
    # the Standardizer took the batch four times (VAIL: five), with next states twice as often
    k = (5 if vail else 4) * (2 if case.endswith("_ns") else 1)
    assert float(g["st_count"][0]) - float(g["st0_count"][0]) == pytest.approx(k * 1280, abs=1e-9)
    assert float(g["st0_count"][0]) == pytest.approx(3000 + 1e-2, abs=1e-9)
    for i in rs.ACCURACIES:
        assert 0.2 < g["values"][i] < 0.8                                        # neither collapsed nor fooled: the step functions are live


@pytest.mark.parametrize("case", rs.CASES)
def test_no_logit_inside_the_band(case):
    out, _, _ = restated(case)
    inside = sum(int(np.sum(np.abs(d) < rs.BAND)) for d in out["logits"])
    assert inside == 0


@pytest.mark.parametrize("case", rs.CASES)
def test_restatement_reproduces_every_scalar(case):
    """The float32 fixture against float64: the spread per scalar is printed (DESIGN section 16 lists it), each scalar is
    within the tolerance the rule derives from it, and every spread is below a tenth of 2e-5, so that the device
    tolerance is the project's 2e-5 throughout.  Accuracies agree exactly."""
    out, g, _ = restated(case)
    want = fixture_scalars(g)
    spread = rel(out["scalars"], want)
    for name, s, a, b in zip(rs.NAMES, spread, out["scalars"], want):
        print(f"{case:8s} {name:48s} fixture {b:+.9e} restated {a:+.9e} spread {s:.2e}")
    for i in rs.ACCURACIES:
        assert out["scalars"][i] == want[i]
    assert np.all(spread <= rs.tolerances(spread))
    assert np.all(spread < rs.TOL / 10), spread
    if not case.startswith("vail"):
        assert np.all(out["scalars"][9:] == 0)


@pytest.mark.parametrize("case", rs.CASES)
def test_restatement_reproduces_the_final_statistics(case):
    """With the reference's own arithmetic for the running sums (float32 column sums into float32 sums) the chain of
    additions ends on the fixture's statistics to 1e-12 relative; the float64 sums the device keeps are within the
    float32 rounding of those."""
    out, g, _ = restated(case, stats="ref")
    st = out["stats"]
    assert st.count == pytest.approx(float(g["st_count"][0]), rel=1e-12)
    assert np.all(np.abs(st.sum - g["st_sum"]) <= 1e-12 * np.abs(g["st_sum"]))
    assert np.all(np.abs(st.sumsq - g["st_sumsq"]) <= 1e-12 * np.abs(g["st_sumsq"]))
    assert rel(out["scalars"], fixture_scalars(g)).max() < rs.TOL / 10
    cs = restated(case)[0]["colstats"]
    assert np.all(np.abs(cs[1] - g["st_sum"]) <= 2e-5 * np.maximum(1, np.abs(g["st_sum"])))
    assert np.all(np.abs(cs[2] + 1e-2 - g["st_sumsq"]) <= 2e-5 * np.abs(g["st_sumsq"]))


@pytest.mark.parametrize("chain", ("single", "all_each"))
@pytest.mark.parametrize("case", rs.CASES)
def test_wrong_readings_of_the_chain_miss(case, chain):
    """All forwards under S1, or the whole batch added once per forward whatever rows it evaluates: each misses at least
    one scalar of every fixture by ten tolerances or more."""
    out, g, _ = restated(case, chain=chain)
    want = fixture_scalars(g)
    good = rel(restated(case)[0]["scalars"], want)
    miss = rel(out["scalars"], want) / rs.tolerances(good)
    print(f"{case} {chain}: worst miss {miss.max():.1f} tolerances at {rs.NAMES[int(miss.argmax())]}")
    assert miss.max() >= 10


def test_the_six_statistics_differ_visibly():
    out, _, _ = restated("gail_s")
    means = [b[0][1] / (b[0][0] + 1e-2) for b in out["blocks"]]
    for a, b in zip(means, means[1:]):
        assert np.abs(a - b).max() > 1e-3
    ns = restated("gail_ns")[0]["blocks"]
    assert all(b[1][0, 0] - b[0][0, 0] > 0 for b in ns)                          # two blocks per forward with next states
    assert all(np.array_equal(b[0], b[1]) for b in out["blocks"])


def test_vail_dual_update_of_the_copy_shows():
    """The logging's copy of the VDBLoss moves its beta between the three loss evaluations (math.py:70,80-81): without
    that, Expert_Loss and Generator_loss miss the fixture."""
    for case in ("vail_s", "vail_sa"):
        args, g = rs.load_case(case)
        frozen = rs.restate_log(**dict(args, lr_beta=0.0))["scalars"]
        want = fixture_scalars(g)
        assert rel(frozen[7:9], want[7:9]).min() > 100 * rs.TOL
        assert rel(frozen[[0, 9, 10, 11]], want[[0, 9, 10, 11]]).max() < rs.TOL / 10


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_abi_and_names_agree():
    from olympic_hip import il_agent
    raw = _header()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in K19_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    assert int(re.search(r"#define OLY_DISC_LOG_SCALARS (\d+)", txt).group(1)) == _abi.OLY_DISC_LOG_SCALARS == 12
    assert _abi.DISC_LOG_TAGS == rs.NAMES
    assert il_agent.DISC_LOG_NAMES["gail"] == rs.NAMES[:9] and il_agent.DISC_LOG_NAMES["vail"] == rs.NAMES
    # the header documents the slots in the same order
    doc = re.findall(r"^ \*\s+(\d+) ([A-Za-z_.]+(?: Bernoulli Ent\.(?: Loss)?| Ent\.)?)", raw, flags=re.M)
    slots = {int(i): name for i, name in doc if int(i) < 12}
    for i, name in enumerate(rs.NAMES):
        assert name.startswith(slots[i]), (i, slots.get(i), name)


@pytest.mark.parametrize("cls,ctype", ((_abi.GailDiscLog, "oly_gail_disc_log_args"), (_abi.DiscLog, "oly_disc_log_args")))
def test_struct_layouts_match_the_header(tmp_path, cls, ctype):
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


def test_workspace_sizes_and_refusals():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    for fn, per_row in ((L.oly_gail_disc_log_ws_floats, 1), (L.oly_disc_log_ws_floats, 257)):
        sizes = [int(fn(n)) for n in (2, 300, 4096, 16384, 16385, 100000)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        # logits (and mu / logvar) are held for one chunk, not for n: beyond a chunk only the partial slots grow
        assert sizes[5] - sizes[3] < (100000 - 16384) // 2 and sizes[3] - sizes[0] >= (16384 - 4) * per_row
        for bad in (1, 0, -5):
            assert int(fn(bad)) == -1
    # a NULL context is refused before anything is read
    assert L.oly_gail_disc_log(None, None, None, None) == _abi.OLY_EINVAL
    assert L.oly_disc_log(None, None, None, None) == _abi.OLY_EINVAL
