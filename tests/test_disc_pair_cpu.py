"""The paired discriminator inputs, (s, s') and (s, a), without a GPU: the four reference-run fixtures of
tests/golden/disc_pair_fit/, the float64 restatement of tests/pair_restate.py held to them, the rule they pin (two
Standardizer updates per forward in next-state mode), the C ABI of the oly_*_pair entry points and the refusals that
need no device."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import pair_restate as pr
from olympic_hip import _abi

gen = pr.gen
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 2e-5            # the device tolerance per tensor (tests/il_shapes.py)
PAIR_ENTRIES = ("oly_disc_forward_pair", "oly_disc_reward_step_pair", "oly_disc_fit_pair_ws_floats",
                "oly_disc_fit_epoch_pair", "oly_gail_disc_forward_pair", "oly_gail_reward_step_pair",
                "oly_gail_disc_fit_pair_ws_floats", "oly_gail_disc_fit_epoch_pair")
NS_CASES = tuple(c for c in pr.CASES if pr.case_standardise(c))


def _reference_dir():
    import _ref_stubs
    return _ref_stubs.REF


@pytest.mark.skipif(not os.path.isdir(_reference_dir()), reason="the reference tree is only in the build container")
def test_fixtures_regenerate_byte_for_byte(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "gen_disc_pair_fit.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONHASHSEED="random"))
    assert r.returncode == 0, r.stderr[-2000:]
    for case in pr.CASES:
        a, b = np.load(pr.fixture(case)), np.load(str(tmp_path / f"{case}.npz"))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert a[k].tobytes() == b[k].tobytes(), f"{case}: {k} does not regenerate"


def test_fixture_shape():
    assert pr.CASES == ("gail_ns", "gail_sa", "vail_ns", "vail_sa")
    data = gen.inputs()
    assert data["plcy_obs"].shape == (640, 34) and data["plcy_next"].shape == (640, 34) and data["plcy_act"].shape == (640, 13)
    assert data["demo_states"].shape == data["demo_next_states"].shape == (1000, 34) and data["demo_actions"].shape == (1000, 13)
    assert data["hold_obs"].shape == (4096, 34)
    for case in pr.CASES:
        g = np.load(pr.fixture(case))
        ds, d2 = gen.widths(case)
        assert (ds, d2) == ((32, 32) if case.endswith("_ns") else (32, 11))
        assert g["state_mask"].shape == (32,) and g["act_mask"].shape == (11,)
        assert g["perms"].shape == (2, 1280) and all(sorted(p) == list(range(1280)) for p in g["perms"])
        assert g["demo_idx"].shape == (2, 640) and all(len(set(d)) == 640 for d in g["demo_idx"])
        assert int(g["batch"]) == 512                       # 512, 512, 256 per epoch: the last one partial
        for k in (("loss", "bce", "ent") if pr.case_algo(case) == "gail" else ("loss", "bce", "kl", "beta")):
            assert g[k].shape == (6,), k
        for name, p0 in zip(gen.names(case), gen.init_params(case)):
            assert g[f"final_{name}"].shape == p0.shape and g[f"final_{name}"].dtype == np.float32
        assert gen.init_params(case)[0].shape[1] == ds + d2
        assert g["reward_logits"].shape == g["reward"].shape == (4096,) and g["reward"].dtype == np.float32
        assert ("targets" in g.files) == case.endswith("_sa") == bool(g["noisy"]) == (float(g["wd"]) == 1e-3)
        assert os.path.getsize(pr.fixture(case)) < 1 << 20
        # only data: no object arrays, nothing pickled
        assert all(g[k].dtype != object for k in g.files)


@pytest.mark.parametrize("case", pr.CASES)
def test_the_fit_moves_every_tensor_far_beyond_the_tolerance(case):
    g = np.load(pr.fixture(case))
    for p0, name in zip(gen.init_params(case), gen.names(case)):
        move = pr.rel(p0, g[f"final_{name}"])
        print(f"{case} {name}: moved {move:.3e}")
        assert move > 50 * TOL, (name, move)


@pytest.mark.parametrize("case", pr.CASES)
def test_float64_restatement_reproduces_the_reference_run(case):
    g = np.load(pr.fixture(case))
    o = pr.restate_case(case, g)
    assert o["step"] == 6
    for i, name in enumerate(gen.names(case)):
        r = pr.rel(o["params"][i].numpy(), g[f"final_{name}"])
        print(f"{case} {name}: rel {r:.3e}")
        assert r <= 1e-6, name
    for k in o["rec"]:
        np.testing.assert_allclose(o["rec"][k], g[k], rtol=2e-6, atol=2e-6, err_msg=k)
    d, r = o["logits"].numpy(), o["reward"].numpy()
    print(f"{case}: logits max err {np.abs(d - g['reward_logits']).max():.3e}, reward {np.abs(r - g['reward']).max():.3e}")
    np.testing.assert_allclose(d, g["reward_logits"], rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(r, g["reward"], rtol=2e-6, atol=2e-6)
    pr.check_statistics(o["colstats_fit"].numpy(), g, "fit_st")
    pr.check_statistics(o["colstats"].numpy(), g, "st")


@pytest.mark.parametrize("case", pr.CASES)
def test_the_count_rises_by_two_batches_per_forward_with_next_states(case):
    """gail_TRPO.py:206 adds the 1280 concatenated states per epoch; every minibatch forward adds its rows once (actions)
    or twice (next states); the reward evaluation adds its 4096 rows likewise."""
    g = np.load(pr.fixture(case))
    k = 2 if pr.case_standardise(case) else 1
    assert float(g["fit_st_count"][0]) == pytest.approx(1e-2 + 2 * (1280 + k * 1280), abs=1e-9)
    assert float(g["st_count"][0]) - float(g["fit_st_count"][0]) == pytest.approx(k * 4096, abs=1e-9)
    # one Standardizer of Ds columns in both modes
    assert g["st_sum"].shape == g["st_sumsq"].shape == (32,)


@pytest.mark.parametrize("case", NS_CASES)
@pytest.mark.parametrize("variant", ["shared", "count_b"])
def test_a_single_stage_reading_of_the_statistics_misses_the_fixture(case, variant):
    """The fixtures pin the two-stage rule: with both halves standardised by S2, or with the count rising by B only, the
    restatement misses the reference's logits and fitted parameters by a wide multiple of the device tolerance, while
    the two-stage restatement sits 20 times below it."""
    g = np.load(pr.fixture(case))
    right, wrong = pr.restate_case(case, g), pr.restate_case(case, g, variant=variant)
    ok = pr.rel(right["logits"].numpy(), g["reward_logits"])
    gap = pr.rel(wrong["logits"].numpy(), g["reward_logits"])
    pgap = max(pr.rel(wrong["params"][i].numpy(), g[f"final_{n}"]) for i, n in enumerate(gen.names(case)))
    print(f"{case} {variant}: logits off by {gap:.3e} ({gap / TOL:.0f} TOL; two-stage {ok:.3e}), parameters by {pgap:.3e}")
    assert ok <= TOL / 5
    assert gap >= 25 * TOL and pgap >= 25 * TOL


# ------------------------------------------------------------------------------ C ABI
def _header():
    return open(os.path.join(ROOT, "include", "olympic_hip.h")).read()


def test_header_declares_the_pair_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in PAIR_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _abi.SIGNATURES, name
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    # every new entry point cites the reference lines it replaces
    full = _header()
    for name in PAIR_ENTRIES:
        decl = full.index(f"{name}(")
        comment = full[full.rindex("/*", 0, decl):decl]
        assert "ws_floats" in name or re.search(r"(gail_TRPO|networks|vail_TRPO)\.py:\d+", comment), name


def test_pair_descriptor_layout_matches_the_header(tmp_path):
    cls = _abi.DiscPair
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             'printf("size %zu\\n", sizeof(oly_disc_pair));']
    lines += [f'printf("{f} %zu\\n", offsetof(oly_disc_pair, {f}));' for f, _ in cls._fields_]
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
    for pair_fn, fn in ((L.oly_gail_disc_fit_pair_ws_floats, L.oly_gail_disc_fit_ws_floats),
                        (L.oly_disc_fit_pair_ws_floats, L.oly_disc_fit_ws_floats)):
        assert int(pair_fn(2048, 32, 32, 1)) == int(fn(2048, 64)) > 0
        assert int(pair_fn(2048, 32, 11, 0)) == int(fn(2048, 43)) > 0
        assert int(pair_fn(1, 1, 63, 0)) > 0 and int(pair_fn(4096, 63, 1, 0)) > 0
        for bad in ((2048, 32, 33, 0),      # D > 64
                    (2048, 33, 33, 1),      # D > 64 with next states (Atlas / Talos masks doubled)
                    (2048, 32, 0, 0),       # D2 == 0
                    (2048, 32, 11, 1),      # next states of another width than the states
                    (2048, 0, 11, 0), (0, 32, 11, 0), (4097, 32, 32, 1)):
            assert int(pair_fn(*bad)) == -1, bad
    # a NULL context is refused before anything is read
    assert L.oly_gail_disc_fit_epoch_pair(None, None, None, None, 0, 1, None) == _abi.OLY_EINVAL
    assert L.oly_disc_fit_epoch_pair(None, None, None, None, 0, 1, None) == _abi.OLY_EINVAL
    assert L.oly_gail_disc_forward_pair(None, 0, 1, 1, *([None] * 9)) == _abi.OLY_EINVAL
    assert L.oly_gail_reward_step_pair(None, 0, 1, 1, None, None, None, None, None, 0, *([None] * 5)) == _abi.OLY_EINVAL
    assert L.oly_disc_forward_pair(None, 0, 1, 1, *([None] * 12)) == _abi.OLY_EINVAL
    assert L.oly_disc_reward_step_pair(None, 0, 1, 1, None, None, None, None, None, 0, *([None] * 8)) == _abi.OLY_EINVAL


def test_host_refusals_that_need_no_device():
    from olympic_hip._ffi import OlyError
    from olympic_hip.gail import (DiscriminatorReward, GAILDiscriminator, GAILDiscriminatorReward, VariationalDiscriminator,
                                  pair_masks)
    cpu = torch.device("cpu")
    m, m2, mx, mx2 = pair_masks("t", "next_state", 64, np.arange(2, 34), None, cpu)
    assert torch.equal(m, m2) and m.dtype == torch.int32 and (mx, mx2) == (33, 33)
    m, m2, mx, mx2 = pair_masks("t", "action", 43, np.arange(2, 34), [0, 1, 3, 4, 5, 6, 7, 8, 10, 11, 12], cpu)
    assert m.numel() == 32 and m2.numel() == 11 and mx2 == 12
    assert pair_masks("t", "action", 43, np.arange(32), None, cpu)[1] is None          # the actions as they are
    for bad in (dict(pair="next_state", dim=64, sm=np.arange(32), am=[0, 1]),          # the three-part combination
                dict(pair="next_state", dim=63, sm=None, am=None),                     # an odd width cannot be (s, s')
                dict(pair="next_state", dim=64, sm=np.arange(31), am=None),            # 2 Ds != the network's width
                dict(pair="action", dim=43, sm=np.arange(32), am=[]),                  # D2 == 0
                dict(pair="action", dim=32, sm=np.arange(32), am=None),                # D2 == 0
                dict(pair="action", dim=43, sm=np.arange(30), am=np.arange(11)),       # widths do not add up
                dict(pair="action", dim=43, sm=None, am=None),
                dict(pair="action", dim=43, sm=np.arange(32), am=[-1] + list(range(10))),
                dict(pair="states", dim=32, sm=None, am=None)):
        with pytest.raises(OlyError):
            pair_masks("t", bad["pair"], bad["dim"], bad["sm"], bad["am"], cpu)
    eng = types.SimpleNamespace(device=cpu)
    with pytest.raises(OlyError, match="not supported"):
        GAILDiscriminatorReward(eng, GAILDiscriminator(64), state_mask=np.arange(32), pair="next_state", act_mask=[0, 1])
    with pytest.raises(OlyError, match="not supported"):
        DiscriminatorReward(eng, VariationalDiscriminator(in_dim=64), state_mask=np.arange(32), pair="next_state",
                            act_mask=[0, 1])
    with pytest.raises(OlyError):        # D > 64: the network itself is refused
        GAILDiscriminatorReward(eng, GAILDiscriminator(66), state_mask=np.arange(33), pair="next_state")
    with pytest.raises(OlyError):        # an act_mask without the mode
        GAILDiscriminatorReward(eng, GAILDiscriminator(32), state_mask=np.arange(32), act_mask=[0, 1])
    r = GAILDiscriminatorReward(eng, GAILDiscriminator(43), state_mask=np.arange(2, 34), pair="action",
                                act_mask=np.arange(11))
    assert (r.ds, r.d2) == (32, 11) and tuple(r.stand.colstats.shape) == (3, 32)
    v = DiscriminatorReward(eng, VariationalDiscriminator(in_dim=64), state_mask=np.arange(2, 34), pair="next_state")
    assert (v.ds, v.d2) == (32, 32) and tuple(v.stand.colstats.shape) == (3, 32)
    x = torch.zeros((5, 36))
    for rr, x2_bad in ((r, torch.zeros((5, 10))), (v, torch.zeros((5, 33)))):
        with pytest.raises(OlyError):    # the second tensor is missing
            rr._check_pair(x, None)
        with pytest.raises(OlyError):    # a mask that reads past the source's columns
            rr._check_pair(x, x2_bad)
        with pytest.raises(OlyError):
            rr._check_pair(torch.zeros((5, 33)), torch.zeros((5, 36)))
        with pytest.raises(OlyError):    # rows differ
            rr._check_pair(x, torch.zeros((4, 36)))
