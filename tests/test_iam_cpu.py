"""The inverse action model's kernel layer without a GPU: the argument blocks that grew (oly_bc_fit, oly_bc_fit_log,
oly_sg_act_args) and the new oly_bc_pair against a compiled C snippet, the header's contract, the case table of
tests/iam_restate.py held to the issue's, the float64 twins, and the refusals that need no engine."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import bc_restate as br
import iam_restate as ir
from olympic_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = (("oly_bc_pair", _abi.BCPair), ("oly_bc_fit", _abi.BCFit), ("oly_bc_fit_log", _abi.BCFitLog),
           ("oly_sg_act_args", _abi.SGAct))


@pytest.mark.parametrize("name,cls", STRUCTS, ids=[s[0] for s in STRUCTS])
def test_struct_layouts_match_the_header(tmp_path, name, cls):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/olympic_hip.h"', "int main(){",
             f'printf("size %zu\\n", sizeof({name}));']
    lines += [f'printf("{f} %zu\\n", offsetof({name}, {f}));' for f, *_ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    assert len(out) == len(cls._fields_) + 1
    for f, *_ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def test_the_blocks_grew_at_their_ends_and_the_abi_version_stayed():
    assert _abi.BCFit._fields_[-1][0] == "pair" and _abi.BCFit._fields_[-2][0] == "out"
    names = [f[0] for f in _abi.SGAct._fields_]
    assert names[names.index("pad") + 1:] == ["x2", "d2", "stride1", "stride2", "n_rows", "idx", "clip_lo", "clip_hi"]
    raw = open(os.path.join(ROOT, "include", "olympic_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert int(re.search(r"#define OLY_ABI_VERSION (\d+)", txt).group(1)) == _abi.ABI_VERSION == 8
    # the paired paths go through the entry points K24 and K25 have: the header gained a struct and no function
    assert re.search(r"typedef struct oly_bc_pair\s*\{", txt) and "const oly_bc_pair* pair;" in txt
    assert not re.search(r"\boly_(iam|bc_pair|bc_fit_pair|sg_act_pair)\w*\s*\(", txt)
    assert "action_models.py:257-528" in raw and "lsiqfo.py:90" in raw
    # an all-zero tail is the call as it was
    f = _abi.SGAct(n=1, in_dim=2, act_dim=1)
    assert not f.x2 and not f.idx and not f.clip_lo and not f.clip_hi and (f.d2, f.stride1, f.stride2, f.n_rows) == (0, 0, 0, 0)
    assert not _abi.BCFit().pair


def test_the_table_is_the_issues():
    assert {(c.d1, c.d2) for c in ir.CASES} == {(1, 1), (5, 12), (16, 17), (32, 32), (3, 61)}
    assert {c.A for c in ir.CASES} == {1, 8, 9, 16} and {c.batch for c in ir.CASES} == {1, 15, 16, 17, 33}
    wide = [bool(c.pad1 or c.pad2) for c in ir.CASES]
    assert sum(wide) * 2 == len(wide), "strides wider than the widths in half the cases"
    assert ir.RING == 40 and ir.STEPS == 3 and all(c.d1 + c.d2 <= 64 for c in ir.CASES)
    for c in ir.CASES:
        k = ir.build(c)
        idx = k["idx"]
        assert idx.shape == (3, c.batch) and 0 in idx and ir.RING - 1 in idx
        if c.batch > 1:
            assert all(len(set(row.tolist())) < c.batch for row in idx), "duplicates inside a batch"
        u = (k["actions"] - k["central"]) / k["delta"]
        assert (np.abs(u) >= 1).any() and (np.abs(u) < 1).any()
        assert abs(float(np.abs(k["targets"]).max()) - 8.3177662) <= 1e-5, "the clip at f32(1 - 1e-7) is reached"
        assert k["states"].shape == (ir.RING, c.d1 + c.pad1) and np.isnan(k["states"][:, c.d1:]).all()
        assert np.array_equal(k["table"], np.concatenate([k["states"][:, :c.d1], k["next_states"][:, :c.d2]], axis=1))


@pytest.mark.parametrize("c", ir.CASES, ids=[ir.case_id(c) for c in ir.CASES])
def test_float32_twin_lies_within_the_tolerance_of_float64(c):
    k = ir.build(c)
    _, r64 = ir.fit_twin(c, k, steps=2)
    _, r32 = ir.fit_twin(c, k, steps=2, dtype=torch.float32)
    err = max(float(np.abs(a - b).max()) for a, b in zip(r64["params"][-1], r32["params"][-1]))
    print(f"{ir.case_id(c)}: |f32 - f64| max {err:.3e}")
    assert err <= ir.TOL
    assert all(float(np.abs(a - b).max()) > 0 for a, b in zip(r64["params"][-1], k["params"])), "the fit moves every tensor"


def test_draw_twin_clips_in_float64_and_feeds_the_standardizer():
    c = ir.CASES[1]
    k = ir.build(c)
    rows = k["idx"].reshape(-1)[:9]
    D = c.d1 + c.d2
    plain = ir.draw_twin(c, k, rows, colstats=np.zeros((3, D)))
    lo, hi = k["central"] - 0.3 * k["delta"].astype(np.float64), k["central"] + 0.3 * k["delta"].astype(np.float64)
    clipped = ir.draw_twin(c, k, rows, colstats=np.zeros((3, D)), clip=(lo, hi))
    assert (clipped["action"] >= lo).all() and (clipped["action"] <= hi).all() and (clipped["action"] != plain["action"]).any()
    assert plain["colstats"][0, 0] == 9
    # the wrong reading that leaves the rows out of the statistics misses by far more than the tolerance
    seen = ir.draw_twin(c, k, rows, colstats=plain["colstats"])
    unseen = ir.draw_twin(c, k, rows, colstats=None)
    assert float(np.abs(seen["mu"] - unseen["mu"]).max()) > 100 * ir.TOL
    mean = ir.draw_twin(c, k, rows, colstats=np.zeros((3, D)), eps=False)
    assert np.allclose(mean["action"], np.tanh(mean["mu"]) * k["delta"] + k["central"], atol=1e-7)


def test_engine_refuses_a_bad_pair_before_any_call():
    from olympic_hip._ffi import OlyError
    from olympic_hip.engine import Engine
    fake = types.SimpleNamespace(device=torch.device("cpu"))
    rows = lambda *a, **kw: Engine._bc_rows(fake, "bc_fit_steps", *a, **kw)
    s, ns, act = torch.zeros((9, 7)), torch.zeros((9, 5)), torch.zeros((9, 3))
    cen, dl = torch.zeros(3), torch.ones(3)
    good = dict(x2=ns, actions=act, central=cen, delta=dl)
    in_dim, A, bp = rows(s, None, good)
    assert (in_dim, A, bp.d1, bp.d2, bp.stride1, bp.stride2) == (12, 3, 7, 5, 7, 5) and bp.x2 == ns.data_ptr()
    in_dim, A, bp = rows(s, None, dict(good, d1=2, d2=4))
    assert (in_dim, bp.d1, bp.d2, bp.stride1, bp.stride2) == (6, 2, 4, 7, 5)
    assert rows(s, torch.zeros((9, 3)), None) == (7, 3, None)
    for bad, why in ((dict(good, d1=8), "widths"), (dict(good, d2=6), "widths"), (dict(good, d1=-1), "widths"),
                     (dict(good, x3=ns), "unknown"), (dict(good, x2=None), "x2"), (dict(good, actions=torch.zeros(9)), "actions"),
                     (dict(good, central=None), "central"), (dict(good, delta=torch.ones(4)), "delta"),
                     (dict(good, x2=torch.zeros((8, 5))), "x2"), (dict(good, x2=ns.double()), "x2")):
        with pytest.raises(OlyError, match=why):
            rows(s, None, bad)
    with pytest.raises(OlyError, match="targets must be None"):
        rows(s, torch.zeros((9, 3)), good)
    with pytest.raises(OlyError, match="targets"):
        rows(s, None, None)


def test_model_refuses_shapes_before_it_needs_an_engine():
    from olympic_hip._ffi import OlyError
    from olympic_hip.iqfo import DeviceGaussianInvActionModel
    lin = torch.nn.Linear
    lo, hi = -np.ones(4), np.ones(4)
    with pytest.raises(OlyError, match="in <= 64"):           # 2 * in_dim > 64: a row (s | s') of 66 columns
        DeviceGaussianInvActionModel(None, [lin(66, 512), lin(512, 256), lin(256, 8)], lo, hi, 1e-3)
    with pytest.raises(OlyError, match="three Linear"):
        DeviceGaussianInvActionModel(None, [lin(12, 512), lin(512, 8)], lo, hi, 1e-3)
    with pytest.raises(OlyError, match="2A"):
        DeviceGaussianInvActionModel(None, [lin(12, 512), lin(512, 256), lin(256, 7)], lo, hi, 1e-3)
    with pytest.raises(OlyError, match="min_a / max_a"):
        DeviceGaussianInvActionModel(None, [lin(12, 512), lin(512, 256), lin(256, 8)], lo[:3], hi[:3], 1e-3)


def test_agents_refuse_before_they_need_an_engine():
    """The refusals of the from-observations agents' constructors, each with a message that names what it refuses."""
    from olympic_hip import iqfo
    from olympic_hip._ffi import OlyError
    pol = types.SimpleNamespace(in_dim=6, act_dim=5)
    demo = dict(states=np.zeros((4, 6)), next_states=np.zeros((4, 6)), absorbing=np.zeros(4))
    for cls in (iqfo.DeviceIQfOSAC, iqfo.DeviceLSIQfOSAC, iqfo.DeviceLSIQfOHSAC, iqfo.DeviceLSIQfOHCSAC):
        for kw, why in ((dict(add_noise_to_obs=True), "add_noise_to_obs"),
                        (dict(ext_normalizer_action_model=object()), "ext_normalizer_action_model"),
                        (dict(action_model="KLGaussianInvActionModel"), "KL-Gaussian"), (dict(action_model="GCPActionModel"), "GCP"),
                        (dict(action_model="KLGCPActionModel"), "KL-GCP"),
                        (dict(action_model="LearnableVarGaussianInvActionModel"), "learnable-variance"),
                        (dict(action_model="FixedVarGaussianInvActionModel"), "fixed-variance"),
                        (dict(interpolate_expert_states=True, state_mask=[0, 1, 2, 3, 4, 5]), "state_mask"),
                        (dict(), "DeviceGaussianInvActionModel")):
            with pytest.raises(OlyError, match=why):
                cls(None, pol, None, demo, 0.99, 9, True, **kw)
        with pytest.raises(OlyError, match="2 \\* in_dim = 66 > 64"):
            cls(None, types.SimpleNamespace(in_dim=33, act_dim=5), None, demo, 0.99, 9, True)
    assert iqfo.DeviceLSIQfOSAC.CLIP_DRAW and not any(c.CLIP_DRAW for c in (iqfo.DeviceIQfOSAC, iqfo.DeviceLSIQfOHSAC,
                                                                          iqfo.DeviceLSIQfOHCSAC))
    assert "init_epochs" in iqfo.__doc__ and "unreachable" in iqfo.__doc__ and "IQfO_ORIG" in iqfo.__doc__


# ------------------------------------------------------------------------------ the reference-run fixtures
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("iqfo", "lsiqfo")
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def fixture_params(g):
    """The six initial tensors: layer 2's weights are the generator's seeded draws, the rest is stored."""
    import sys
    sys.path.insert(0, GOLDEN)
    import gen_iam_fit as gen
    import gen_iq_q_update as gq
    return [gq.w2_init(gen.W2_SEED) if n == "w2" else g[f"init_{n}"] for n in NAMES]


def tolerance(g, group):
    return max(2e-5, 4 * float(g[f"spread_{group}"]))         # the project's rule


def fixture_miss(g, twin):
    """The largest distance of a twin from the reference run, per group: the stored parameters (layer 2's weights by
    their first 16 rows after the last iteration), the scalars, the drawn actions."""
    p = 0.0
    for it in range(ir.SEQ_ITERS):
        for i, n in enumerate(NAMES):
            if n != "w2":
                p = max(p, float(np.abs(twin["params"][it][i] - g[f"{n}_it{it}"]).max()))
    p = max(p, float(np.abs(twin["params"][-1][2][:16] - g["w2_rows_final"]).max()))
    scal = np.asarray(twin["scalars"])[:, -8:]           # the eight logged scalars (the twin's row holds the fit losses first)
    return dict(params=p, scalars=float(np.abs(scal - g["scalars"]).max()),
                drawn=float(np.abs(twin["drawn"] - g["drawn"]).max()))


def agent_params(g, group):
    """The six initial tensors of the fixture's policy or critic (layer 2's weights from the generator's seeds)."""
    import sys
    sys.path.insert(0, GOLDEN)
    import gen_iam_fit as gen
    import gen_iq_q_update as gq
    seed = gen.W2_SEED + (1 if group == "policy" else 2)
    return [gq.w2_init(seed) if n == "w2" else g[f"{group}_init_{n}"] for n in NAMES]


def agent_miss(g, nets, actor_rows=None):
    """nets: dict(policy, critic, target: six float64 arrays each) after the four iterations; the largest distance from
    the reference run per network (layer 2's weights by their first 16 rows) and of the Actor/... scalars."""
    out = {}
    for group, params in nets.items():
        out[group] = max(float(np.abs(np.asarray(a)[:16] - g[f"{group}_w2_head"]).max()) if n == "w2"
                         else float(np.abs(np.asarray(a) - g[f"{group}_{n}"]).max()) for n, a in zip(NAMES, params))
    if actor_rows is not None:
        import sys
        sys.path.insert(0, GOLDEN)
        import gen_iam_fit as gen
        got = np.array([[actor_rows[i + 1][t] for t in gen.ACTOR_TAGS] for i in range(ir.SEQ_ITERS)])
        out["actor_scalars"] = float(np.abs(got - g["actor_scalars"]).max())
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_whole_fit_twin_against_the_reference_run_and_both_wrong_readings(golden, name):
    """tests/golden/iam_fit holds the reference's own IQfO_SAC.fit / LSIQfO.fit, executed for four logging iterations:
    the float64 twin of the whole fit follows it on the policy, the critic and its target; the two wrong readings of
    the action model's Standardizer reach the critic and the policy through the drawn actions and miss."""
    g = golden(f"iam_fit/{name}.npz")
    args = (g, name, fixture_params(g), agent_params(g, "policy"), agent_params(g, "critic"))
    t = ir.fo_fit_twin(*args)
    nets = lambda t: dict(policy=t["policy"]["params"], critic=t["critic"]["params"], target=t["critic"]["target"])
    miss = agent_miss(g, nets(t), t["actor_scalars"])
    print(name, miss)
    for group, v in miss.items():
        assert v <= tolerance(g, group), (group, v)
    for key, got in (("policy", t["policy"]["colstats"]), ("critic", t["critic"]["colstats"]), ("target", t["critic"]["tcolstats"])):
        want = g[f"{key}_colstats"]
        assert np.abs(got[0] - want[0]).max() <= 1e-9, key
        assert np.all(np.abs(got - want) <= 2e-5 * np.maximum(1, np.abs(want))), key
    assert np.abs(t["am_scalars"][:, 2:] - g["scalars"]).max() <= tolerance(g, "scalars")
    for wrong in ("draw", "logging"):
        w = agent_miss(g, nets(ir.fo_fit_twin(*args, wrong=wrong)))
        assert w["critic"] > 10 * tolerance(g, "critic") and w["policy"] > 10 * tolerance(g, "policy"), (wrong, w)
        for group in ("critic", "policy"):
            stored = float(g[f"miss_{wrong}_{group}"])
            # stored: over the whole network; measured here: over what the fixture keeps of it (16 rows of layer 2)
            assert stored > 10 * tolerance(g, group) and w[group] <= stored * (1 + 1e-6), (wrong, group, w[group], stored)


@pytest.mark.parametrize("name", FIXTURES)
def test_twin_against_the_reference_run_and_both_wrong_readings(golden, name):
    g = golden(f"iam_fit/{name}.npz")
    p0 = fixture_params(g)
    clip = name == "lsiqfo"
    twin = ir.sequence_twin(g, p0, clip=clip)
    miss = fixture_miss(g, twin)
    print(name, miss)
    for group, v in miss.items():
        assert v <= tolerance(g, group), (group, v)
    # the statistics: the reference sums the float32 rows in float32 (networks.py:77-78); the count is exact
    cs = twin["colstats"]
    assert np.abs(cs[:, 0] - g["colstats"][:, 0]).max() <= 1e-9        # stored as the reference's _count - 1e-2
    assert cs[-1, 0, 0] == ir.SEQ_ITERS * (ir.SEQ_FITS * ir.SEQ_AMB + 6 * ir.SEQ_AMB + ir.SEQ_B)
    assert np.all(np.abs(cs - g["colstats"]) <= 2e-5 * np.maximum(1, np.abs(g["colstats"])))
    u = (g["ring_a"] - g["central"]) / g["delta"]
    assert (np.abs(u) >= 1).any(), "the clip at f32(1 - 1e-7) is exercised"
    for wrong in ("draw", "logging"):
        m = fixture_miss(g, ir.sequence_twin(g, p0, wrong=wrong, clip=clip))
        worst = max(m["params"], m["scalars"])
        assert worst > 10 * max(tolerance(g, "params"), tolerance(g, "scalars")), (wrong, m)
        assert abs(worst - float(g[f"miss_{wrong}"])) <= 1e-6 * max(1.0, worst), (wrong, worst, float(g[f"miss_{wrong}"]))
    assert os.path.getsize(os.path.join(GOLDEN, "iam_fit", f"{name}.npz")) < 1 << 20


def _reference_dir():
    import sys
    sys.path.insert(0, GOLDEN)
    import _ref_stubs
    return _ref_stubs.REF


@pytest.mark.skipif(not os.path.isdir(_reference_dir()), reason="the reference tree is only in the build container")
def test_fixtures_regenerate_byte_for_byte(tmp_path):
    import sys
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "gen_iam_fit.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONHASHSEED="random"))
    assert r.returncode == 0, r.stderr[-2000:]
    for name in FIXTURES:
        a = open(os.path.join(GOLDEN, "iam_fit", f"{name}.npz"), "rb").read()
        assert a == open(str(tmp_path / f"{name}.npz"), "rb").read(), f"{name} does not regenerate"
