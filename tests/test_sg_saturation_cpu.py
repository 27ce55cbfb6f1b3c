"""The saturated tables of tests/sg_saturation.py without a GPU: they hold what they are for (bands of |u| up to exact
fp64 tanh = -+1, a column clamped at log_std_max, a large unclamped sigma), the kernels' arithmetic (float32 with the fp64
epilogue) can be held to TOL / 4 on them on 1, 4, 8 and 16 threads, torch's all-float32 run cannot be held to TOL on any of
them (they lie where the older sweeps had to stay out), and the two wrong readings of the tanh correction pass
iq_pi_restate's sweep and miss these tables by more than 10 TOL."""
import numpy as np
import pytest
import torch

import iq_pi_restate as P
import sg_saturation as S

TOL = S.TOL
TABLE = S.table()
IDS = [S.run_id(*t) for t in TABLE]


@pytest.fixture
def threads():
    keep = torch.get_num_threads()
    yield torch.set_num_threads
    torch.set_num_threads(keep)


def test_the_tables_hold_what_they_are_for():
    seen = S.required_present()
    assert len(seen) == len(TABLE) + len(S.SG_CASES) + 2          # the paired path's case on either row selection
    for who, facts in seen.items():
        for i, f in enumerate(facts):
            print(f"{who} update {i}: bands {[sum(b) for b in f['bands']]} (-, +: {f['bands']}), clamped high {f['high']}, "
                  f"low {f['low']}, unclamped {f['unclamped']}, large-sigma saturated {f['big_sigma_saturated']}")
    # the clamp is the agents', the table leaves out only A = 1, and the two-critic step runs on shapes 1 and 4
    assert S.SAT_LS == (-20.0, 2.0) and S.SAT_SHAPES == (1, 2, 3, 4) and S.TWO_CRITICS == (1, 4)
    assert [S.SG_CASES[i][:3] for i in range(2)] == [(45, 19, 7), (33, 32, 11)]
    # the hand-placed noise is in every update's, in K25's and in the older sweep's nowhere
    for k in S.SAT_SHAPES:
        assert all(tuple(s["eps"][:4, 0]) == S.PLACED for s in S.sat_inputs(k)["steps"])
        assert S.sat_inputs(k)["pparams"][5][P.SHAPES[k][1]:][:3].tolist() == [3.0, 1.5, -6.0]
        assert float(np.abs(P.sweep_inputs(k)["pparams"][5][P.SHAPES[k][1]:]).max()) == 6.0
    assert all(tuple(S.sg_sat_case(i)["eps"][:4, 0]) == S.PLACED for i in range(2))
    assert all(float(np.abs(S.sg_sat_case(i)["eps"]).max()) > 2.0 for i in range(2)), "the noise is not clipped"


def test_the_recording_act_is_the_policys(threads):
    """sat_yardstick runs Policy.act restated (it records the sample): the same bits as iq_pi_restate.run's own (on one
    thread: with more, torch's sums differ by an ulp between two graphs of the same expressions)."""
    k, j = 1, 0
    threads(1)
    ref = P.run(S.sat_inputs(k), S.SAT_CONFIGS[j], act=S.recording_act([]))
    plain = P.run(S.sat_inputs(k), S.SAT_CONFIGS[j])
    assert np.array_equal(ref[1], plain[1])
    assert all(np.array_equal(a, b) for a, b in zip(ref[0]["policy"]["params"], plain[0]["policy"]["params"]))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(ref[2], plain[2]))


@pytest.mark.parametrize("k,j,two", TABLE, ids=IDS)
def test_the_kernel_model_lies_within_a_quarter_of_tol(threads, k, j, two):
    """The conditioning check of a saturated case: the twin in float32 with K25's / K27's fp64 epilogue against float64,
    every tensor of the rule, with torch's sums on 1, 4, 8 and 16 threads."""
    case, cfg, ref = S.sat_inputs(k), S.SAT_CONFIGS[j], S.sat_yardstick(k, j, two)
    assert np.isfinite(ref[1]).all()
    for n in S.THREADS:
        threads(n)
        d = S.distances(S.run_model(case, cfg, two), ref)
        print(f"{S.run_id(k, j, two)} {n} threads: model / TOL " + ", ".join(f"{key} {v:.4f}" for key, v in d.items()))
        assert S.worst(d) <= 0.25, (n, d)
    # every weight tensor moves by 10 TOL over the three updates: the comparison sees the update
    for name, p0, p1 in zip(P.NAMES, case["pparams"], ref[0]["policy"]["params"]):
        assert float(np.abs(p1 - p0.astype(np.float64)).max()) >= 10 * TOL, name


@pytest.mark.parametrize("k,j,two", TABLE, ids=IDS)
def test_torchs_float32_run_cannot_be_held_to_tol_here(k, j, two):
    """The regime the older sweeps had to avoid: evaluated in float32, 1 - a^2 + 1e-6 is ill conditioned, and torch's own
    all-float32 run misses TOL on some tensor of every case."""
    d = S.distances(S.run_with(S.sat_inputs(k), S.SAT_CONFIGS[j], torch.float32, two=two), S.sat_yardstick(k, j, two))
    print(f"{S.run_id(k, j, two)}: float32 / TOL " + ", ".join(f"{key} {v:.2f}" for key, v in d.items()))
    assert S.worst(d) > 1.0, d


@pytest.mark.parametrize("kind", S.READINGS)
@pytest.mark.parametrize("k,j,two", TABLE, ids=IDS)
def test_a_wrong_reading_misses_a_saturated_case_by_ten_tol(k, j, two, kind):
    d = S.distances(S.run_reading(S.sat_inputs(k), S.SAT_CONFIGS[j], kind, two), S.sat_yardstick(k, j, two))
    print(f"{S.run_id(k, j, two)} {kind}: / TOL " + ", ".join(f"{key} {v:.3g}" for key, v in d.items()))
    assert S.worst(d) >= 10.0, d


@pytest.mark.parametrize("kind", S.READINGS)
def test_a_wrong_reading_passes_the_older_sweep(kind):
    """The hole, stated: with the clamp [-3, -0.5] and no saturated entry a policy update whose tanh correction has the
    stable identity's gradient, or no guard at all, lies within TOL of the float64 yardstick on every case of
    iq_pi_restate's sweep."""
    seen = 0.0
    for k in range(len(P.SHAPES)):
        for j, cfg in enumerate(P.CONFIGS):
            d = S.distances(P.run(P.sweep_inputs(k), cfg, act=S.reading_act(kind)), P.yardstick(k, j))
            seen = max(seen, S.worst(d))
            assert S.worst(d) <= 1.0, (P.SHAPES[k], P.cfg_id(cfg), d)
    print(f"{kind}: worst distance on the older sweep {seen:.4f} TOL")


@pytest.mark.parametrize("k,j,two", TABLE, ids=IDS)
def test_the_float64_action_is_a_bound_where_tanh_is_one(k, j, two):
    case, (_, _, acts, log) = S.sat_inputs(k), S.sat_yardstick(k, j, two)
    central, delta = case["central"].astype(np.float64), case["delta"].astype(np.float64)
    for (a, _), e in zip(acts, log):
        last = np.abs(e["u"]) >= S.EDGES[2]
        assert last[:4, 0].all() and last.sum() >= 4
        want = central[None, :] + np.sign(e["u"]) * delta[None, :]
        assert np.array_equal(a[last], want[last])
        assert not np.array_equal(a[~last], want[~last])


@pytest.mark.parametrize("i", range(len(S.SG_CASES)), ids=[S.sg_id(i) for i in range(len(S.SG_CASES))])
def test_k25s_cases_can_be_held_to_a_quarter_of_tol(threads, i):
    k, A = S.sg_sat_case(i), S.SG_CASES[i][2]
    ref = S.sg_host(k, A)
    assert np.isfinite(ref["log_prob"]).all()
    for n in S.THREADS:
        threads(n)
        d = S.sg_distances(S.sg_host(k, A, torch.float32), ref)
        print(f"{S.sg_id(i)} {n} threads: model / TOL action {d['action']:.4f}, log_prob {d['log_prob']:.4f}")
        assert max(d.values()) <= 0.25, d
    last = np.abs(ref["u"]) >= S.EDGES[2]
    want = k["central"].astype(np.float64)[None, :] + np.sign(ref["u"]) * k["delta"].astype(np.float64)[None, :]
    assert last.sum() >= 4 and np.array_equal(ref["action"][last], want[last])
