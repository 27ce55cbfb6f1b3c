"""The tables of tests/iq_big_shapes.py without a GPU: that they hold the shapes and configs they exist for; that every case
is one torch's own float32 run holds within a quarter of the GPU test's tolerance, taking the float64 run's side of every
clip, Huber kink and running-maximum branch on every row (the chosen seeds are re-asserted, not trusted); and that the cases
can tell a batch-machinery bug from rounding: the float64 restatement with ONE misread row, or the alpha update's sum over
the first 256 rows only, misses the GPU test's tolerance at least ten times over (the 10 is tests/il_shapes.py's rule)."""
import os

import numpy as np
import pytest
import torch

import iq_big_shapes as S
import iq_pi_restate as P

TOL = S.TOL
ISSUE_SHAPES = {(17, 6, 257, 1), (32, 11, 300, 150), (48, 16, 1040, 520), (48, 16, 4096, 2048), (1, 1, 4095, 4094)}


def check_tables():
    S.required_shapes_present()
    S.required_configs_present()
    assert set(S.K26_SHAPES) == ISSUE_SHAPES and set(S.K27_SHAPES) == {s[:3] for s in ISSUE_SHAPES}
    assert set(S.ALPHA_N) == {256, 257, 4095, 4096} and S.UPDATES == 2


def test_tables_hold_the_required_shapes_and_configs():
    check_tables()
    assert [S.tiles(s[2]) for s in S.K26_SHAPES] == [17, 19, 65, 256, 256]
    assert [S.last_tile(s[2]) for s in S.K26_SHAPES] == [1, 12, 16, 16, 15]
    assert S.steps_of(1040) == (195, 49) and S.stat_slices(257) == [17] * 15 + [2]
    assert len(S.Q_CASES) == len(set(S.Q_CASES)) and len(S.PI_CASES) == len(set(S.PI_CASES))
    for fam, seeds in S.SEEDS.items():
        assert len(seeds) == len(S.K26_SHAPES) and all(10 <= s < 10 + S.TRIED for s in seeds), fam
    assert S.TRIED >= 20


def test_a_table_without_one_of_its_shapes_is_noticed(monkeypatch):
    full = S.K26_SHAPES
    for i in range(len(full)):
        cut = full[:i] + full[i + 1:]
        monkeypatch.setattr(S, "K26_SHAPES", cut)
        monkeypatch.setattr(S, "K27_SHAPES", tuple(s[:3] for s in cut))
        with pytest.raises(AssertionError):
            S.required_shapes_present()
    monkeypatch.setattr(S, "K26_SHAPES", full)
    monkeypatch.setattr(S, "K27_SHAPES", tuple(s[:3] for s in full))
    for n in S.ALPHA_N:
        monkeypatch.setattr(S, "ALPHA_N", tuple(m for m in S.ALPHA_N if m != n))
        with pytest.raises(AssertionError):
            S.required_shapes_present()
        monkeypatch.undo()
    check_tables()


def test_a_config_table_without_one_of_its_entries_is_noticed(monkeypatch):
    full = S.Q_CONFIGS
    for i in range(len(full)):
        monkeypatch.setattr(S, "Q_CONFIGS", full[:i] + full[i + 1:])
        with pytest.raises(AssertionError):
            S.required_configs_present()
    monkeypatch.setattr(S, "Q_CONFIGS", full)
    monkeypatch.setattr(S, "PI_CONFIGS", S.PI_CONFIGS[1:])
    with pytest.raises(AssertionError):
        S.required_configs_present()
    monkeypatch.undo()
    check_tables()


# ------------------------------------------------------------------------------ every case: float32 can hold it
@pytest.mark.parametrize("case", S.Q_CASES, ids=S.q_case_id)
def test_k26_case_is_one_float32_can_hold(case):
    """The chosen seed's float32 run lies within TOL / 4 of float64 on the parameters and the target; q_yardstick has
    compared the two runs' sides row by row (the LSIQ families)."""
    ref, ref_out, f32, f32_out = S.q_yardstick(case)
    for key in ("params", "target"):
        spread = float(np.abs(S.cat(f32[key]) - S.cat(ref[key])).max())
        print(f"{S.q_case_id(case)} {key}: float32 {spread:.3e} from float64")
        assert spread <= TOL / 4, (S.q_case_id(case), key, spread)
    fam, cfg = S.Q_CONFIGS[case[1]]
    used = 9 if fam == "h" else 13
    assert np.isfinite(ref_out[:, :used]).all() and np.isfinite(ref_out[:, 7 if fam == "h" else 15]).all()
    # the second update starts from moments and, with Standardizers, from statistics the first one left
    assert all(float(np.abs(m).max()) > 0 for m in ref["exp_avg"])
    if cfg.standardizer:
        assert float(ref["colstats"][0, 0]) > S.K26_SHAPES[case[0]][2]


@pytest.mark.parametrize("case", S.PI_CASES, ids=S.pi_case_id)
def test_k27_case_is_one_float32_can_hold(case):
    ref, ref_out, _, f32, _, _ = S.pi_yardstick(case)
    spread = float(np.abs(S.cat(f32["policy"]["params"]) - S.cat(ref["policy"]["params"])).max())
    print(f"{S.pi_case_id(case)} policy: float32 {spread:.3e} from float64")
    assert spread <= TOL / 4, (S.pi_case_id(case), spread)
    assert np.isfinite(ref_out).all()


@pytest.mark.parametrize("n", S.ALPHA_N)
def test_alpha_case_is_one_float32_can_hold(n):
    lps, te, lr, init = S.alpha_case(n)
    want = P.alpha_adam(lps, te, lr, init=init)
    assert S.worst(S.alpha_errors(P.alpha_adam(lps, te, lr, init=init, dtype=torch.float32), want)) <= 0.25


# ------------------------------------------------------------------------------ one misread row misses the tolerance
def _q_sensitivity(case, dst, src, what):
    k, j = case
    fam, cfg = S.Q_CONFIGS[j]
    steps, params = S.q_case_inputs(fam, k)
    state, out, _ = S.q_run(fam, cfg, params, S.misread_row(steps, dst, src), S.K26_SHAPES[k][3])
    errs = S.q_errors(S.q_state_of(state), out, S.q_yardstick(case))
    print(f"{S.q_case_id(case)} {what}: " + ", ".join(f"{n} {e / t:.0f}x" for n, e, t in errs))
    assert S.worst(errs) >= 10, (S.q_case_id(case), what, errs)


def _iq_and_sqil_cases(k):
    cases = [(kk, j) for kk, j in S.Q_CASES if kk == k and S.Q_CONFIGS[j][0] == "iq"]
    assert {S.Q_CONFIGS[j][1].algo for _, j in cases} == {"iq", "sqil"}
    return cases


@pytest.mark.parametrize("k", range(len(S.K26_SHAPES)), ids=["-".join(map(str, s)) for s in S.K26_SHAPES])
def test_k26_cases_notice_one_misread_row(k):
    """The last row read as row 0, and the last policy row read as the first expert row, in every field: the float64 run
    on such inputs is at least 10 tolerances away on some compared tensor or scalar, for every IQ and SQIL case of the
    shape."""
    _, _, B, n_policy = S.K26_SHAPES[k]
    for case in _iq_and_sqil_cases(k):
        _q_sensitivity(case, B - 1, 0, "last row misread")
        _q_sensitivity(case, n_policy - 1, n_policy, "boundary row misread")


@pytest.mark.parametrize("k", range(len(S.K27_SHAPES)), ids=["-".join(map(str, s)) for s in S.K27_SHAPES])
def test_k27_cases_notice_one_misread_row(k):
    Bp = S.K27_SHAPES[k][2]
    cases = [c for c in S.PI_CASES if c[0] == k]
    assert cases
    for case in cases:
        cfg, two = S.PI_CONFIGS[case[1]]
        inp = S.pi_case_inputs(k)
        state, out, acts = S.pi_run(cfg, two, dict(inp, steps=S.misread_row(inp["steps"], Bp - 1, 0)))
        errs = S.pi_errors(S.pi_state_of(state), out, acts[-1], S.pi_yardstick(case))
        print(f"{S.pi_case_id(case)} last row misread: " + ", ".join(f"{n} {e / t:.0f}x" for n, e, t in errs))
        assert S.worst(errs) >= 10, (S.pi_case_id(case), errs)


@pytest.mark.parametrize("n", [n for n in S.ALPHA_N if n > S.THREADS])
def test_alpha_cases_notice_a_sum_over_the_first_trip_only(n):
    lps, te, lr, init = S.alpha_case(n)
    errs = S.alpha_errors(P.alpha_adam(S.first_trip_only(lps, te), te, lr, init=init), P.alpha_adam(lps, te, lr, init=init))
    print(f"n={n} first 256 rows only: " + ", ".join(f"{k} {e / t:.0f}x" for k, e, t in errs))
    assert S.worst(errs) >= 10, (n, errs)


def test_alpha_at_one_trip_is_unchanged_by_that_reading():
    lps, te, lr, init = S.alpha_case(S.THREADS)
    assert np.array_equal(P.alpha_adam(S.first_trip_only(lps, te), te, lr, init=init), P.alpha_adam(lps, te, lr, init=init))


# ------------------------------------------------------------------------------ the workspaces
def test_workspace_sizes_for_every_shape():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    for in_dim, A, B, _ in S.K26_SHAPES:
        nq, npi = int(L.oly_iq_q_ws(B, in_dim, A)), int(L.oly_iq_pi_ws(B, in_dim, A))
        BP = S.tiles(B) * S.TILE
        # per row and gradient pass 64 + 512 + 256 activations and 512 + 256 + 1 deltas, three passes in K26
        assert nq >= 3 * BP * 1601 + 256 * 512 and npi > 0, (B, nq, npi)
        off = int(L.oly_iq_q_ws_values(B, in_dim, A))
        assert 0 < off and off + 3 * BP <= nq
        off = int(L.oly_iq_pi_ws_values(B, in_dim, A))
        assert 0 <= off and off + B <= npi
    assert int(L.oly_iq_q_ws(4096, 48, 16)) >= 19_000_000
