"""The tables of tests/bc_big_shapes.py without a GPU: that they hold the shapes they exist for; that every case is one
torch's own float32 run holds within a quarter of the GPU test's tolerance on every parameter tensor (the chosen seeds are
re-asserted, not trusted); and that the cases can tell a batch-machinery bug from rounding: the float64 restatement with one
misread index position, with the scalars of the first 256 rows only, or with statistics of one row per chain, misses the GPU
test's tolerance at least ten times over (the 10 is tests/il_shapes.py's rule)."""
import os

import numpy as np
import pytest

import bc_big_shapes as S
import bc_restate as br

TOL = S.TOL
ISSUE_BC = {(17, 6, 257, 300, True, False), (33, 11, 300, 1000, True, True), (45, 12, 1040, 1100, True, True),
            (64, 16, 4096, 5000, True, True), (64, 16, 4096, 4096, False, False), (1, 1, 4095, 4100, True, False)}
ISSUE_IAM = {(5, 12, 6, 257, 3, 1, True): 300, (16, 17, 11, 300, 0, 0, True): 40, (3, 61, 9, 1040, 0, 0, True): 1100,
             (32, 32, 16, 4096, 4, 9, True): 5000, (5, 12, 16, 4096, 2, 5, False): 4096, (1, 1, 1, 4095, 0, 0, True): 4100}

# (kind, index, logged) of every run the GPU test compares with float64; the saturated logged case also as its twin
RUNS = [("bc", i, False) for i in range(len(S.BC_SHAPES))] + [("iam", i, False) for i in range(len(S.IAM_SHAPES))] + \
       [("bc", i, True) for i in S.BC_LOGGED] + [("twin", i, True) for i in S.BC_LOGGED if S.BC_SHAPES[i][5]] + \
       [("iam", i, True) for i in S.IAM_LOGGED]


def run_of(kind, i):
    return S.paired(i) if kind == "iam" else S.unpaired(i, twin=kind == "twin")


def run_id(r):
    kind, i, logged = r
    return f"{kind}-{run_of(kind, i)['who']}" + ("-logged" if logged else "")


def check_tables():
    S.required_shapes_present()
    S.required_logged_present()
    assert set(S.BC_SHAPES) == ISSUE_BC and dict(zip(S.IAM_SHAPES, S.RINGS)) == ISSUE_IAM and S.UPDATES == 2
    assert {S.BC_SHAPES[i][:3] for i in S.BC_LOGGED} == {(17, 6, 257), (64, 16, 4096), (1, 1, 4095)}
    assert {(S.IAM_SHAPES[i][3], S.RINGS[i]) for i in S.IAM_LOGGED} == {(257, 300), (300, 40), (4096, 5000)}


def test_tables_hold_the_required_shapes():
    check_tables()
    batches = [s[2] for s in S.BC_SHAPES]
    assert batches == [s[3] for s in S.IAM_SHAPES]
    assert [S.tiles(b) for b in batches] == [17, 19, 65, 256, 256, 256]
    assert [S.last_tile(b) for b in batches] == [1, 12, 16, 16, 16, 15]
    assert S.wave_shares(257) == [5, 5, 5, 2] and S.wave_shares(1040) == [17, 17, 17, 14] and S.wave_shares(4096) == [64] * 4
    assert S.wave_shares(256) == [4] * 4 and S.wave_shares(33) == [1, 1, 1, 0], "what the small tables reach"
    assert S.stat_slices(257) == [17] * 15 + [2] and S.stat_slices(33) == [3] * 11 + [0] * 5
    for seeds in (S.BC_SEEDS, S.IAM_SEEDS, (S.TWIN_SEED,)):
        assert all(10 <= s < 10 + S.TRIED for s in seeds)
    assert len(S.BC_SEEDS) == len(S.BC_SHAPES) and len(S.IAM_SEEDS) == len(S.IAM_SHAPES) and S.TRIED >= 16


def test_a_table_without_one_of_its_shapes_is_noticed(monkeypatch):
    for name in ("BC_SHAPES", "IAM_SHAPES"):
        full = getattr(S, name)
        for i in range(len(full)):
            monkeypatch.setattr(S, name, full[:i] + full[i + 1:])
            if name == "IAM_SHAPES":
                monkeypatch.setattr(S, "RINGS", S.RINGS[:i] + S.RINGS[i + 1:])
            with pytest.raises(AssertionError):
                S.required_shapes_present()
            monkeypatch.undo()
    monkeypatch.setattr(S, "RINGS", tuple(max(n, s[3]) for s, n in zip(S.IAM_SHAPES, S.RINGS)))
    with pytest.raises(AssertionError, match="ring"):
        S.required_shapes_present()
    monkeypatch.undo()
    check_tables()


# ------------------------------------------------------------------------------ every case: float32 can hold it
@pytest.mark.parametrize("r", RUNS, ids=run_id)
def test_case_is_one_float32_can_hold(r):
    """The chosen seed's float32 run lies within TOL / 4 of float64 on every parameter tensor after either step; the
    scalars are finite, the second step starts from moments and statistics the first one left."""
    kind, i, logged = r
    run = run_of(kind, i)
    bc = run["bc"]
    ref, f32 = S.yardstick(run, logged)
    for s in range(S.UPDATES):
        for name, a, b in zip(S.NAMES, f32["params"][s], ref["params"][s]):
            spread = float(np.abs(a - b).max())
            print(f"{run_id(r)} step {s} {name}: float32 {spread:.3e} from float64")
            assert spread <= TOL / 4, (run_id(r), s, name, spread)
    assert ref["out"].shape == (S.UPDATES, 4 if logged else 3) and np.isfinite(ref["out"]).all() and np.isfinite(f32["out"]).all()
    # the moments after step 1 are non-zero: Adam's first step moved every tensor (it moves an entry by lr m^ / (sqrt(v^) +
    # eps), which is zero only where m is)
    for name, a, b in zip(S.NAMES, ref["params"][0], run["kk"]["params"]):
        assert float(np.abs(a - np.asarray(b, np.float64)).max()) > 0, (run_id(r), name)
    assert all(float(np.abs(m).max()) > 0 for m in ref["exp_avg"]) and all(float(v.max()) > 0 for v in ref["exp_avg_sq"])
    if bc.standardizer:
        assert np.all(ref["colstats"][0] == (4 if logged else 2) * bc.batch)
    else:
        assert ref["colstats"] is None
    # the restatement written out row by row (what the wrong reading (b) is computed from) gives the scalars back
    again = S.scalars_from(S.step_rows(run, ref, logged), bc.A)
    assert np.all(np.abs(again - ref["out"]) <= 1e-9 * np.maximum(1.0, np.abs(ref["out"]))), (again, ref["out"])
    # the yardstick against itself, and torch's float32 run against it, by the GPU test's rule
    assert S.worst(S.fit_errors(S.state_of(ref), (ref, f32))) == 0.0
    assert S.worst(S.fit_errors(S.state_of(f32), (ref, f32))) <= 1.0


# ------------------------------------------------------------------------------ each wrong reading is noticed
def _noticed(r, what, got, fourth=True):
    errs = S.fit_errors(got, S.yardstick(run_of(r[0], r[1]), r[2]), fourth=fourth)
    top = sorted(errs, key=lambda e: -e[1] / e[2])[:3]
    print(f"{run_id(r)} {what}: " + ", ".join(f"{n} {e / t:.0f}x" for n, e, t in top))
    assert S.worst(errs) >= 10, (run_id(r), what, errs)


def _fourth(r):
    """The sampled entropy of a saturated run is not compared (it is held on the twin)."""
    return not run_of(r[0], r[1])["bc"].saturated


@pytest.mark.parametrize("r", RUNS, ids=run_id)
def test_cases_notice_one_misread_position(r):
    """(a) the last position of every step's idx reads the row of position 0."""
    run = run_of(r[0], r[1])
    kk = S.misread_position(run["kk"])
    assert any(a[-1] != b[-1] for a, b in zip(kk["idx"], run["kk"]["idx"])), "the reading changes a row"
    _noticed(r, "last position misread", S.state_of(S.restate(run, logged=r[2], kk=kk)), _fourth(r))


@pytest.mark.parametrize("r", RUNS, ids=run_id)
def test_cases_notice_scalars_of_the_first_256_rows_only(r):
    """(b) a loss_tree or a bc_log_fold_kernel that folds 16 of the tiles' partials."""
    run = run_of(r[0], r[1])
    assert run["bc"].batch > S.THREADS
    ref = S.yardstick(run, r[2])[0]
    got = S.first_tiles_only(run, ref, r[2])
    _noticed(r, "scalars of the first 256 rows", got, _fourth(r))
    if r[2] and _fourth(r):      # the fourth scalar alone (bc_log_fold_kernel), the other three as they should be
        out = ref["out"].copy()
        out[:, 3] = got["out"][:, 3]
        _noticed(r, "sampled entropy of the first 256 rows", dict(got, out=out))


@pytest.mark.parametrize("logged", (False, True), ids=("plain", "logged"))
def test_scalars_at_256_rows_are_unchanged_by_that_reading(logged):
    """The largest batch of the small tables, (64, 16, 256): 16 partials are all there are."""
    c = br.CASES[5]._replace(steps=S.UPDATES)
    assert c.batch == S.THREADS
    run = S.bc_run(c)
    ref = S.restate(run, logged=logged)
    terms = S.step_rows(run, ref, logged)
    assert np.array_equal(S.scalars_from(terms, c.A, rows=S.THREADS), S.scalars_from(terms, c.A))


@pytest.mark.parametrize("r", [r for r in RUNS if run_of(r[0], r[1])["bc"].standardizer], ids=run_id)
def test_cases_notice_statistics_of_one_row_per_chain(r):
    """(c) stats_slice / pair_stats_slice with a chain loop that never iterates."""
    run = run_of(r[0], r[1])
    assert S.stat_slices(run["bc"].batch)[0] > S.WAVES
    _noticed(r, "one row per chain", S.one_row_per_chain(run, r[2]), _fourth(r))
    assert br.Standardizer.__name__ == "Standardizer", "the reading is undone"


def test_at_the_small_tables_batches_no_chain_adds_a_second_row():
    """What the issue says of the paired table's 33 rows: slices of 3 rows, so (c) changes nothing there."""
    assert max(S.stat_slices(33)) <= S.WAVES < max(S.stat_slices(256))


# ------------------------------------------------------------------------------ the workspaces
def test_workspace_sizes_for_every_shape():
    from olympic_hip import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.fail(f"{_ffi.LIB_PATH} missing: run python __graft_entry__.py build")
    L = _ffi.lib()
    shapes = [(i, a, b) for i, a, b, *_ in S.BC_SHAPES] + [(d1 + d2, a, b) for d1, d2, a, b, *_ in S.IAM_SHAPES]
    for in_dim, A, B in shapes:
        n, nl = int(L.oly_bc_fit_ws(B, in_dim, A)), int(L.oly_bc_fit_log_ws(B, in_dim, A))
        BP = S.tiles(B) * S.TILE
        # per row xs, h1, h2, dZ1, dZ2, dZ3; the transposed streams W2T [256][512] and W3T [32][256]
        assert n >= BP * (64 + 512 + 256 + 512 + 256 + 32) + 256 * 512 + 32 * 256 > 0, (B, n)
        assert nl == n + BP, (B, n, nl)
    assert int(L.oly_bc_fit_ws(4096, 64, 16)) >= 6_800_000
    for in_dim, A in ((64, 16), (1, 1), (17, 6)):
        assert int(L.oly_bc_fit_ws(S.MAX_BATCH + 1, in_dim, A)) == -1 and int(L.oly_bc_fit_log_ws(S.MAX_BATCH + 1, in_dim, A)) == -1
