"""The ledger of tests/il_fence_ledger.py against include/olympic_hip.h, without a GPU: every function the header
declares with an int or int64_t result, from its first to its last, is either covered by a named test that runs it on
fenced and poisoned operands, or exempt with a reason.  An entry point added to the header later fails here until someone
fences it or says why not."""
import ast
import os
import re

import il_fence_ledger as ledger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = (ledger.ENV, ledger.IL, ledger.K10, ledger.IQ, ledger.IQ_PI)


def header_entry_points():
    """The functions the header declares, in its order (int and int64_t results: the size queries too)."""
    with open(os.path.join(ROOT, "include", "olympic_hip.h")) as f:
        return re.findall(r"^int(?:64_t)?\s+(oly_\w+)\s*\(", f.read(), flags=re.M)


def missing(names, covered, exempt):
    return [n for n in names if n not in covered and n not in exempt]


def test_the_header_range_is_what_the_ledger_was_written_for():
    """The whole header: the oldest kernels, the batchers and the event utilities are inside it."""
    names = header_entry_points()
    assert len(names) == len(set(names)) and len(names) >= 120
    assert names.index("oly_create") <= 1 and names[-1] == "oly_stream_sync"
    for n in ("oly_il_step", "oly_a3_batcher_step", "oly_return_scan_stats", "oly_ppo_loss", "oly_ppo_update_epoch",
              "oly_disc_fit_epoch_pair", "oly_trpo_old_offsets", "oly_il_reset_where", "oly_sg_act", "oly_iq_q_ws_values",
              "oly_iq_alpha_update"):
        assert n in names, n
    assert "oly_event_create" in names and "oly_disc_forward" in names


def test_every_entry_point_is_fenced_or_exempt():
    names = header_entry_points()
    left = missing(names, ledger.COVERED, ledger.EXEMPT)
    assert not left, f"neither fenced nor exempt in tests/il_fence_ledger.py: {left}"
    both = sorted(set(ledger.COVERED) & set(ledger.EXEMPT))
    assert not both, f"both covered and exempt: {both}"
    stale = sorted((set(ledger.COVERED) | set(ledger.EXEMPT)) - set(names))
    assert not stale, f"in the ledger and not in the header: {stale}"
    assert all(isinstance(r, str) and len(r.strip()) > 10 and "\n" not in r for r in ledger.EXEMPT.values())


def test_a_missing_row_is_named():
    names = header_entry_points()
    for gone in ("oly_iter_log", "oly_il_step", "oly_col_stats", "oly_iq_alpha_update"):
        covered = {k: v for k, v in ledger.COVERED.items() if k != gone}
        assert missing(names, covered, ledger.EXEMPT) == [gone]
    assert missing(names + ["oly_k28_update"], ledger.COVERED, ledger.EXEMPT) == ["oly_k28_update"]


def test_every_named_test_exists_and_calls_its_entry_point():
    """The function exists in the file the ledger names, and that file speaks of the entry point or of its Engine method
    (the entry point's name without oly_)."""
    trees = {}
    for entry, (fname, test) in ledger.COVERED.items():
        assert fname in FILES, fname
        if fname not in trees:
            with open(os.path.join(ROOT, "tests", fname)) as f:
                src = f.read()
            trees[fname] = (src, {n.name for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)})
        src, functions = trees[fname]
        assert test.startswith("test_") and test in functions, f"{entry}: no {test} in tests/{fname}"
        assert re.search(rf"\b(oly_)?{entry[4:]}\b", src), f"{entry}: tests/{fname} never names it"
