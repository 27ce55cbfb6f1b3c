"""The ledger of tests/il_fence_ledger.py against include/olympic_hip.h, without a GPU: every entry point declared from
oly_ilmlp_packed_floats down to oly_iq_q_update is either covered by a named test that runs it on fenced and poisoned
operands, or exempt with a reason.  An entry point added to the header later (K27) fails here until someone fences it or
says why not."""
import ast
import os
import re

import il_fence_ledger as ledger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, LAST = "oly_ilmlp_packed_floats", "oly_iq_q_update"


def header_entry_points():
    """The functions the header declares from FIRST to LAST, in its order (int and int64_t results: the size queries too)."""
    with open(os.path.join(ROOT, "include", "olympic_hip.h")) as f:
        names = re.findall(r"^int(?:64_t)?\s+(oly_\w+)\s*\(", f.read(), flags=re.M)
    assert names.count(FIRST) == 1 and names.count(LAST) == 1
    return names[names.index(FIRST):names.index(LAST) + 1]


def missing(names, covered, exempt):
    return [n for n in names if n not in covered and n not in exempt]


def test_the_header_range_is_what_the_ledger_was_written_for():
    names = header_entry_points()
    assert len(names) == len(set(names)) and len(names) >= 42
    for n in ("oly_disc_fit_epoch_pair", "oly_trpo_old_offsets", "oly_il_reset_where", "oly_sg_act", "oly_iq_q_ws_values"):
        assert n in names, n
    assert "oly_event_create" not in names and "oly_disc_forward" not in names


def test_every_entry_point_is_fenced_or_exempt():
    names = header_entry_points()
    left = missing(names, ledger.COVERED, ledger.EXEMPT)
    assert not left, f"neither fenced nor exempt in tests/il_fence_ledger.py: {left}"
    both = sorted(set(ledger.COVERED) & set(ledger.EXEMPT))
    assert not both, f"both covered and exempt: {both}"
    stale = sorted((set(ledger.COVERED) | set(ledger.EXEMPT)) - set(names))
    assert not stale, f"in the ledger and not in the header's range: {stale}"
    assert all(isinstance(r, str) and len(r.strip()) > 10 and "\n" not in r for r in ledger.EXEMPT.values())


def test_a_missing_row_is_named():
    names = header_entry_points()
    covered = {k: v for k, v in ledger.COVERED.items() if k != "oly_iter_log"}
    assert missing(names, covered, ledger.EXEMPT) == ["oly_iter_log"]
    assert missing(names + ["oly_k27_update"], ledger.COVERED, ledger.EXEMPT) == ["oly_k27_update"]


def test_every_named_test_exists_and_calls_its_entry_point():
    """The function exists in the file the ledger names, and that file speaks of the entry point or of its Engine method
    (the entry point's name without oly_)."""
    trees = {}
    for entry, (fname, test) in ledger.COVERED.items():
        assert fname in (ledger.IL, ledger.K10, ledger.IQ), fname
        if fname not in trees:
            with open(os.path.join(ROOT, "tests", fname)) as f:
                src = f.read()
            trees[fname] = (src, {n.name for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)})
        src, functions = trees[fname]
        assert test.startswith("test_") and test in functions, f"{entry}: no {test} in tests/{fname}"
        assert re.search(rf"\b(oly_)?{entry[4:]}\b", src), f"{entry}: tests/{fname} never names it"
