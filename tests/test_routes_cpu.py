"""Completeness of the kernel-route table (tests/kernel_routes.py), checked without a GPU: every name a launcher of
diffsptk_amd/csrc hands to check_launch() is a key of exactly one of ROUTES, PINNED_ELSEWHERE and EXEMPT; a pointer of
PINNED_ELSEWHERE names a test function that reads last_kernel(); every measured tolerance has its base values in the table; and the
inputs of every case keep the float64 restatement itself well inside the case's bound (tests/routes_ref.py evaluated twice)."""
import ast
import glob
import os
import re

import pytest

import kernel_routes as KR
import routes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = sorted(glob.glob(os.path.join(ROOT, "diffsptk_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "diffsptk_amd", "csrc", "*.h")))


def launch_names(text):
    """every double-quoted literal inside the parentheses of a check_launch(...) call (a ternary gives two names)"""
    names = set()
    for m in re.finditer(r"\bcheck_launch\(", text):
        depth, j = 1, m.end()
        while depth and j < len(text):
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        names.update(re.findall(r'"([^"]+)"', text[m.end():j]))
    return names


def collected():
    return set().union(*(launch_names(open(p).read()) for p in SOURCES))


def test_the_pattern_still_finds_the_names():
    assert launch_names('return check_launch(bwd ? "a_bwd" : "a_fwd"); x = check_launch(f(1) ? "b"\n : "c");') == {"a_bwd", "a_fwd", "b", "c"}
    assert len(collected()) > 100


def test_forwarded_names_are_spelled_where_the_table_says():
    for name, where in KR.FORWARDED.items():
        path, line = where.rsplit(":", 1)
        text = open(os.path.join(ROOT, "diffsptk_amd", path)).read().splitlines()
        near = "\n".join(text[max(int(line) - 3, 0):int(line) + 2])
        assert f'"{name}"' in near, f"{where} does not spell \"{name}\" (the table's FORWARDED entry is stale)"
    assert not set(KR.FORWARDED) & collected(), "a FORWARDED name is a literal of a check_launch() call: drop it from FORWARDED"


def test_every_route_is_in_exactly_one_table():
    routes = collected() | set(KR.FORWARDED)
    tables = {"ROUTES": set(KR.ROUTES), "PINNED_ELSEWHERE": set(KR.PINNED_ELSEWHERE), "EXEMPT": set(KR.EXEMPT)}
    claimed = set().union(*tables.values())
    missing = routes - claimed
    assert not missing, f"routes of the library that no table of tests/kernel_routes.py names: {sorted(missing)} -- give each a case in ROUTES"
    stale = claimed - routes
    assert not stale, f"tests/kernel_routes.py names routes the sources do not have: {sorted(stale)}"
    for a, b in (("ROUTES", "PINNED_ELSEWHERE"), ("ROUTES", "EXEMPT"), ("PINNED_ELSEWHERE", "EXEMPT")):
        assert not tables[a] & tables[b], f"in both {a} and {b}: {sorted(tables[a] & tables[b])}"
    assert all(cases for cases in KR.ROUTES.values()), "a route of ROUTES without a case"


def test_exemptions_are_few_and_reasoned():
    assert len(KR.EXEMPT) <= 5
    assert all(isinstance(reason, str) and len(reason.split()) >= 3 for reason in KR.EXEMPT.values())


def test_pinned_elsewhere_points_at_tests_that_read_last_kernel():
    for route, pointer in KR.PINNED_ELSEWHERE.items():
        path, _, func = pointer.partition("::")
        assert path.startswith("tests/") and os.path.exists(os.path.join(ROOT, path)), (route, pointer)
        src = open(os.path.join(ROOT, path)).read()
        nodes = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == func]
        assert func.startswith("test_") and nodes, f"{pointer} (for {route}) is not a test function of {path}"
        assert "last_kernel" in ast.get_source_segment(src, nodes[0]), f"{pointer} (for {route}) does not read last_kernel()"


ALL = [(route, c) for route, cases in KR.ROUTES.items() for c in cases]


def test_cases_are_well_formed_and_measured_ones_have_their_base_values():
    ids = [KR.case_id(route, c) for route, c in ALL]
    assert len(ids) == len(set(ids))
    for route, c in ALL:
        assert c["call"] in R.REFS and c["call"] in R.INPUTS and c["when"] in ("fwd", "bwd") and c["metric"] in ("max", "rows"), (route, c)
        assert set(c["dtypes"]) <= {"f64", "f32"} and c["dtypes"] and (c["when"] == "fwd") == (not c["wrt"]), (route, c)
        if c["tol_from"] == KR.MEAS:
            assert KR.case_id(route, c) in KR.MEASURED, f"no base values for {KR.case_id(route, c)}: run python tests/routes_ref.py"
        else:
            path, _, func = c["tol_from"].partition("::")
            assert os.path.exists(os.path.join(ROOT, path)) and f"def {func}(" in open(os.path.join(ROOT, path)).read(), (route, c["tol_from"])
            assert all(c["tol"][dt == "f32"] is not None for dt in c["dtypes"]), (route, c)
    measured = {KR.case_id(route, c) for route, c in ALL if c["tol_from"] == KR.MEAS}
    assert set(KR.MEASURED) == measured, f"base values of no case: {sorted(set(KR.MEASURED) - measured)}"
    assert KR.tolerance("levdur_fwd", KR.ROUTES["levdur_fwd"][0], "f64") == 64 * max(KR.MEASURED[KR.case_id("levdur_fwd", KR.ROUTES["levdur_fwd"][0])][0], 2.0 ** -53)


@pytest.mark.parametrize("route,c", ALL, ids=[KR.case_id(route, c) for route, c in ALL])
def test_inputs_keep_the_reference_inside_the_bound(route, c):
    """The restatement evaluated twice in float64 (opposite summation order) and once in float32, on the case's inputs: both differences
    stay below the case's bound -- a measured bound is 64 (8) times what was measured when the table was written, so this also says that
    the measurement reproduces here within that margin."""
    for dt, base in zip(("f64", "f32"), R.bases(c)):
        if dt in c["dtypes"] and (dt == "f64" or c["tol_from"] == KR.MEAS):   # (a bound taken from a kernel's own test says nothing about float32 torch)
            assert base <= KR.tolerance(route, c, dt), (dt, base, KR.tolerance(route, c, dt))
