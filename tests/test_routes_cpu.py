"""Completeness of the kernel-route table (tests/kernel_routes.py), checked without a GPU: every name a launcher of
diffsptk_amd/csrc hands to check_launch() is a key of exactly one of ROUTES, PINNED_ELSEWHERE and EXEMPT; a pointer of
PINNED_ELSEWHERE names a test function that reads last_kernel(); every measured tolerance has its base values in the table; and the
inputs of every case keep the float64 restatement itself well inside the case's bound (tests/routes_ref.py evaluated twice).  The
same for the refusals: every DSA_ERR_UNSUPPORTED of the sources is claimed by exactly one of REFUSALS, CEILINGS and NOT_A_CEILING."""
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


# ------------------------------------------------------------------ the refusals: REFUSALS, CEILINGS, NOT_A_CEILING against the sources
def unsupported_sites(texts):
    """{message: ["file:line", ...]} of every fail(DSA_ERR_UNSUPPORTED, "message" ...) of {file: text} -- adjacent literals joined, the
    trailing %s of the library's fail() dropped -- and, for the returns without a message, "return DSA_ERR_UNSUPPORTED @ file xN" """
    sites = {}
    for name, text in texts.items():
        for m in re.finditer(r'fail\(\s*DSA_ERR_UNSUPPORTED\s*,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text):
            message = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1)))
            message = message[:-2] if message.endswith("%s") and message != "%s" else message
            sites.setdefault(message, []).append(f"{name}:{text.count(chr(10), 0, m.start()) + 1}")
        bare = [text.count(chr(10), 0, m.start()) + 1 for m in re.finditer(r"return\s+DSA_ERR_UNSUPPORTED\s*;", text)]
        if bare:
            sites[f"return DSA_ERR_UNSUPPORTED @ {name} x{len(bare)}"] = [f"{name}:{n}" for n in bare]
    return sites


def source_sites():
    return unsupported_sites({os.path.basename(p): open(p).read() for p in SOURCES})


def claims():
    """table -> the messages it claims: a CEILINGS row claims what its outside raises and what its refusal shadows"""
    rows = [r for r in KR.CEILINGS if r["outside"] != KR.IN_REFUSALS]
    return {"REFUSALS": {r[4] for r in KR.REFUSALS},
            "CEILINGS": {o["message"] for r in rows for o in r["outside"] if o["expect"] == "raises"} | {m for r in KR.CEILINGS for m in r["shadowed"]},
            "NOT_A_CEILING": set(KR.NOT_A_CEILING)}


def site_problems(sites, tables):
    """what test_every_unsupported_site_is_in_exactly_one_table reports, as a list of sentences that name the site"""
    out = []
    for message, where in sorted(sites.items()):
        holders = [t for t, held in tables.items() if message in held]
        if not holders:
            out.append(f"{', '.join(where)}: \"{message}\" is in none of REFUSALS, CEILINGS, NOT_A_CEILING")
        if len(holders) > 1:
            out.append(f"{', '.join(where)}: \"{message}\" is in {' and '.join(holders)}")
    for t, held in tables.items():
        out += [f"{t} names \"{message}\", which the sources no longer have" for message in sorted(held - set(sites))]
    return out


def test_the_site_pattern_still_finds_the_messages():
    text = 'if (a) return fail(DSA_ERR_UNSUPPORTED, "x: too long%s");\nreturn fail(DSA_ERR_UNSUPPORTED,\n  "y: needs a, "\n  "b (c)%s");\n' \
           'if (b) return DSA_ERR_UNSUPPORTED;\n// DSA_ERR_UNSUPPORTED otherwise\nreturn fail(DSA_ERR_UNSUPPORTED, "%s: z", what);'
    assert unsupported_sites({"f.hip": text}) == {"x: too long": ["f.hip:1"], "y: needs a, b (c)": ["f.hip:2"], "%s: z": ["f.hip:7"],
                                                   "return DSA_ERR_UNSUPPORTED @ f.hip x1": ["f.hip:5"]}
    n_found = sum(len(w) for w in source_sites().values())
    # every other mention of the status in code (not behind //) is a comparison `== DSA_ERR_UNSUPPORTED)`: a site spelled in a way the
    # patterns above do not know would show as a difference here
    n_all = sum(len(re.findall(r"^[^/\n]*?(?<![=!] )\bDSA_ERR_UNSUPPORTED\b(?! *\))", open(p).read(), re.M)) for p in SOURCES)
    assert n_found > 100 and n_found == n_all, (n_found, n_all)


def test_every_unsupported_site_is_in_exactly_one_table():
    problems = site_problems(source_sites(), claims())
    assert not problems, "\n".join(problems)


def test_a_missing_row_and_a_new_site_fail_by_name():
    sites, tables = source_sites(), claims()
    less = dict(tables, CEILINGS=tables["CEILINGS"] - {"fftcep: fft_length above 1022 is not supported"})
    assert site_problems(sites, less) == ['fftcep.hip:344: "fftcep: fft_length above 1022 is not supported" is in none of REFUSALS, CEILINGS, NOT_A_CEILING']
    more = dict(sites, **unsupported_sites({"new.hip": 'return fail(DSA_ERR_UNSUPPORTED, "new: limit%s");'}))
    assert site_problems(more, tables) == ['new.hip:1: "new: limit" is in none of REFUSALS, CEILINGS, NOT_A_CEILING']
    twice = dict(tables, NOT_A_CEILING=tables["NOT_A_CEILING"] | {"acorr: frame too long for LDS"})
    assert site_problems(sites, twice) == ['lpc.hip:357: "acorr: frame too long for LDS" is in REFUSALS and NOT_A_CEILING']
    stale = dict(tables, REFUSALS=tables["REFUSALS"] | {"gone: message"})
    assert site_problems(sites, stale) == ['REFUSALS names "gone: message", which the sources no longer have']


def pointer_exists(pointer):
    path, _, func = pointer.partition("::")
    return path.startswith("tests/") and os.path.exists(os.path.join(ROOT, path)) and f"def {func}(" in open(os.path.join(ROOT, path)).read()


def test_ceiling_rows_point_at_their_conditions_and_are_reasoned():
    sites = source_sites()
    refused = {r[4] for r in KR.REFUSALS}
    for row in KR.CEILINGS:
        for where in row["where"]:
            path, line = where.rsplit(":", 1)
            text = open(os.path.join(ROOT, "diffsptk_amd", path)).read().splitlines()
            assert 1 <= int(line) <= len(text), where
            if not row["says"].startswith("reshapes"):   # a refusal: the line is a site of the row's message, or the condition within 20 lines above one
                lines = [int(w.rsplit(":", 1)[1]) for m in (row["says"],) + row["shadowed"] for w in sites[m] if w.startswith(os.path.basename(path) + ":")]
                assert any(0 <= n - int(line) <= 20 for n in lines), f"{where} is not where \"{row['says']}\" is raised (the row is stale): {sites[row['says']]}"
        assert row["inside"] or row["cited"], row["where"]
        if row["outside"] == KR.IN_REFUSALS:
            assert row["says"] in refused, row["says"]
        else:
            assert row["outside"] and all(o["expect"] in ("raises", "route") for o in row["outside"]), row["where"]
            assert all(o["text"].split(":")[-1] in o["message"] for o in row["outside"] if o["expect"] == "raises"), row["where"]
        assert row["cited"] is None or pointer_exists(row["cited"]), row["cited"]
    assert all(pointer_exists(p) for p in KR.LDS_FIXED.values())
    assert set(KR.LDS_FIXED) <= collected() | set(KR.FORWARDED)
    assert all(isinstance(why, str) and len(why.split()) >= 3 for why in KR.NOT_A_CEILING.values())


def test_ceiling_bounds_meet_the_cap():
    """a case at a ceiling whose bound exceeds 1e-3 (float32) or 1e-9 (float64) tests too little: its inputs are chosen for that"""
    for row in KR.CEILINGS:
        sides = list(row["inside"]) + ([] if row["outside"] == KR.IN_REFUSALS else [(o["route"], o["case"]) for o in row["outside"] if o["expect"] == "route"])
        for route, c in sides:
            for dt in c["dtypes"]:
                assert KR.tolerance(route, c, dt) <= (1e-3 if dt == "f32" else 1e-9), (KR.case_id(route, c), dt, KR.tolerance(route, c, dt))


ALL = KR.all_cases()


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
