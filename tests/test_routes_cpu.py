"""Completeness of the kernel-route table (tests/kernel_routes.py), checked without a GPU: every name a launcher of
diffsptk_amd/csrc hands to check_launch() is a key of exactly one of ROUTES, PINNED_ELSEWHERE and EXEMPT; a pointer of
PINNED_ELSEWHERE names a test function that reads last_kernel(); every check_launch() argument that is neither a literal nor a name
table is followed to the literals assigned to it, or to a FORWARDED anchor in its file; every measured tolerance has its base values in the table; and the
inputs of every case keep the float64 restatement itself well inside the case's bound (tests/routes_ref.py evaluated twice).  The
same for the refusals: every DSA_ERR_UNSUPPORTED of the sources is claimed by exactly one of REFUSALS, CEILINGS and NOT_A_CEILING.

The tables point into the sources as "csrc/<file>::<function>"; function_span() finds the definition, so nothing here depends on a line
number.  Every test that reads the sources takes them as `texts` ({file: text}, by default the files as they are): the last tests of
that kind run all of them again on shifted sources, and on sources in which an anchored function was renamed."""
import ast
import glob
import os
import re

import pytest

import kernel_routes as KR
import routes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = sorted(glob.glob(os.path.join(ROOT, "diffsptk_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "diffsptk_amd", "csrc", "*.h")))
TEXTS = {os.path.basename(p): open(p).read() for p in SOURCES}   # {file: text}: what every check of the sources below reads
NAME_TABLE = re.compile(r"\bconst\s+char\s*\*\s*const\s+(k\w+(?:Routes|Names))\s*(?:\[[^\]]*\]\s*)+=\s*\{(.*?)\}\s*;", re.S)


def launch_arguments(text):
    """what stands between the parentheses of every check_launch(...) call"""
    out = []
    for m in re.finditer(r"\bcheck_launch\(", text):
        depth, j = 1, m.end()
        while depth and j < len(text):
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append(text[m.end():j])
    return out


def name_tables(text):
    """{identifier: its literals} of every array declared `const char* const k<Name>Routes[...]` or `k<Name>Names[...]`, of any rank,
    up to its `};`"""
    return {m.group(1): set(re.findall(r'"([^"]+)"', m.group(2))) for m in NAME_TABLE.finditer(text)}


def launch_names(text):
    """every double-quoted literal inside the parentheses of a check_launch(...) call (a ternary gives two names), and every literal of
    a name table (a launcher indexes it on its way to check_launch(): test_no_name_table_is_dead)"""
    return set().union(*(re.findall(r'"([^"]+)"', a) for a in launch_arguments(text)), *name_tables(text).values())


def collected(texts=TEXTS):
    return set().union(*(launch_names(t) for t in texts.values()))


def function_span(texts, where, row):
    """(file, first line, last line) of the definition that where = "csrc/<file>::<function>" names in {file: text}, lines counted from 1.
    The layout of the sources makes this short: a definition starts at column 0 and is the text up to its `{` (no `;`: that is a
    declaration), the body closes with the next `}` at column 0, and what else starts at column 0 inside a body is a preprocessor line.
    Fails by `row`, the table entry that holds the anchor, unless the file defines the function exactly once."""
    path, _, fn = where.partition("::")
    file = os.path.basename(path)
    assert path == "csrc/" + file and fn and file in texts, f"{row}: {where} is not csrc/<file>::<function> of a source file"
    text = texts[file]
    heads = list(re.finditer(r"^(?![#/}\s])[^;{}]*?\b%s\s*\([^;{}]*\{" % re.escape(fn), text, re.M))
    assert len(heads) == 1, f"{row}: {where} is defined {len(heads)} times in that file, not once (the anchor is stale)"
    close = re.compile(r"^\}", re.M).search(text, heads[0].end())
    assert close, f"{row}: the body of {where} does not close at column 0"
    return file, text.count("\n", 0, heads[0].start()) + 1, text.count("\n", 0, close.start()) + 1


def test_the_pattern_still_finds_the_names(texts=TEXTS):
    assert launch_names('return check_launch(bwd ? "a_bwd" : "a_fwd"); x = check_launch(f(1) ? "b"\n : "c");') == {"a_bwd", "a_fwd", "b", "c"}
    tables = 'const char* const kAbNames[] = {"n0", "n1"};\nconst char* const kCdRoutes[2][1][2] = {\n    {{"r0_f32", "r0_f64"}},\n' \
             '    {{"r1_f32", "r1_f64"}},\n};\nconst char* other[] = {"no"};\nconst char* const kEfRoutes[1][2] = {\n    {"e_f32", "e_f64"}};\n' \
             'int f() { return check_launch(kCdRoutes[0][0][1]); }'
    assert name_tables(tables) == {"kAbNames": {"n0", "n1"}, "kCdRoutes": {"r0_f32", "r0_f64", "r1_f32", "r1_f64"}, "kEfRoutes": {"e_f32", "e_f64"}}
    assert launch_names(tables) == {"n0", "n1", "r0_f32", "r0_f64", "r1_f32", "r1_f64", "e_f32", "e_f64"}
    assert dead_tables(tables) == ["kAbNames", "kEfRoutes"]
    assert dead_tables(tables + "\nvoid g(const char*& route) { route = kEfRoutes[0][1]; }\nint h() { return rc ? rc : check_launch(route); }") == ["kAbNames"]
    assert len(collected(texts)) > 100 and sum(len(name_tables(t)) for t in texts.values()) >= 9


def dead_tables(text):
    """the name tables of `text` that no check_launch(...) call reads, neither by name nor through a variable assigned from one"""
    args = launch_arguments(text)
    dead = []
    for table in name_tables(text):
        through = [table] + re.findall(r"\b(\w+)\s*=\s*%s\b" % table, text)
        if not any(re.search(r"\b%s\b" % v, a) for v in through for a in args):
            dead.append(table)
    return sorted(dead)


def test_no_name_table_is_dead(texts=TEXTS):
    """a table nothing launches with must not feed names to the tables of tests/kernel_routes.py"""
    for name, text in texts.items():
        assert not dead_tables(text), f"{name}: no check_launch() call is given a name of {dead_tables(text)}"


def test_function_spans_are_the_definitions():
    text = "int f(int a);\n\n// f(x) {\ntemplate <typename T>\nstatic int f(int a,\n          int b)\n{\n#if X\n    if (a) { g(a); }\n#endif\n    return b;\n}\n\n" \
           "int g(int a) { return a; }\nint g(int a)\n{\n    return f(a, a);\n}\n"
    assert function_span({"x.hip": text}, "csrc/x.hip::f", "row") == ("x.hip", 4, 12)
    with pytest.raises(AssertionError, match=r"row R: csrc/x.hip::g is defined 2 times"):
        function_span({"x.hip": text}, "csrc/x.hip::g", "row R")
    with pytest.raises(AssertionError, match=r"row R: csrc/x.hip::h is defined 0 times"):
        function_span({"x.hip": text}, "csrc/x.hip::h", "row R")
    with pytest.raises(AssertionError, match=r"row R: csrc/y.hip::f is not csrc/<file>::<function> of a source file"):
        function_span({"x.hip": text}, "csrc/y.hip::f", "row R")


def test_forwarded_names_are_spelled_where_the_table_says(texts=TEXTS):
    for name, where in KR.FORWARDED.items():
        file, first, last = function_span(texts, where, f'FORWARDED["{name}"]')
        body = "\n".join(texts[file].splitlines()[first - 1:last])
        assert f'"{name}"' in body, f"FORWARDED[\"{name}\"]: {where} does not spell \"{name}\" (the entry is stale)"
    assert not set(KR.FORWARDED) & collected(texts), "a FORWARDED name is a literal of a check_launch() call or of a name table: drop it from FORWARDED"


def test_every_route_is_in_exactly_one_table(texts=TEXTS):
    routes = collected(texts) | set(KR.FORWARDED)
    tables = {"ROUTES": set(KR.ROUTES), "PINNED_ELSEWHERE": set(KR.PINNED_ELSEWHERE), "EXEMPT": set(KR.EXEMPT)}
    claimed = set().union(*tables.values())
    missing = routes - claimed
    assert not missing, f"routes of the library that no table of tests/kernel_routes.py names: {sorted(missing)} -- give each a case in ROUTES"
    stale = claimed - routes
    assert not stale, f"tests/kernel_routes.py names routes the sources do not have: {sorted(stale)}"
    for a, b in (("ROUTES", "PINNED_ELSEWHERE"), ("ROUTES", "EXEMPT"), ("PINNED_ELSEWHERE", "EXEMPT")):
        assert not tables[a] & tables[b], f"in both {a} and {b}: {sorted(tables[a] & tables[b])}"
    assert all(cases for cases in KR.ROUTES.values()), "a route of ROUTES without a case"


def argument_problems(texts, forwarded):
    """What test_every_check_launch_argument_is_accounted_for reports, as sentences that name the file and the route: every argument of
    a check_launch(...) call either holds a literal or names a name table (collected() has those), or is an identifier V.  If the file
    assigns V (`V = ...;`, a declaration included), every literal of the right-hand sides is a collected name or a key of `forwarded`;
    a name table there counts as collected.  If the file never assigns V, V is a parameter, and an anchor of `forwarded` points into
    the file: the callers' names are then held by test_forwarded_names_are_spelled_where_the_table_says."""
    names, out = collected(texts), []
    for file, text in sorted(texts.items()):
        code = re.sub(r"//[^\n]*", "", text)
        tables = name_tables(code)
        for arg in sorted(set(launch_arguments(code))):
            arg = arg[:-1].strip()
            if re.fullmatch(r"const\s+char\s*\*\s*\w+", arg):   # the definition of check_launch itself (csrc/common.h)
                continue
            if '"' in arg or any(re.search(r"\b%s\b" % t, arg) for t in tables):
                continue
            if not re.fullmatch(r"[A-Za-z_]\w*", arg):
                out.append(f"{file}: check_launch({arg}) holds no literal, names no name table and is no identifier")
                continue
            assigned = re.findall(r"\b%s\s*=(?!=)([^;]*);" % arg, code)
            if not assigned and not any(where.startswith(f"csrc/{file}::") for where in forwarded.values()):
                out.append(f"{file}: check_launch({arg}) gets a parameter, and no FORWARDED anchor points into {file}")
            for rhs in assigned:
                for name in re.findall(r'"([^"]+)"', rhs):
                    if name not in names and name not in forwarded:
                        out.append(f"{file}: \"{name}\" reaches check_launch({arg}) through `{arg} = ...` and is neither collected nor in FORWARDED")
    return out


def test_every_check_launch_argument_is_accounted_for(texts=TEXTS):
    """collected() reads literals inside check_launch(...) and inside name tables only: a launcher that keeps its names in a local was
    invisible to test_every_route_is_in_exactly_one_table (csrc/pitch_spec.hip went in that way, with none of its six names in a table)"""
    problems = argument_problems(texts, KR.FORWARDED)
    assert not problems, "\n".join(problems)
    # the tables as they were before the six names of csrc/pitch_spec.hip were registered: exactly those six, by file and name
    six = sorted(f"pitch_spec{e}_{d}" for e in ("", "_vjp_frames", "_vjp_gather") for d in ("f32", "f64"))
    before = {name: where for name, where in KR.FORWARDED.items() if name not in six}
    assert len(before) == len(KR.FORWARDED) - 6
    assert sorted(argument_problems(texts, before)) == [
        f'pitch_spec.hip: "{name}" reaches check_launch(route) through `route = ...` and is neither collected nor in FORWARDED' for name in six]
    # doctored sources: a local with an unregistered name beside a registered table, a parameter in a file nothing points into, a call
    launcher = 'const char* const kAbNames[] = {"n0", "n1"};\nint f(int dtype)\n{\n    const char* route = dtype ? "new_f64" : "n0";\n' \
               '    // route = "in_a_comment";\n    if (route == nullptr) route = kAbNames[1];\n    return check_launch(route);\n}\n'
    assert argument_problems({"new.hip": launcher}, {}) == [
        'new.hip: "new_f64" reaches check_launch(route) through `route = ...` and is neither collected nor in FORWARDED']
    assert argument_problems({"new.hip": launcher}, {"new_f64": "csrc/new.hip::f"}) == []
    shared = "int launch(const char* name)\n{\n    return check_launch(name);\n}\n"
    assert argument_problems({"new.hip": shared}, {"x": "csrc/other.hip::f"}) == [
        "new.hip: check_launch(name) gets a parameter, and no FORWARDED anchor points into new.hip"]
    assert argument_problems({"new.hip": shared}, {"x": "csrc/new.hip::g"}) == []
    assert argument_problems({"new.hip": "int f() { return check_launch(pick(1)); }\ninline int check_launch(const char* name);\n"}, {}) == [
        "new.hip: check_launch(pick(1)) holds no literal, names no name table and is no identifier"]


def test_exemptions_are_few_and_reasoned():
    assert len(KR.EXEMPT) <= 5
    assert all(isinstance(reason, str) and len(reason.split()) >= 3 for reason in KR.EXEMPT.values())


def reads_last_kernel(src, func):
    """whether function `func` of the module text `src` mentions last_kernel, itself or in a function of the module that it names (the
    newer families read the name in a helper that returns it beside the result)"""
    defs = {n.name: n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef)}
    todo, seen = [func], set()
    while todo:
        f = todo.pop()
        if f in defs and f not in seen:
            seen.add(f)
            if "last_kernel" in ast.get_source_segment(src, defs[f]):
                return True
            todo += [n.id for n in ast.walk(defs[f]) if isinstance(n, ast.Name)]
    return False


def test_pinned_elsewhere_points_at_tests_that_read_last_kernel():
    read = {}
    for route, pointer in KR.PINNED_ELSEWHERE.items():
        path, _, func = pointer.partition("::")
        assert path.startswith("tests/") and os.path.exists(os.path.join(ROOT, path)), (route, pointer)
        src = open(os.path.join(ROOT, path)).read()
        assert func.startswith("test_") and re.search(r"^def %s\(" % func, src, re.M), f"{pointer} (for {route}) is not a test function of {path}"
        if pointer not in read:
            read[pointer] = reads_last_kernel(src, func)
        assert read[pointer], f"{pointer} (for {route}) does not read last_kernel()"
    assert not reads_last_kernel("def helper():\n    return 1\n\ndef test_a():\n    assert helper()\n", "test_a")
    assert reads_last_kernel("def run():\n    return _lib.last_kernel()\n\ndef result():\n    return run()\n\ndef test_a():\n    assert result()\n", "test_a")


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


def test_the_site_pattern_still_finds_the_messages(texts=TEXTS):
    text = 'if (a) return fail(DSA_ERR_UNSUPPORTED, "x: too long%s");\nreturn fail(DSA_ERR_UNSUPPORTED,\n  "y: needs a, "\n  "b (c)%s");\n' \
           'if (b) return DSA_ERR_UNSUPPORTED;\n// DSA_ERR_UNSUPPORTED otherwise\nreturn fail(DSA_ERR_UNSUPPORTED, "%s: z", what);'
    assert unsupported_sites({"f.hip": text}) == {"x: too long": ["f.hip:1"], "y: needs a, b (c)": ["f.hip:2"], "%s: z": ["f.hip:7"],
                                                   "return DSA_ERR_UNSUPPORTED @ f.hip x1": ["f.hip:5"]}
    n_found = sum(len(w) for w in unsupported_sites(texts).values())
    # every other mention of the status in code (not behind //) is a comparison `== DSA_ERR_UNSUPPORTED)`: a site spelled in a way the
    # patterns above do not know would show as a difference here
    n_all = sum(len(re.findall(r"^[^/\n]*?(?<![=!] )\bDSA_ERR_UNSUPPORTED\b(?! *\))", text, re.M)) for text in texts.values())
    # (73 sites since the 55 spellings of the dtype refusal became the one of csrc/common.h; the floor only says that the pattern works)
    assert n_found > 60 and n_found == n_all, (n_found, n_all)


def test_every_unsupported_site_is_in_exactly_one_table(texts=TEXTS):
    problems = site_problems(unsupported_sites(texts), claims())
    assert not problems, "\n".join(problems)


def test_a_missing_row_and_a_new_site_fail_by_name(texts=TEXTS):
    sites, tables = unsupported_sites(texts), claims()
    fftcep, acorr = "fftcep: fft_length above 1022 is not supported", "acorr: frame too long for LDS"
    assert len(sites[fftcep]) == len(sites[acorr]) == 1 and sites[fftcep][0].startswith("fftcep.hip:") and sites[acorr][0].startswith("lpc.hip:")
    less = dict(tables, CEILINGS=tables["CEILINGS"] - {fftcep})
    assert site_problems(sites, less) == [f'{sites[fftcep][0]}: "{fftcep}" is in none of REFUSALS, CEILINGS, NOT_A_CEILING']
    more = dict(sites, **unsupported_sites({"new.hip": 'return fail(DSA_ERR_UNSUPPORTED, "new: limit%s");'}))
    assert site_problems(more, tables) == ['new.hip:1: "new: limit" is in none of REFUSALS, CEILINGS, NOT_A_CEILING']
    twice = dict(tables, NOT_A_CEILING=tables["NOT_A_CEILING"] | {acorr})
    assert site_problems(sites, twice) == [f'{sites[acorr][0]}: "{acorr}" is in REFUSALS and NOT_A_CEILING']
    stale = dict(tables, REFUSALS=tables["REFUSALS"] | {"gone: message"})
    assert site_problems(sites, stale) == ['REFUSALS names "gone: message", which the sources no longer have']


def pointer_exists(pointer):
    path, _, func = pointer.partition("::")
    return path.startswith("tests/") and os.path.exists(os.path.join(ROOT, path)) and f"def {func}(" in open(os.path.join(ROOT, path)).read()


def test_ceiling_rows_point_at_their_conditions_and_are_reasoned(texts=TEXTS):
    sites = unsupported_sites(texts)
    refused = {r[4] for r in KR.REFUSALS}
    for row in KR.CEILINGS:
        for where in row["where"]:
            file, first, last = function_span(texts, where, f"the CEILINGS row \"{row['says']}\"")   # (a row that reshapes: the function exists)
            if not row["says"].startswith("reshapes"):   # a refusal: the function holds a site of the row's message, or of one it shadows
                lines = [int(w.rsplit(":", 1)[1]) for m in (row["says"],) + row["shadowed"] for w in sites[m] if w.startswith(file + ":")]
                assert any(first <= n <= last for n in lines), f"{where} is not where \"{row['says']}\" is raised (the row is stale): {sites[row['says']]}"
        assert row["inside"] or row["cited"], row["where"]
        if row["outside"] == KR.IN_REFUSALS:
            assert row["says"] in refused, row["says"]
        else:
            assert row["outside"] and all(o["expect"] in ("raises", "route") for o in row["outside"]), row["where"]
            assert all(o["text"].split(":")[-1] in o["message"] for o in row["outside"] if o["expect"] == "raises"), row["where"]
        assert row["cited"] is None or pointer_exists(row["cited"]), row["cited"]
    assert all(pointer_exists(p) for p in KR.LDS_FIXED.values())
    assert set(KR.LDS_FIXED) <= collected(texts) | set(KR.FORWARDED)
    assert all(isinstance(why, str) and len(why.split()) >= 3 for why in KR.NOT_A_CEILING.values())


# ------------------------------------------------------------------ the anchors: an edit elsewhere in a file leaves them valid, a renamed function does not
SOURCE_CHECKS = [f for name, f in sorted(globals().items()) if name.startswith("test_") and f.__code__.co_varnames[:f.__code__.co_argcount] == ("texts",)]


def test_shifted_sources_pass():
    """three blank lines in front of every file: every site is reported three lines further down, the names are the same, and every check
    of the sources passes with no table edited"""
    moved = {name: "\n\n\n" + text for name, text in TEXTS.items()}
    down = {m: [f"{w.rsplit(':', 1)[0]}:{int(w.rsplit(':', 1)[1]) + 3}" for w in where] for m, where in unsupported_sites(TEXTS).items()}
    assert unsupported_sites(moved) == down and collected(moved) == collected(TEXTS)
    _, first, last = function_span(TEXTS, "csrc/lpc.hip::acorr_fwd_impl", "-")
    assert function_span(moved, "csrc/lpc.hip::acorr_fwd_impl", "-") == ("lpc.hip", first + 3, last + 3)
    assert len(SOURCE_CHECKS) == 9   # every test above that reads the sources takes them as `texts`
    for check in SOURCE_CHECKS:
        check(moved)


def test_a_stale_anchor_fails_by_name():
    renamed = dict(TEXTS, **{"lpc.hip": TEXTS["lpc.hip"].replace("acorr_fwd_impl", "acorr_forward_impl")})
    with pytest.raises(AssertionError, match=r'the CEILINGS row "acorr: frame too long for LDS": csrc/lpc\.hip::acorr_fwd_impl is defined 0 times'):
        test_ceiling_rows_point_at_their_conditions_and_are_reasoned(renamed)
    renamed = dict(TEXTS, **{"fbank.hip": TEXTS["fbank.hip"].replace("fbank_mfma_launch(", "fbank_mfma_start(")})
    with pytest.raises(AssertionError, match=r'FORWARDED\["fbank_mfma_fwd"\]: csrc/fbank\.hip::fbank_mfma_launch is defined 0 times'):
        test_forwarded_names_are_spelled_where_the_table_says(renamed)
    # the function is there and the site has left it: the condition moved to another function
    moved = dict(TEXTS, **{"lpc.hip": TEXTS["lpc.hip"].replace("static int acorr_fwd_impl(", "static int acorr_fwd_impl(int)\n{\n    return 0;\n}\n\nstatic int acorr_fwd_rest(")})
    with pytest.raises(AssertionError, match=r'csrc/lpc\.hip::acorr_fwd_impl is not where "acorr: frame too long for LDS" is raised'):
        test_ceiling_rows_point_at_their_conditions_and_are_reasoned(moved)


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
