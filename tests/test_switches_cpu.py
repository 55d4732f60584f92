"""The DSA_* route switches, checked without a GPU from the sources (as tests/test_routes_cpu.py does for routes and ceilings): the
environment is read only inside the two parsers (csrc/env.h, diffsptk_amd/_lib.py); a name has one default and one layer that reads
it; the table of INTEGRATION.md ("Environment switches") has exactly the names the sources read, with the defaults the sources give,
plus the two of bench.py; every name a test or a tool sets is in the table; and the two parsers agree on every kind of value, the
C++ one compiled alone into a stand-alone program that also times a read."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from diffsptk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diffsptk_amd")
CSRC = {os.path.relpath(p, ROOT): open(p).read() for p in sorted(glob.glob(os.path.join(PKG, "csrc", "*.h*")))}
PYTHON = {os.path.relpath(p, ROOT): open(p).read() for p in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))}
CALLERS = {os.path.relpath(p, ROOT): open(p).read() for d in ("tests", "tools") for p in sorted(glob.glob(os.path.join(ROOT, d, "*.py")))
           if os.path.abspath(p) != os.path.abspath(__file__)}   # (this file spells made-up names as examples for its own patterns)
TABLE = open(os.path.join(ROOT, "INTEGRATION.md")).read()
DRIVER = {"DSA_BENCH_SINGLE_DEVICE", "DSA_BENCH_BACKEND"}   # bench.py's own
TEXT = "unset"                                              # the "default" of a text-valued switch (env_text), as the table writes it


def raw_reads(texts, word, allowed):
    """["file:line", ...] of every occurrence of `word` outside the file `allowed`"""
    return [f"{name}:{text.count(chr(10), 0, m.start()) + 1}" for name, text in texts.items() if os.path.basename(name) != allowed
            for m in re.finditer(re.escape(word), text)]


def reads(texts):
    """[(name, default, "file:line"), ...] of every env_int("DSA_...", d) and env_text("DSA_...") of {file: text}"""
    return [(m.group(2), TEXT if m.group(1) == "text" else int(m.group(3)), f"{name}:{text.count(chr(10), 0, m.start()) + 1}")
            for name, text in texts.items() for m in re.finditer(r'\benv_(int|text)\(\s*"(DSA_\w+)"\s*(?:,\s*(-?\d+)\s*)?\)', text)]


def read_problems(csrc, python):
    """one sentence per name with two defaults, and per name read in both layers"""
    out, seen = [], {}
    for name, default, where in reads(csrc) + reads(python):
        seen.setdefault(name, {}).setdefault(default, []).append(where)
    out += [f"{name} has the defaults {sorted(map(str, by))}: {sorted(w for ws in by.values() for w in ws)}" for name, by in sorted(seen.items()) if len(by) > 1]
    both = {n for n, _, _ in reads(csrc)} & {n for n, _, _ in reads(python)}
    out += [f"{name} is read in csrc/ and in Python: {sorted(w for n, _, w in reads(csrc) + reads(python) if n == name)}" for name in sorted(both)]
    return out


def table_rows(text):
    """name -> the row's cells (default, values, read by, read at, selects) of the switch table"""
    return {m.group(1): [c.strip() for c in m.group(2).split("|")] for m in re.finditer(r"^\| `(DSA_\w+)` \|(.*)\|$", text, re.M)}


def table_problems(csrc, python, table):
    rows, out = table_rows(table), []
    code = {name: (default, "library" if where.startswith(os.path.join("diffsptk_amd", "csrc")) else "Python")
            for name, default, where in reads(csrc) + reads(python)}
    out += [f"{name} is read by the sources and has no row in INTEGRATION.md" for name in sorted(set(code) - set(rows))]
    out += [f"INTEGRATION.md has a row for {name}, which nothing reads" for name in sorted(set(rows) - set(code) - DRIVER)]
    out += [f"bench.py's {name} has no row in INTEGRATION.md" for name in sorted(DRIVER - set(rows))]
    for name in sorted(set(code) & set(rows)):
        default, layer = code[name]
        if rows[name][0] != str(default):
            out.append(f"{name}: default {default} in the sources, {rows[name][0]} in INTEGRATION.md")
        if rows[name][2] != layer:
            out.append(f"{name}: read by {layer}, INTEGRATION.md says {rows[name][2]}")
    return out


def set_names(texts):
    """{name: "file:line"} of the DSA_* names assigned through setenv( or environ["""
    return {m.group(1): f"{name}:{text.count(chr(10), 0, m.start()) + 1}" for name, text in texts.items()
            for m in re.finditer(r"""(?:setenv\(|environ\[)\s*["'](DSA_\w+)["']""", text)}


def test_the_environment_is_read_only_inside_the_two_parsers():
    assert raw_reads(CSRC, "getenv", "env.h") == [], "raw getenv in csrc/: use dsa::env_int / dsa::env_text (csrc/env.h)"
    assert raw_reads(PYTHON, "os.environ", "_lib.py") == [], "raw os.environ in diffsptk_amd/: use _lib.env_int / _lib.env_text"
    assert "getenv" in CSRC[os.path.join("diffsptk_amd", "csrc", "env.h")] and "os.environ" in PYTHON[os.path.join("diffsptk_amd", "_lib.py")]
    header = CSRC[os.path.join("diffsptk_amd", "csrc", "env.h")]
    assert "static" not in header and "hip" not in header.lower(), "env.h caches nothing and includes no HIP header"


def test_the_patterns_still_find_the_reads():
    text = 'a = env_int("DSA_A", 1) != 0; b = env_int( "DSA_B" , -1 );\nif (!strcmp(env_text("DSA_C"), "x")) return _lib.env_int("DSA_A", 1)'
    assert reads({"f.hip": text}) == [("DSA_A", 1, "f.hip:1"), ("DSA_B", -1, "f.hip:1"), ("DSA_C", TEXT, "f.hip:2"), ("DSA_A", 1, "f.hip:2")]
    assert len({n for n, _, _ in reads(CSRC)}) >= 14 and len({n for n, _, _ in reads(PYTHON)}) >= 11
    # every mention of a parser in code is a read the pattern understands (its own definition and documentation aside)
    for texts, own in ((CSRC, "env.h"), (PYTHON, "_lib.py")):
        n_all = sum(len(re.findall(r"\benv_(?:int|text)\(", t)) for name, t in texts.items() if os.path.basename(name) != own)
        assert n_all == len([r for r in reads(texts) if os.path.basename(r[2].split(":")[0]) != own]), (own, n_all)
    assert set_names({"t.py": 'monkeypatch.setenv("DSA_A", "0")\nos.environ[\'DSA_B\'] = "1"\nx = os.environ.get("DSA_C")'}) == {"DSA_A": "t.py:1", "DSA_B": "t.py:2"}


def test_a_name_has_one_default_and_one_layer():
    assert read_problems(CSRC, PYTHON) == []


def test_the_table_has_every_name_with_its_default_and_its_reader():
    assert table_problems(CSRC, PYTHON, TABLE) == []
    rows = table_rows(TABLE)
    assert all(len(cells) == 5 and all(cells) for cells in rows.values()), "a row of the table with a cell missing"
    at_construction = {name for name, cells in rows.items() if "construction" in cells[3]}
    assert at_construction == {"DSA_MGCEP_STEP_BWD_H"}
    assert all(cells[3] == "every call" for name, cells in rows.items() if name not in at_construction | DRIVER)


def test_every_name_a_test_or_a_tool_sets_is_in_the_table():
    rows, names = table_rows(TABLE), set_names(CALLERS)
    assert len(names) >= 15
    unknown = {name: where for name, where in names.items() if name not in rows}
    assert not unknown, f"set, and read by nothing (a mistyped or retired name): {unknown}"


def test_a_raw_read_a_second_default_and_a_missing_row_fail_by_name():
    more = dict(CSRC, **{"diffsptk_amd/csrc/new.hip": 'int f()\n{\n    return getenv("DSA_X") != nullptr;\n}'})
    assert raw_reads(more, "getenv", "env.h") == ["diffsptk_amd/csrc/new.hip:3"]
    assert raw_reads(dict(PYTHON, **{"diffsptk_amd/new.py": 'import os\nx = os.environ.get("DSA_X")'}), "os.environ", "_lib.py") == ["diffsptk_amd/new.py:2"]
    second = dict(CSRC, **{"diffsptk_amd/csrc/new.hip": 'bool on = env_int("DSA_STFT_BIG", 0) != 0;'})
    assert [p.split(":")[0] for p in read_problems(second, PYTHON)] == ["DSA_STFT_BIG has the defaults ['0', '1']"]
    twice = dict(PYTHON, **{"diffsptk_amd/new.py": 'on = _lib.env_int("DSA_MCEP_BIG", 1) != 0'})
    assert [p.split(":")[0] for p in read_problems(CSRC, twice)] == ["DSA_MCEP_BIG is read in csrc/ and in Python"]
    less = "\n".join(line for line in TABLE.splitlines() if not line.startswith("| `DSA_FREQT_GENERIC` |"))
    assert table_problems(CSRC, PYTHON, less) == ["DSA_FREQT_GENERIC is read by the sources and has no row in INTEGRATION.md"]
    other = TABLE.replace("| `DSA_MCEP_BIG_STAGGER` | 5 |", "| `DSA_MCEP_BIG_STAGGER` | 6 |")
    assert table_problems(CSRC, PYTHON, other) == ["DSA_MCEP_BIG_STAGGER: default 5 in the sources, 6 in INTEGRATION.md"]
    stale = TABLE + "\n| `DSA_GONE` | 1 | 0, 1 | library | every call | nothing |\n"
    assert table_problems(CSRC, PYTHON, stale) == ["INTEGRATION.md has a row for DSA_GONE, which nothing reads"]


# ------------------------------------------------------------------ the two parsers agree; what a read costs
PROGRAM = """#include "env.h"
#include <chrono>
#include <stdio.h>
int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    printf("%d\\n", dsa::env_int(argv[1], atoi(argv[2])));
    const auto t0 = std::chrono::steady_clock::now();
    long sum = 0;
    for (int i = 0; i < 1000000; ++i) {
        sum += dsa::env_int(argv[1], i);
        asm volatile("" ::: "memory");   // the environment may have changed: read it again
    }
    printf("%.1f ns per env_int (checksum %ld)\\n", std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / 1e6, sum);
    return 0;
}
"""
NAME = "DSA_TEST_SWITCH"
VALUES = [(None, None), ("", None), ("0", 0), ("1", 1), ("-1", -1), ("2", 2), ("11", 11), ("00", 0), (" 1", None), ("1x", None), ("abc", None),
          ("f64", None), ("1234567890", None), ("123456789", 123456789), ("-123456789", -123456789), ("-", None), ("+1", None), ("1 ", None)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    compiler = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("c++")) if c and os.path.exists(c)), None)
    if compiler is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("env")
    (d / "env_main.cpp").write_text(PROGRAM)
    exe = str(d / "env_main")
    subprocess.run([compiler, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), str(d / "env_main.cpp"), "-o", exe], check=True)
    return exe


def test_the_two_parsers_agree(program, monkeypatch):
    for value, expected in VALUES:
        for default in (-1, 0, 7):
            env = {k: v for k, v in os.environ.items() if k != NAME}
            monkeypatch.delenv(NAME, raising=False)
            if value is not None:
                env[NAME] = value
                monkeypatch.setenv(NAME, value)
            want = default if expected is None else expected
            got = int(subprocess.run([program, NAME, str(default)], env=env, check=True, capture_output=True, text=True).stdout.splitlines()[0])
            assert got == want and _lib.env_int(NAME, default) == want, (value, default, got, _lib.env_int(NAME, default), want)
    monkeypatch.setenv(NAME, "f64")
    assert _lib.env_text(NAME) == "f64"
    monkeypatch.delenv(NAME)
    assert _lib.env_text(NAME) == ""


def test_what_a_read_costs(program):
    """A record, not a threshold: 10^6 reads under this process's environment, a set variable and an unset one, printed."""
    for env in (dict(os.environ, **{NAME: "1"}), {k: v for k, v in os.environ.items() if k != NAME}):
        out = subprocess.run([program, NAME, "0"], env=env, check=True, capture_output=True, text=True).stdout.splitlines()
        print(f"{len(env)} variables, {NAME} {'set' if NAME in env else 'unset'}: {out[1]}")
        assert re.match(r"[0-9.]+ ns per env_int", out[1])
