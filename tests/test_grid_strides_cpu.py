"""Completeness of the capped grids' table (tests/grid_strides.py), checked without a GPU: every `__global__` kernel of
diffsptk_amd/csrc whose body mentions `gridDim.` is a key of exactly one of CAPPED, PINNED_ELSEWHERE and OUT_OF_REACH; a CAPPED entry's
cap is spelled, in the file it names, on a line that sizes a grid; a pointer of PINNED_ELSEWHERE names a test function that exists; and
every case's batch exceeds its cap by rows that differ from the rows of the trip before (the cap in rows is no multiple of 251)."""
import glob
import os
import re

import pytest

import grid_strides as GS
import kernel_routes as KR
import routes_ref

KR_CALLS = set(routes_ref.NAMES)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffsptk_amd", "csrc")
SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
# the head of a device-side function: `__global__` or `__device__`, anything but a parenthesis, a brace or a semicolon, then NAME(
HEAD = re.compile(r"\b(__global__|__device__)\b[^;{}()]*?\b(\w+)\s*\(", re.S)


def without_launch_bounds(text):
    """`__launch_bounds__(...)` blanked, nested parentheses included (they would end a head early); offsets stay"""
    out, at = list(text), 0
    while (at := text.find("__launch_bounds__", at)) >= 0:
        j = text.index("(", at)
        depth, k = 1, j + 1
        while depth:
            depth += {"(": 1, ")": -1}.get(text[k], 0)
            k += 1
        out[at:k] = " " * (k - at)
        at = k
    return "".join(out)

SIZES_A_GRID = re.compile(r"\b(grid|blocks|pq_blocks|wgs|waves|dim3|g2)\b")


def sizes_a_grid_with(cap, line):
    """the cap as the whole right-hand side of a comparison or an assignment (`> 256)`, `= 256;`, `< (1 << 14) ?`) on a line that
    names a grid: `256` is not found in `256L * 16`, nor in `dim3(256)`"""
    whole = re.compile(r"[<>=]\s*\(?\s*" + re.escape(cap) + r"\s*\)?\s*[;?)]")
    return bool(whole.search(line)) and bool(SIZES_A_GRID.search(line)) and not line.lstrip().startswith("//")


def grid_stride_kernels(texts):
    """{kernel: "file:line"} of every `gridDim.` of {file: text}, by the `__global__ ... void NAME(` that encloses it"""
    found = {}
    for name, text in texts.items():
        text = without_launch_bounds(text)
        heads = [(m.start(), m.group(1), m.group(2)) for m in HEAD.finditer(text)]
        for m in re.finditer(r"\bgridDim\.", text):
            where = f"{name}:{text.count(chr(10), 0, m.start()) + 1}"
            before = [(kind, k) for at, kind, k in heads if at < m.start()]
            assert before, f"{where}: gridDim. outside any device-side function"
            kind, kernel = before[-1]
            assert kind == "__global__", f"{where}: gridDim. inside the __device__ function {kernel}: the table is kept per kernel -- read it in the kernels that call it"
            found.setdefault(kernel, where)
    return found


def sources():
    return {os.path.basename(p): open(p).read() for p in SOURCES}


def table_problems(found, tables):
    """what test_every_grid_stride_kernel_is_in_exactly_one_table reports, as sentences that name the kernel"""
    out = []
    for kernel, where in sorted(found.items()):
        holders = [t for t, held in tables.items() if kernel in held]
        if not holders:
            out.append(f"{kernel} ({where}) walks a capped grid and is in none of CAPPED, PINNED_ELSEWHERE, OUT_OF_REACH of tests/grid_strides.py")
        if len(holders) > 1:
            out.append(f"{kernel} ({where}) is in {' and '.join(holders)}")
    for t, held in tables.items():
        out += [f"{t} names {kernel}, which no source has (or which no longer mentions gridDim)" for kernel in sorted(set(held) - set(found))]
    return out


def tables():
    return {"CAPPED": set(GS.CAPPED), "PINNED_ELSEWHERE": set(GS.PINNED_ELSEWHERE), "OUT_OF_REACH": set(GS.OUT_OF_REACH)}


def test_the_pattern_still_finds_the_kernels():
    text = ("template <typename T>\n__global__ __launch_bounds__(64) void a_kernel(const T* x, long F)\n{\n    for (long f = blockIdx.x; f < F; f += gridDim.x) {}\n}\n"
            "__global__ void b_kernel(float* y)\n{\n    y[blockIdx.x] = 0;\n}\n"
            "template <int N> __global__ void __launch_bounds__(256) c_kernel(float* y, long n)\n{\n    const long s = (long)gridDim.x * 256;\n    (void)gridDim.y;\n}\n")
    assert grid_stride_kernels({"f.hip": text}) == {"a_kernel": "f.hip:4", "c_kernel": "f.hip:12"}
    helper = text + "__device__ __forceinline__ long d_stride(int w)\n{\n    return (long)gridDim.x * w;\n}\n"   # not charged to c_kernel
    with pytest.raises(AssertionError, match="f.hip:17: gridDim. inside the __device__ function d_stride"):
        grid_stride_kernels({"f.hip": helper})
    assert len(grid_stride_kernels(sources())) >= 50


def test_every_grid_stride_kernel_is_in_exactly_one_table():
    problems = table_problems(grid_stride_kernels(sources()), tables())
    assert not problems, "\n".join(problems)
    assert len(GS.OUT_OF_REACH) <= 8 and all(isinstance(why, str) and "GiB" in why for why in GS.OUT_OF_REACH.values())


def test_a_missing_entry_a_new_kernel_and_a_double_entry_fail_by_name():
    found, t = grid_stride_kernels(sources()), tables()
    less = dict(t, CAPPED=t["CAPPED"] - {"excite_kernel"})
    assert table_problems(found, less) == [f"excite_kernel ({found['excite_kernel']}) walks a capped grid and is in none of CAPPED, PINNED_ELSEWHERE, "
                                           "OUT_OF_REACH of tests/grid_strides.py"]
    more = dict(found, **grid_stride_kernels({"new.hip": "__global__ void new_kernel(long n)\n{\n    for (long i = blockIdx.x; i < n; i += gridDim.x) {}\n}\n"}))
    assert table_problems(more, t) == ["new_kernel (new.hip:3) walks a capped grid and is in none of CAPPED, PINNED_ELSEWHERE, OUT_OF_REACH of tests/grid_strides.py"]
    twice = dict(t, OUT_OF_REACH=t["OUT_OF_REACH"] | {"excite_kernel"})
    assert table_problems(found, twice) == [f"excite_kernel ({found['excite_kernel']}) is in CAPPED and OUT_OF_REACH"]
    stale = dict(t, PINNED_ELSEWHERE=t["PINNED_ELSEWHERE"] | {"gone_kernel"})
    assert table_problems(found, stale) == ["PINNED_ELSEWHERE names gone_kernel, which no source has (or which no longer mentions gridDim)"]


def test_every_cap_is_spelled_where_a_grid_is_sized():
    texts = sources()
    for kernel, e in GS.CAPPED.items():
        lines = [ln for ln in texts[e["file"]].splitlines() if sizes_a_grid_with(e["cap"], ln)]
        assert lines, f"{kernel}: no line of csrc/{e['file']} sizes a grid with `{e['cap']}` (the entry is stale)"
        assert isinstance(e["trip"], int) and e["trip"] >= 1 and e["unit"] and e["cases"], kernel
        # the kernel is launched from that file, or from the header's kernels' own launcher file
        assert kernel in texts[e["file"]], f"{kernel} is not launched from csrc/{e['file']}"


def test_a_cap_is_matched_as_a_whole():
    assert sizes_a_grid_with("256", "    if (blocks > 256) blocks = 256;   // one persistent workgroup per CU")
    assert not sizes_a_grid_with("256", "    if (blocks > 256L * 32) blocks = 256L * 32;")
    assert not sizes_a_grid_with("256", "    long grid = F < 256L * 16 ? (long)F : 256L * 16;")
    assert not sizes_a_grid_with("256", "    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), 0, st);")
    assert not sizes_a_grid_with("256", "    // if (blocks > 256) blocks = 256;")
    assert sizes_a_grid_with("1 << 14", "        const dim3 grid((unsigned)(F < (1 << 14) ? F : (1 << 14)));")
    assert sizes_a_grid_with("1L << 20", "inline unsigned pq_blocks(long n) { return (unsigned)((n + 255) / 256 < (1L << 20) ? (n + 255) / 256 : (1L << 20)); }")
    assert sizes_a_grid_with("256L * 2 * 4", "            const long waves = 256L * 2 * 4;                 // two four-wave workgroups per CU")


def test_pinned_elsewhere_points_at_tests_that_exist():
    for kernel, e in GS.PINNED_ELSEWHERE.items():
        path, _, func = e["test"].partition("::")
        assert path.startswith("tests/") and os.path.exists(os.path.join(ROOT, path)), (kernel, e["test"])
        assert func.startswith("test_") and f"def {func}(" in open(os.path.join(ROOT, path)).read(), f"{e['test']} (for {kernel}) is not a test of {path}"
        assert e["rows"] and e["trips"] >= 2, kernel


def test_every_case_passes_its_cap_with_rows_that_differ():
    ids = []
    routes = {KR.case_id(route, c) for route, c in KR.all_cases()}
    for kernel, e in GS.CAPPED.items():
        for c in e["cases"]:
            ids += [GS.case_id(kernel, c) + "-" + dt for dt in c["dtypes"]]
            n = GS.rows_of_cap(e, c)
            assert c["when"] in ("fwd", "bwd") and c["dtypes"] and set(c["dtypes"]) <= {"f32", "f64"} and c["route"], (kernel, c)
            assert n % GS.PRIME != 0, f"{kernel}: the cap is {n} rows, a multiple of {GS.PRIME}: rows f and f + cap would be the same row"
            assert all(B > n for B in GS.batches(e, c)) and GS.batches(e, c)[0] == n + 3, (kernel, GS.batches(e, c), n)
            assert len(GS.batches(e, c)) == 1 or GS.batches(e, c)[1] == 2 * n + 1 > 2 * n
            if not c["promised"]:   # compared with two calls on slices: each half stays under the cap
                assert not c.get("third_trip") and GS.batches(e, c)[0] - GS.batches(e, c)[0] // 2 < n, kernel
            if c["family"] == "routes" and "spec" in c["shape"]:
                assert c["shape"]["spec"][0] in KR_CALLS and KR.MEAS not in getattr(KR, c["shape"]["spec"][1])["tol_from"], kernel
            elif c["family"] == "routes":
                assert c["shape"]["like"] in routes, f"{kernel}: tests/kernel_routes.py has no case {c['shape']['like']}"
            assert c.get("flag") in (None, "failed", "unstable") and c["promised"] in (True, False)
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    # every case carries its measured time, and none takes more than a few seconds
    assert set(GS.SECONDS) == set(ids), sorted(set(GS.SECONDS) ^ set(ids))
    assert max(GS.SECONDS.values()) <= 5.0
