#!/usr/bin/env python3
"""Instruction mix of a kernel's innermost loop, read off the shipped code object, priced with the measured issue costs of
profiles/r03_issue_calibration.txt (cycles a wave64 instruction occupies the float32 datapath of its SIMD: multiply-add class /
DPP / conversions / packed 4, two-operand and move class 2, transcendentals 8, v_mfma_f32_4x4x1 8, v_mfma_f32_16x16x4_f32 32;
binary16 matrix products run on the separate matrix pipe: 16 cycles each, listed beside).

    python tools/isa_mix.py [diffsptk_amd/lib/libdiffsptk_amd.so] [kernel-name-substring ...]      -> JSON per kernel
    python tools/isa_mix.py --diff parent.so branch.so      -> per-kernel comparison of two builds (diff_libs), exit status 1 if it fails

The loop taken is the LAST innermost loop of the kernel (for the mel-cepstral kernels: the Newton step; one pass = 16 frames).  Where
that loop holds an if / else whose two arms both contain binary16 matrix products -- the coarse and the full chain phase of the
tuned forward -- the arms and the rest of the step are listed separately: a pass runs one arm, not both."""
import collections
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
TWO = {"v_mov_b32", "v_add_f32", "v_mul_f32", "v_and_b32", "v_or_b32", "v_add_u32", "v_sub_f32", "v_sub_u32", "v_lshlrev_b32",
       "v_lshrrev_b32", "v_xor_b32", "v_subrev_f32", "v_subrev_u32", "v_max_f32", "v_min_f32", "v_cndmask_b32", "v_accvgpr_write_b32",
       "v_accvgpr_read_b32", "v_mov_b64"}
EIGHT = {"v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_rcp_f32_dpp"}


def disassemble(lib):
    """{kernel symbol: [(address, mnemonic, text)]} of the gfx950 code objects bundled in `lib` (the .hip_fatbin section holds
    one clang offload bundle per translation unit: header magic, entry table (offset, size, triple), code objects).
    A symbol defined in two code objects of the library raises ValueError: the second would replace the first here."""
    import struct

    tmp = "/tmp/isa_mix_%d" % os.getpid()
    os.makedirs(tmp, exist_ok=True)
    fat = os.path.join(tmp, "fat.bin")
    # llvm-objcopy without an output operand REWRITES its input: work on a private copy and send the output to a scratch file,
    # the product library is only ever read (tests/test_host_cpu.py checks its bytes before / after)
    import shutil

    priv = os.path.join(tmp, "lib_copy.so")
    shutil.copyfile(lib, priv)
    subprocess.run([OBJDUMP.replace("objdump", "objcopy"), "--dump-section", ".hip_fatbin=" + fat, priv, os.path.join(tmp, "lib_out.so")],
                   check=True)
    for f_ in (priv, os.path.join(tmp, "lib_out.so")):
        if os.path.exists(f_):
            os.remove(f_)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    kernels, pos, n = {}, 0, 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            break
        nb = struct.unpack_from("<Q", data, i + 24)[0]
        off = i + 32
        for _ in range(nb):
            o, sz, tl = struct.unpack_from("<QQQ", data, off)
            off += 24
            triple = data[off: off + tl].decode()
            off += tl
            if "gfx950" in triple and sz:
                co = os.path.join(tmp, "co%d.o" % n)
                n += 1
                open(co, "wb").write(data[i + o: i + o + sz])
                txt = subprocess.run([OBJDUMP, "-d", co], capture_output=True, text=True).stdout
                cur = None
                for line in txt.splitlines():
                    m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                    if m:
                        cur = m.group(1)
                        if cur in kernels:
                            raise ValueError("%s: %s is defined in two code objects" % (lib, cur))
                        kernels[cur] = []
                        continue
                    m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
                    if m and cur:
                        kernels[cur].append((int(m.group(3), 16), m.group(1), m.group(2)))
                os.remove(co)
        pos = i + 24
    os.remove(fat)
    return kernels


def crossed_packed_f32(kernels):
    """{kernel: [instruction text]} of every packed float32 instruction with a SET op_sel bit -- a LOW result half that reads a
    HIGH source half -- in `kernels` (the output of disassemble()).  That is the instruction class of every transient wrong
    result DESIGN.md 4 recorded; the product must contain none (tests/test_host_cpu.py::test_no_crossed_packed_float32).
    `python tools/isa_mix.py --audit [lib.so]` prints the per-kernel counts."""
    bad = {}
    for name, ins in kernels.items():
        for _, op, txt in ins:
            if re.match(r"v_pk_\w+_f32", op):
                m = re.search(r"op_sel:\[([01,]+)\]", txt)
                if m and "1" in m.group(1):
                    bad.setdefault(name, []).append(op + " " + txt)
    return bad


# scalar integer ALU: address and loop set-up, which the compiler derives anew from the set of callers a translation unit holds
SALU_INT = re.compile(r"s_(add|addc|sub|subb|mul|mul_hi|lshl|lshr|ashr|lshl[1-4]_add|and|or|xor|andn2|orn2|not|mov|movk|cmov|cmp|cmpk|cselect|"
                      r"bfe|bfm|min|max|sext|abs)_\w*[iub](16|32|64)$")
TUNED = re.compile(r"stft512_|stft_big_|zerodf_\w*_rows|mcep_|mgcep_|thsolve_quad|lpc24")   # the kernels that must stay identical: classes (b) / (c)


def _views(ins):
    """The three views of a kernel that diff_libs compares: as is; with the literal of pc-relative address formation (the s_add_u32 /
    s_addc_u32 pair behind s_getpc_b64) masked; and with, further, every scalar integer ALU instruction that touches neither exec nor
    vcc dropped and every SGPR operand replaced by a placeholder that keeps its width.  The s_nop run behind a final s_endpgm is
    left out of all three: it is the padding of the code object's text section, which falls to whichever kernel is linked last.
    (Likewise behind a final s_branch or s_setpc_b64 -- a kernel whose last block loops back, a noinline device function's
    return: nothing falls through an unconditional transfer into the run.)"""
    end = len(ins)
    while end and ins[end - 1][1] == "s_nop":
        end -= 1
    if end and ins[end - 1][1] in ("s_endpgm", "s_branch", "s_setpc_b64"):
        ins = ins[:end]
    plain = [op + " " + txt for _, op, txt in ins]
    masked, since_getpc = [], 9
    for _, op, txt in ins:
        since_getpc = 0 if op == "s_getpc_b64" else since_getpc + 1
        if since_getpc in (1, 2) and op in ("s_add_u32", "s_addc_u32"):
            txt = re.sub(r"(0x[0-9a-f]+|\d+)$", "<pcrel>", txt)
        masked.append((op, txt))
    loose = []
    for op, txt in masked:
        if SALU_INT.match(op) and not re.search(r"\b(exec|vcc)", txt):
            continue
        loose.append(op + " " + re.sub(r"\bs\[(\d+):(\d+)\]", lambda m: "s[x%d]" % (int(m.group(2)) - int(m.group(1)) + 1),
                                       re.sub(r"\bs\d+\b", "s", txt)))
    return plain, [op + " " + txt for op, txt in masked], loose


def diff_libs(parent, branch):
    """(report text, passed) of two builds of the library, per kernel symbol: (a) both hold the same symbols, each once;
    (b) identical; (c) identical but for the literal of pc-relative addresses; (d) identical, at an equal instruction count, but for
    scalar integer ALU instructions and SGPR numbering; (e) anything else.  Passes when (a) holds, nothing is in (e) and every
    tuned kernel (TUNED) is in (b) or (c)."""
    import difflib

    try:
        kp, kb = disassemble(parent), disassemble(branch)
    except ValueError as e:
        return "(a) FAILS: %s\n" % e, False
    out, cls = [], {}
    only = sorted(set(kp) ^ set(kb))
    for name in sorted(set(kp) & set(kb)):
        vp, vb = _views(kp[name]), _views(kb[name])
        cls[name] = "b" if vp[0] == vb[0] else "c" if vp[1] == vb[1] else "d" if vp[2] == vb[2] and len(vp[0]) == len(vb[0]) else "e"
    bad_tuned = [n for n, c in cls.items() if c in "de" and TUNED.search(n)]
    passed = not only and "e" not in cls.values() and not bad_tuned
    out.append("parent %s: %d symbols, %d instructions; branch %s: %d symbols, %d instructions" % (
        os.path.basename(parent), len(kp), sum(map(len, kp.values())), os.path.basename(branch), len(kb), sum(map(len, kb.values()))))
    out.append("(a) same symbols, each in one code object: %s" % ("yes" if not only else "NO, in one build only: " + ", ".join(only)))
    for c, what in (("b", "identical"), ("c", "identical but for pc-relative literals"),
                    ("d", "identical but for scalar integer ALU and SGPR numbering"), ("e", "different")):
        names = [n for n in cls if cls[n] == c]
        out.append("(%s) %-56s %4d kernels, %d of them tuned (%s)" % (c, what, len(names), sum(1 for n in names if TUNED.search(n)), TUNED.pattern))
    out.append("result: %s" % ("PASS" if passed else "FAIL"))
    for c in "cde":
        for n in (n for n in cls if cls[n] == c):
            out.append("\n(%s) %s  [%d instructions]" % (c, n, len(kb[n])))
            if c != "c":
                out.extend(difflib.unified_diff(_views(kp[n])[1], _views(kb[n])[1], "parent", "branch", lineterm="", n=1))
    return "\n".join(out) + "\n", passed


def innermost_last_loop(ins):
    """(start, end) indices of the last backward branch's span that contains no other backward branch target span."""
    addr = {a: i for i, (a, _, _) in enumerate(ins)}
    loops = []
    for i, (a, op, txt) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            try:
                simm = int(txt.split()[0], 0)
            except (ValueError, IndexError):
                continue
            if simm >= 0x8000:
                simm -= 0x10000
            t = a + 4 + 4 * simm   # branch target = address of the next instruction + 4 * simm16
            if t in addr and addr[t] < i:
                loops.append((addr[t], i))
    inner = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
    return max(inner, key=lambda l: l[1] - l[0]) if inner else None


def _target(a, txt):
    simm = int(txt.split()[0], 0)
    return a + 4 + 4 * (simm - 0x10000 if simm >= 0x8000 else simm)


def chain_arms(ins, lp):
    """The two arms of the if / else inside the loop `lp` that both hold binary16 matrix products (round 11: the chain phase of a
    coarse and of a full Newton step): ((start, end), (start, end)) index spans in layout order, or None.  An arm is the span a
    forward conditional branch of the loop skips; taken are the spans with such products that contain no other such span, and
    there must be exactly two (the compiler lays the else arm out behind a second test of the condition, not behind an s_branch)."""
    addr = {a: i for i, (a, _, _) in enumerate(ins)}
    spans = []
    for h in range(lp[0], lp[1]):
        a, op, txt = ins[h]
        t = addr.get(_target(a, txt), -1) if op.startswith("s_cbranch") else -1
        if h < t <= lp[1] + 1 and any(op_.startswith("v_mfma") and "f16" in op_ for _, op_, _ in ins[h + 1: t]):
            spans.append((h + 1, t - 1))
    inner = [s_ for s_ in spans if not any(o != s_ and s_[0] <= o[0] and o[1] <= s_[1] for o in spans)]
    return tuple(sorted(inner)) if len(inner) == 2 else None


def _summary(part):
    c, cyc = mix(part)
    vec = c["valu_multiply_add_class"] + c["valu_two_operand"] + c["valu_transcendental"]
    return {"instructions": len(part), "counts": dict(c), "f32_datapath_cycles": sum(cyc.values()), "vector_instructions": vec,
            "xdl_cycles": 16 * c["mfma_f16_xdl"], "v_fma_mix": sum(1 for _, op, _ in part if op.startswith("v_fma_mix")),
            "lds_reads_16_bytes": sum(1 for _, op, _ in part if op == "ds_read_b128")}


def mix(ins):
    c, cyc = collections.Counter(), collections.Counter()
    for _, op, txt in ins:
        base = re.sub(r"_e32$|_e64$|_dpp$|_sdwa$", "", op)
        if op.startswith("v_mfma_f32_4x4x1"):
            k, cy = "mfma_f32_4x4x1", 8
        elif op.startswith("v_mfma_f32_16x16x4"):
            k, cy = "mfma_f32_16x16x4", 32
        elif op.startswith("v_mfma"):
            k, cy = "mfma_f16_xdl", 0
        elif op.startswith("v_"):
            if base in EIGHT or op in EIGHT:
                k, cy = "valu_transcendental", 8
            elif base in TWO and not op.endswith("_dpp"):
                k, cy = "valu_two_operand", 2
            else:
                k, cy = "valu_multiply_add_class", 4
        elif op.startswith("ds_"):
            k, cy = "lds", 0
        elif op == "s_nop":
            k, cy = "s_nop", 0
        elif op.startswith("s_"):
            k, cy = "salu", 0
        else:
            k, cy = "vmem", 0
        c[k] += 1
        cyc[k] += cy
    return c, cyc


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].endswith(".so") else os.path.join(ROOT, "diffsptk_amd", "lib", "libdiffsptk_amd.so")
    names = [a for a in sys.argv[1:] if not a.endswith(".so")] or ["mcep_mfma_fwd_kernel_h", "mcep_mfma_bwd_kernel_h"]
    ks = disassemble(lib)
    res = {}
    for sym, ins in ks.items():
        if not any(n in sym for n in names) or not ins:
            continue
        lp = innermost_last_loop(ins)
        if lp is None:
            continue
        c, cyc = mix(ins[lp[0]: lp[1] + 1])
        vec = c["valu_multiply_add_class"] + c["valu_two_operand"] + c["valu_transcendental"]
        res[sym] = {"loop_instructions": lp[1] - lp[0] + 1, "counts": dict(c), "f32_datapath_cycles_per_pass": sum(cyc.values()),
                    "vector_instructions_per_pass": vec, "matrix_f32_instructions_per_pass": c["mfma_f32_4x4x1"] + c["mfma_f32_16x16x4"],
                    "xdl_cycles_per_pass": 16 * c["mfma_f16_xdl"], "frames_per_pass": 16}
        arms = chain_arms(ins, lp)
        if arms:   # the loop holds BOTH variants of the chain phase; a pass runs one of them
            parts = sorted((_summary(ins[s0: s1 + 1]) for s0, s1 in arms), key=lambda d: d["xdl_cycles"])
            res[sym]["chain_phase_coarse"], res[sym]["chain_phase_full"] = parts
            res[sym]["rest_of_the_step"] = _summary(ins[lp[0]: arms[0][0]] + ins[arms[1][1] + 1: lp[1] + 1])
    print(json.dumps(res, indent=1))


if __name__ == "__main__" and "--diff" in sys.argv:
    libs = [a for a in sys.argv[1:] if a != "--diff"]
    report, ok = diff_libs(*libs)
    sys.stdout.write(report)
    sys.exit(0 if ok else 1)
elif __name__ == "__main__" and "--audit" in sys.argv:
    args = [a for a in sys.argv[1:] if a != "--audit"]
    ks = disassemble(args[0] if args else os.path.join(ROOT, "diffsptk_amd", "lib", "libdiffsptk_amd.so"))
    bad = crossed_packed_f32(ks)
    npk = sum(1 for ins in ks.values() for _, op, _t in ins if re.match(r"v_pk_\w+_f32", op))
    for k_, v_ in sorted(bad.items()):
        print("%5d  %s" % (len(v_), k_))
    print("%d kernels, %d packed float32 instructions, %d with a set op_sel bit in %d kernels" % (len(ks), npk, sum(map(len, bad.values())), len(bad)))
    sys.exit(1 if bad else 0)
elif __name__ == "__main__":
    main()
