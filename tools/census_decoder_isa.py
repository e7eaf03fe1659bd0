#!/usr/bin/env python
"""Static instruction census of the persistent decoder's step loop (csrc/taco_decoder_xcd.h) and of the post-net scan's (k_bigru_oct,
csrc/taco_bigru_xcd.h).  CPU only: compiles csrc/taco_lib.hip for
gfx950 with the flags of csrc/build.sh, keeps the device assembly, finds the step loop of k_decoder_xcd in the production instantiation
(<4, false, false, 256, 2, false>), the eight-rows-per-group one and the TAPE one, and prints how many instructions of each class one
pass over the loop body holds (inner loops -- poll retries, the score and context loops -- are counted once, as they stand in the text).
The kernel carries the body twice, once per exchange protocol (XCD-local / write-through): both loops are listed.
--scan: the same for k_bigru_oct<4> (production, TAPE) and <2>, <1>.

Second view, for the XCD-local loop of every kernel listed: the instructions between each barrier (or the top of the loop) and the next
exchange store (global_store_dwordx2) in the text -- what a wave issues before its value leaves, which lengthens the exchange chain one for
one -- and between that store and the next barrier.  A stretch with no exchange store is listed as such.

    python tools/census_decoder_isa.py [--scan] [--asm FILE.s] [--keep FILE.s] [-D...]       # --asm: read an assembly file instead of compiling

What the table is for: the step is VALU-issue bound on its second waves, so a cut is worth a GPU visit only if the VALU total
of the production loop falls here first."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-speaker-tacotron-tensorflow_amd", "csrc")
KERNELS = [("production  <4, false, false, 256, 2, false>", "_Z13k_decoder_xcdILi4ELb0ELb0ELi256ELi2ELb0EEv6DxArgs"),
           ("RG = 8      <8, false, false, 256, 2, false>", "_Z13k_decoder_xcdILi8ELb0ELb0ELi256ELi2ELb0EEv6DxArgs"),
           ("TAPE        <4, true, false, 256, 2, false>", "_Z13k_decoder_xcdILi4ELb1ELb0ELi256ELi2ELb0EEv6DxArgs")]
SCAN_KERNELS = [("production  <4, false, false>", "_Z11k_bigru_octILi4ELb0ELb0EEv6GdArgs"),
                ("TAPE        <4, true, false>", "_Z11k_bigru_octILi4ELb1ELb0EEv6GdArgs"),
                ("16 rows     <2, false, false>", "_Z11k_bigru_octILi2ELb0ELb0EEv6GdArgs"),
                ("8 rows      <1, false, false>", "_Z11k_bigru_octILi1ELb0ELb0EEv6GdArgs")]
CLASSES = ["packed FMA", "scalar FMA", "other float VALU", "cross-lane (DPP, permlane, readlane)", "transcendental", "compare / select / move",
           "address and integer VALU", "VALU total", "LDS", "vector memory", "scalar ALU / control", "s_waitcnt", "s_barrier", "s_sleep / s_nop",
           "all instructions"]
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
FLOAT = ("v_add_f", "v_sub_f", "v_subrev_f", "v_mul_f", "v_max_f", "v_min_f", "v_pk_add_f", "v_pk_mul_f", "v_med3_f", "v_max3_f", "v_min3_f",
         "v_cvt_", "v_ldexp_f", "v_frexp_", "v_fract_", "v_floor_", "v_ceil_", "v_rndne_", "v_trunc_", "v_mul_legacy", "v_div_")


def compile_asm(out, defines):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"] + defines + ["-o", out, "taco_lib.hip"]
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)


def functions(path, stem="_Z13k_decoder_xcd"):
    """mangled name -> (instruction lines with their labels, trailer comments) for every kernel in the file whose mangled name starts with `stem`"""
    out, name, body = {}, None, None
    for line in open(path, errors="replace"):
        s = line.strip()
        m = re.match(r"^(%s\w+):" % stem, s)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(s)
        if s.startswith(".Lfunc_end"):
            out[name] = [body, []]
            last, name = name, None
            continue
    # the resource comments follow .Lfunc_end; read them in a second pass
    cur = None
    for line in open(path, errors="replace"):
        s = line.strip()
        m = re.match(r"^; Kernel info:|^; -- End function", s)
        m2 = re.match(r"^(%s\w+):" % stem, s)
        if m2:
            cur = m2.group(1)
        elif cur in out and s.startswith(";") and re.search(r"(NumVgprs|NumAgprs|ScratchSize|TotalNumSgprs|Occupancy|LDSByteSize|codeLenInByte)", s):
            out[cur][1].append(s.lstrip("; "))
        elif s.startswith(".text") or s.startswith(".section"):
            cur = None if (cur and out.get(cur, [None, []])[1]) else cur
    return out


def classify(ins):
    op = ins.split()[0]
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_barrier":
        return "s_barrier"
    if op in ("s_sleep", "s_nop"):
        return "s_sleep / s_nop"
    if op.startswith("s_"):
        return "scalar ALU / control"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vector memory"
    if not op.startswith("v_"):
        return "scalar ALU / control"
    if "dpp" in op or re.search(r"\b(quad_perm|row_shl|row_shr|row_ror|row_mirror|row_half_mirror|row_bcast|row_newbcast|wave_shl|wave_shr)", ins) \
            or op.startswith(("v_permlane", "v_readlane", "v_readfirstlane", "v_writelane")):
        return "cross-lane (DPP, permlane, readlane)"
    if op.startswith("v_pk_fma"):
        return "packed FMA"
    if op.startswith(("v_fma_f", "v_fmac_f", "v_mac_f", "v_mad_f", "v_fma_mix", "v_fmaak", "v_fmamk")):
        return "scalar FMA"
    if op.startswith(TRANS):
        return "transcendental"
    if op.startswith(("v_cmp", "v_cndmask", "v_mov_", "v_accvgpr", "v_swap", "v_pk_mov")):
        return "compare / select / move"
    if op.startswith(FLOAT):
        return "other float VALU"
    return "address and integer VALU"


def loops(body):
    """outermost loops of a function: (first line, last line) of every backward branch whose span no other one contains"""
    label = {}
    for i, s in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            label[m.group(1)] = i
    spans = []
    for i, s in enumerate(body):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\w+)", s)
        if m and label.get(m.group(1), i + 1) < i:
            spans.append((label[m.group(1)], i))
    outer = [sp for sp in spans if not any(o != sp and o[0] <= sp[0] and sp[1] <= o[1] for o in spans)]
    return sorted(set(outer))


def census(body, span):
    c = dict.fromkeys(CLASSES, 0)
    for s in body[span[0]:span[1] + 1]:
        s = s.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        k = classify(s)
        c[k] += 1
        c["all instructions"] += 1
        if s.startswith("v_"):
            c["VALU total"] += 1
    return c


def protocol(body, span):
    st = [s for s in body[span[0]:span[1] + 1] if s.startswith("global_store_dwordx2")]
    return "write-through" if st and all(" sc1" in s for s in st) else "XCD-local"


def instructions(body, span):
    for s in body[span[0]:span[1] + 1]:
        s = s.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            yield s


def stretches(body, span):
    """[(from, to, census)] over the loop text: barrier (or loop top) -> next exchange store, exchange store -> next barrier (or loop end)"""
    out, c, start, stores = [], dict.fromkeys(CLASSES, 0), "loop top", 0

    def close(end):
        nonlocal c
        out.append((start, end, c))
        c = dict.fromkeys(CLASSES, 0)

    for s in instructions(body, span):
        op = s.split()[0]
        if op == "s_barrier":
            close("barrier")
            start, stores = "barrier", 0
            continue
        c[classify(s)] += 1
        c["all instructions"] += 1
        if s.startswith("v_"):
            c["VALU total"] += 1
        if op == "global_store_dwordx2" and stores == 0:       # the first exchange store of the stretch: the value leaves here
            close("exchange store")
            start, stores = "exchange store", 1
    close("loop end")
    return out


def print_stretches(body, span):
    cols = ["VALU total", "packed FMA", "scalar FMA", "cross-lane (DPP, permlane, readlane)", "transcendental", "LDS", "vector memory", "s_waitcnt", "all instructions"]
    head = ["VALU", "pk FMA", "FMA", "x-lane", "trans", "LDS", "vmem", "waitcnt", "all"]
    print("  between barriers and exchange stores (XCD-local loop, text order)")
    print("  %3s %-16s %-16s" % ("#", "from", "to") + "".join("%8s" % h for h in head))
    for i, (a, b, c) in enumerate(stretches(body, span)):
        print("  %3d %-16s %-16s" % (i, a, b) + "".join("%8d" % c[k] for k in cols))


def main():
    args = sys.argv[1:]
    scan = "--scan" in args
    asm = args[args.index("--asm") + 1] if "--asm" in args else None
    keep = args[args.index("--keep") + 1] if "--keep" in args else None
    defines = [a for a in args if a.startswith("-D")]
    tmp = None
    if asm is None:
        tmp = keep or tempfile.mkstemp(suffix=".s")[1]
        compile_asm(os.path.abspath(tmp), defines)
        asm = tmp
    fns = functions(asm, "_Z11k_bigru_octI" if scan else "_Z13k_decoder_xcd")
    print("%s step loop, static instructions per loop body (gfx950%s)" % ("k_bigru_oct" if scan else "k_decoder_xcd", "; " + " ".join(defines) if defines else ""))
    for title, mangled in (SCAN_KERNELS if scan else KERNELS):
        if mangled not in fns:
            sys.exit("kernel %s not found in %s" % (mangled, asm))
        body, res = fns[mangled]
        big = sorted(loops(body), key=lambda sp: sp[0] - sp[1])[:2]      # the step loop of each protocol: the two largest outermost loops
        cols = [(protocol(body, sp), census(body, sp), sp) for sp in sorted(big)]
        cols.sort(key=lambda pc: pc[0])      # XCD-local (what a whole MI355X runs) first
        print("\n%s" % title)
        print("  " + "; ".join(res))
        print("  %-40s" % "class" + "".join("%16s" % p for p, _, _ in cols))
        for k in CLASSES:
            print("  %-40s" % k + "".join("%16d" % c[k] for _, c, _ in cols))
        print_stretches(body, cols[0][2])
    if tmp and not keep:
        os.remove(tmp)


if __name__ == "__main__":
    main()
