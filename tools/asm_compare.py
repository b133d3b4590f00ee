#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two trees, kernel instance by kernel instance (no GPU needed).

    python tools/asm_compare.py PARENT_CSRC RESULT_CSRC gemm_bf16.hip band_ffn.hip [--experiments] [--flags "-mllvm ..."]

Each named translation unit is compiled from both csrc directories with the build's flags (versband_amd/build.py) plus
--cuda-device-only -S.  Per kernel symbol: the opcode sequence with operands ignored, split at the first and the last MFMA of the kernel
(prologue | first..last MFMA | epilogue); where that middle part differs, whether its LDS accesses, DMAs / global accesses, s_waitcnt, barriers
and MFMAs - with their operands, so wait counts and offsets included; register numbers masked - still come in the parent's order; and the resource figures of the code object's metadata (VGPR, AGPR, SGPR, LDS, scratch,
spills).  This is how profiles/r07_ring_window_asm.txt, r09_conv_staged_asm.txt and r10_gemm_tile_asm.txt were made.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count",
             ".sgpr_spill_count")


def compile_asm(csrc, unit, extra, out):
    pre = os.path.join(csrc, unit.replace(".hip", ".s"))      # (a directory may hold assembly made earlier with the same flags instead)
    if os.path.exists(pre):
        return open(pre).read()
    include = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    cmd = [HIPCC, *FLAGS, *extra, "-I", include, "--cuda-device-only", "-S", os.path.join(csrc, unit), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"hipcc failed for {csrc}/{unit}:\n{r.stderr}")
    return open(out).read()


def kernels(text, full=False):
    """symbol -> list of opcodes, for every function of the assembly"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith((".L", "BB")):
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        s = line.strip()
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        cur.append(s.split(";")[0].strip() if full else s.split()[0])
    return {k: v for k, v in out.items() if v}


ORDERED = ("ds_", "global_", "buffer_", "scratch_", "flat_", "s_waitcnt", "s_barrier", "v_mfma", "s_sleep", "s_setprio", "s_sched")


def ordered(lines):
    """the hazard-carrying subsequence between first and last MFMA: memory operations, waits, barriers, MFMAs, registers masked"""
    idx = [i for i, l in enumerate(lines) if l.startswith("v_mfma")]
    if not idx:
        return []
    return [re.sub(r"\b[vsa]\[?\d+(:\d+)?\]?", "R", l) for l in lines[idx[0]:idx[-1] + 1] if l.startswith(ORDERED)]


def resources(text):
    """symbol -> {resource: value} from the amdhsa metadata"""
    out, name, cur = {}, None, {}
    for line in text.splitlines():
        s = line.strip()
        m = re.match(r"-?\s*(\.[a-z_]+):\s*(\S+)$", s)
        if not m:
            continue
        if s.startswith("- ") and cur:
            if name:
                out[name] = cur
            name, cur = None, {}
        if m.group(1) == ".name":
            name = m.group(2)
        elif m.group(1) in RESOURCES:
            cur[m.group(1)] = m.group(2)
    if name:
        out[name] = cur
    return out


def split(ops):
    idx = [i for i, o in enumerate(ops) if o.startswith("v_mfma")]
    if not idx:
        return ops, [], []
    return ops[:idx[0]], ops[idx[0]:idx[-1] + 1], ops[idx[-1] + 1:]


def delta(a, b):
    ca, cb = collections.Counter(a), collections.Counter(b)
    return {k: cb[k] - ca[k] for k in sorted(set(ca) | set(cb)) if cb[k] != ca[k]}


def part(name, a, b):
    if a == b:
        return f"{name} {len(a)} identical"
    d = delta(a, b)
    return f"{name} {len(a)} -> {len(b)} " + (str(d) if d else "(same opcode counts, other order)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("result")
    ap.add_argument("units", nargs="+")
    ap.add_argument("--experiments", action="store_true")
    ap.add_argument("--flags", default="")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="replace OLD by NEW in the parent's symbols (a kernel whose argument type was renamed)")
    a = ap.parse_args()
    extra = (["-DVB_EXPERIMENTS"] if a.experiments else []) + a.flags.split()
    print("## " + ("VB_BUILD_EXPERIMENTS=1 build" if a.experiments else "product build"))
    differing, res_diff, reordered = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for unit in a.units:
            tp = compile_asm(a.parent, unit, extra, os.path.join(tmp, "p.s"))
            for r in a.rename:
                tp = tp.replace(*r.split("=", 1))
            tr = compile_asm(a.result, unit, extra, os.path.join(tmp, "r.s"))
            kp, kr, rp, rr = kernels(tp), kernels(tr), resources(tp), resources(tr)
            fp, fr = kernels(tp, True), kernels(tr, True)
            print(f"# {unit}: kernel symbols parent {len(rp)}, result {len(rr)}, only parent {sorted(set(rp) - set(rr))}, only result {sorted(set(rr) - set(rp))}")
            for sym in sorted(set(rp) & set(rr)):
                p0, p1, p2 = split(kp.get(sym, []))
                r0, r1, r2 = split(kr.get(sym, []))
                mid = "first..last MFMA: opcode sequence IDENTICAL" if p1 == r1 else "first..last MFMA: " + part("DIFFERS", p1, r1)
                if p1 != r1:
                    op, orr = ordered(fp.get(sym, [])), ordered(fr.get(sym, []))
                    same = op == orr
                    mid += f" [memory / wait / barrier / MFMA subsequence, {len(op)} instructions with operands: " + ("the parent's order" if same else "DIFFERS") + "]"
                    if not same:
                        reordered.append(sym)
                print(f"{sym} | total {len(kp.get(sym, []))} -> {len(kr.get(sym, []))} | {part('prologue', p0, r0)} | {mid} | {part('after last MFMA:', p2, r2)}")
                if p1 != r1:
                    differing.append(sym)
                d = {k: (rp[sym].get(k), rr[sym].get(k)) for k in RESOURCES if rp[sym].get(k) != rr[sym].get(k)}
                if d:
                    res_diff.append((sym, d))
    print("resource differences (parent, result):" + ("" if res_diff else " none"))
    for sym, d in res_diff:
        print("  ", sym, d)
    print("instances whose MFMA region differs:", differing)
    print("... of which the memory / wait / barrier / MFMA subsequence differs from the parent's:", reordered)


if __name__ == "__main__":
    main()
