"""Instruction census of reactor_kernel<54, false, false> in an ISA probe (scripts/isa_probe.sh).

    python scripts/isa_count.py [probe.s] [--blocks] [--min N]

Prints the kernel's totals per instruction class and, with --blocks, one line per basic block (label,
instruction count, class histogram, branch targets), so that the strip loops, the 54 pivot-step blocks of
the Gauss-Jordan factorisation and the solve block can be found and compared between two trees.  Classes
are told by generic opcode prefix only:

    f64     FP64 arithmetic (v_*_f64 other than conversions and compares)
    cvt     conversions (v_cvt_*)
    mov     moves, selects and compares (v_mov_*, v_cndmask_*, v_cmp*, v_accvgpr_*)
    lane    cross-lane reads (v_readlane / v_readfirstlane / v_writelane / v_permlane*, any *_dpp form)
    valu    every other v_* instruction
    ds      ds_*
    vmem    scratch_* / global_* / flat_* / buffer_*
    wait    s_waitcnt / s_nop
    salu    every other s_* instruction
"""
import collections
import re
import sys

CLASSES = ["f64", "cvt", "mov", "lane", "valu", "ds", "vmem", "wait", "salu", "other"]
KERNEL = r"^_ZN12_GLOBAL__N_114reactor_kernelILi54ELb0ELb0E.*:"


def classify(op: str) -> str:
    if op.startswith("v_"):
        if op.endswith("_dpp") or op.startswith(("v_readlane", "v_readfirstlane", "v_writelane", "v_permlane")):
            return "lane"
        if op.startswith("v_cvt_"):
            return "cvt"
        if op.startswith(("v_mov_", "v_cndmask_", "v_cmp", "v_accvgpr_")):
            return "mov"
        if re.search(r"_f64(_e32|_e64)?$", op):
            return "f64"
        return "valu"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("scratch_", "global_", "flat_", "buffer_")):
        return "vmem"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return "other"


def kernel_lines(lines):
    st = [i for i, l in enumerate(lines) if re.match(KERNEL, l)][0]
    en = [i for i in range(st, len(lines)) if "s_endpgm" in lines[i]][0]
    return lines[st:en + 1]


def blocks(body):
    """[(label, [(opcode, operands)])] in program order; the entry block carries the label 'entry'."""
    out = [("entry", [])]
    for l in body[1:]:
        s = l.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.LBB[0-9_]+):", s)
        if m:
            out.append((m.group(1), []))
            continue
        if s.startswith(".") or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        out[-1][1].append((parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else "/tmp/ckmi_probe.s"
    show_blocks = "--blocks" in sys.argv
    min_n = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 1
    bl = blocks(kernel_lines(open(path).read().split("\n")))
    total = collections.Counter()
    ops = collections.Counter()
    for label, ins in bl:
        c = collections.Counter(classify(op) for op, _ in ins)
        total.update(c)
        ops.update(op for op, _ in ins)
        if show_blocks and len(ins) >= min_n:
            tg = [a.strip() for op, a in ins if op.startswith(("s_cbranch", "s_branch"))]
            print(f"{label:12s} n={len(ins):5d} " + " ".join(f"{k}={c[k]}" for k in CLASSES if c[k]) +
                  (" -> " + ",".join(tg) if tg else ""))
    n = sum(total.values())
    print("classes " + " ".join(f"{k}={total[k]}" for k in CLASSES if total[k]) + f" total {n} blocks {len(bl)}")
    keys = ["v_mov_b32_e32", "ds_write_b64", "ds_write2_b64", "ds_write_b128", "ds_read_b128", "v_fmac_f64_e32", "v_fma_f64",
            "scratch_store_dword", "scratch_load_dword", "s_and_saveexec_b64", "v_readfirstlane_b32", "s_waitcnt"]
    print(" ".join(f"{k}={ops[k]}" for k in keys))


if __name__ == "__main__":
    main()
