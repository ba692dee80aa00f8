#!/usr/bin/env python3
"""Per-kernel device-code comparison of one HIP source between two trees, without a GPU: both copies are compiled for
gfx950 with the Makefile's flags and `--cuda-device-only -S`, the assembly is cut per kernel symbol, assembler comments,
the __hip_cuid symbol and the function ordinal of local labels are dropped, and the instruction text is compared.  For
kernels whose text differs, the counts of the arithmetic and memory opcodes a refactor must not move are printed side by side,
and the ordered list of the s_waitcnt vmcnt(N) operands: the packed row kernels' speed rests on where the compiler lets a wave
wait for how many loads, which a count per N does not show.
A packed arithmetic instruction (v_pk_add_f32 ...) counts as the two scalar ones it stands for, and LDS traffic is counted in
BYTES per lane and direction, not in instructions: the compiler pairs two ds_read_b32 into one
ds_read2st64_b32 (and back) as the addressing around them changes -- the same bytes.
usage: python scripts/kernel_asm_diff.py <parent csrc dir> <head csrc dir> matvec.hip [attention.hip ...]"""
import collections, concurrent.futures, os, re, subprocess, sys

FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
GROUPS = [("v_fma*", r"v_(pk_)?fma"), ("v_mul_f32", r"v_(pk_)?mul_f32"), ("v_add_f32", r"v_(pk_)?add_f32"), ("v_exp*", r"v_exp"),
          ("v_rcp* / v_div*", r"v_(rcp|div_)"), ("global_load*", r"global_load"), ("global_store* / atomic", r"global_(store|atomic)"),
          ("v_mfma*", r"v_mfma"), ("s_barrier", r"s_barrier")]
LDS_OP = re.compile(r"ds_(read|load|write|store)(2|2st64)?_(?:[a-z]*?)(\d+)")   # ds_read_b128, ds_write2st64_b32, ds_read_u16_d16 ...


def kernels(csrc, src):
    asm = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", src, "-o", "-"],
                         cwd=csrc, capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if "__hip_cuid" in s:
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def counts(text):
    c = collections.OrderedDict((g, 0) for g, _ in GROUPS)
    c["LDS bytes read"] = c["LDS bytes written"] = 0
    for s in text:
        op = s.split()[0]
        for g, pat in GROUPS:
            if re.match(pat, op):
                c[g] += 2 if op.startswith("v_pk_") else 1   # (a packed instruction is two of the scalar one: the same operations)
        m = LDS_OP.match(op)
        if m:   # bytes per lane: the element width, twice for the two-address forms
            c["LDS bytes read" if m.group(1) in ("read", "load") else "LDS bytes written"] += int(m.group(3)) // 8 * (2 if m.group(2) else 1)
    return c


def vmcnts(text):
    """the N of every s_waitcnt vmcnt(N), in program order"""
    return [int(m.group(1)) for s in text if s.startswith("s_waitcnt") for m in [re.search(r"vmcnt\((\d+)\)", s)] if m]


if __name__ == "__main__":
    parent, head = sys.argv[1], sys.argv[2]
    for src in sys.argv[3:]:
        with concurrent.futures.ThreadPoolExecutor(2) as ex:   # (the two compiles side by side)
            a, b = ex.map(lambda d: kernels(d, src), (parent, head))
        differ = [k for k in a if k in b and a[k] != b[k]]
        moved_in = [k for k in differ if counts(a[k]) != counts(b[k])]
        print(f"{src}: kernels parent {len(a)} head {len(b)}; only in parent {sorted(set(a) - set(b))}; only in head {sorted(set(b) - set(a))}; "
              f"instruction text differs in {len(differ)}; a count differs in {len(moved_in)}")
        dem = subprocess.run(["c++filt"], input="\n".join(differ), capture_output=True, text=True).stdout.splitlines()
        for k, d in zip(differ, dem):
            d = re.sub(r"l2z::\(anonymous namespace\)::", "", d)
            d = re.sub(r"\(.*", "", d).replace("void ", "")
            ca, cb = counts(a[k]), counts(b[k])
            moved = ", ".join(f"{g} {ca[g]} -> {cb[g]} (!)" for g in ca if ca[g] != cb[g])
            print(f"  {d}: instructions {len([s for s in a[k] if not s.endswith(':')])} -> {len([s for s in b[k] if not s.endswith(':')])}; "
                  + (moved or "counts equal: " + ", ".join(f"{g} {ca[g]}" for g in ca)))
            va, vb = vmcnts(a[k]), vmcnts(b[k])
            print(f"    vmcnt order {'equal' if va == vb else 'DIFFERS (!)'}: {' '.join(map(str, va))}" + ("" if va == vb else f" -> {' '.join(map(str, vb))}"))
