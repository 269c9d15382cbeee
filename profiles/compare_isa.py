"""Compare the instruction streams of the kernels of two builds of libvecsim (no GPU needed).

    python profiles/compare_isa.py OLD_OBJ_DIR NEW_OBJ_DIR [REGEX]

OLD_OBJ_DIR / NEW_OBJ_DIR are the `build/` object directories of two in-tree builds (simurlacra_amd/csrc/build), e.g. one of
the parent commit and one of the working tree.  Every kernel whose name matches REGEX (default: every kernel) must exist in
both builds with the same instructions: a kernel of the old build that the new one lacks is MISSING, one that only the new
build has is NEW.  Addresses, encodings and branch-target labels are dropped (the kernels may sit elsewhere in the code
object); branch offsets stay.  Names are compared demangled, without the parameter list and without the space between two template
closers (`> >`): two symbols that demangle to the same text are one kernel here.  Exits 1 on any difference.
A kernel that differs is listed with its registers in both builds (VGPRs of which AGPRs -- vgpr_count of a gfx950 code object
is the unified total --, SGPRs, VGPR / SGPR spills, scratch and LDS bytes, waves per SIMD = 512 / (VGPRs rounded up to 8), at
most 8) and marked WORSE if it spills more, gained scratch or lost a wave per SIMD.  The waves are what the registers alone
allow: LDS and the workgroup size may allow fewer in both builds, so WORSE errs on the strict side.  A translation unit that
only one of the two directories holds is reported and counted like a kernel (MISSING / NEW).
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simurlacra_amd.csrc import codeobj  # noqa: E402

DEFAULT = r"^k_"


def kernels(obj_path):
    """{demangled name without parameters: (mangled name, [instructions])} of one translation unit"""
    with tempfile.TemporaryDirectory() as tmp:
        co = codeobj.device_code_object(obj_path, os.path.join(tmp, "dev.co"))
        text = subprocess.run([codeobj._tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True,
                              check=True).stdout
    cur, out = None, {}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.startswith("\t"):
            ins = line.split("//")[0].strip()
            if ins and ins != "...":  # (the disassembler's mark for zero padding behind the last kernel of a section: no instruction)
                out[cur].append(ins)
    names = list(out)
    dm = codeobj._demangle(names)
    res = {}
    for n, d in zip(names, dm):
        # A kernel whose template ends in an EMPTY parameter pack is another symbol than the kernel without the pack (its mangled template
        # arguments gain "JE") and demangles to the same text but for one space: `k<A<0>>` against `k<A<0> >`.  Template closers
        # are written without that space here, in both builds alike; no C++ name has `> >` anywhere else.
        d = re.sub(r">\s+(?=>)", ">", d.replace("void ", "").replace("vs::", ""))
        d = re.sub(r"\(.*$", "", d)
        res[d] = (n, out[n])
    return res


def registers(row):
    return dict(row, waves=min(8, 512 // max(8, (row["vgpr_count"] + 7) // 8 * 8)))


def show(r):
    return (f"{r['vgpr_count']} v ({r['agpr_count']} a), {r['sgpr_count']} s, spills {r['vgpr_spill_count']}/{r['sgpr_spill_count']}, "
            f"scratch {r['private_segment_fixed_size']}, lds {r['group_segment_fixed_size']}, {r['waves']} waves")


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else DEFAULT)
    objs = [{f for f in os.listdir(d) if f.endswith(".o")} for d in (old_dir, new_dir)]
    checked = differ = missing = added = worse = 0
    for u in sorted(objs[0] ^ objs[1]):
        print(f"{'MISSING' if u in objs[0] else 'NEW'} unit {u}")
        missing += u in objs[0]
        added += u in objs[1]
    for u in sorted(objs[0] & objs[1]):
        old = {k: v for k, v in kernels(os.path.join(old_dir, u)).items() if pat.search(k)}
        new = {k: v for k, v in kernels(os.path.join(new_dir, u)).items() if pat.search(k)}
        regs = None
        for k, (sym, ins) in sorted(old.items()):
            checked += 1
            if k not in new:
                missing += 1
                print(f"MISSING {u}: {k}")
            elif new[k][1] != ins:
                differ += 1
                if regs is None:
                    regs = [{r["name"]: registers(r) for r in codeobj.kernels_of(os.path.join(d, u))} for d in (old_dir, new_dir)]
                ro, rn = regs[0][sym], regs[1][new[k][0]]
                bad = (rn["vgpr_spill_count"] > ro["vgpr_spill_count"] or rn["sgpr_spill_count"] > ro["sgpr_spill_count"]
                       or (rn["private_segment_fixed_size"] and not ro["private_segment_fixed_size"]) or rn["waves"] < ro["waves"])
                worse += bad
                print(f"{'WORSE  ' if bad else 'DIFFERS'} {u}: {k}  {len(ins)} -> {len(new[k][1])} instructions | {show(ro)} -> {show(rn)}")
        for k in sorted(set(new) - set(old)):
            added += 1
            print(f"NEW {u}: {k}")
        print(f"{u}: {len(old)} kernels compared", flush=True)
    print(f"{checked} kernels, {differ} differ ({worse} worse), {missing} missing, {added} new")
    sys.exit(1 if differ or missing or added else 0)


if __name__ == "__main__":
    main()
