"""Compare the instruction streams of the fused rollout kernels between two builds of libvecsim (no GPU needed).

    python profiles/compare_isa.py OLD_OBJ_DIR NEW_OBJ_DIR [REGEX]

OLD_OBJ_DIR / NEW_OBJ_DIR are the `build/` object directories of two in-tree builds (simurlacra_amd/csrc/build), e.g. one of
the parent commit and one of the working tree.  Every kernel of the old build whose name matches REGEX (default: the
k_rollout_fnn, k_rollout_rnn and k_rollout_ws families) must exist in the new build with the same instructions.  Addresses,
encodings and branch-target labels are dropped (the kernels may sit elsewhere in the code object); branch offsets stay.
Names are compared demangled, without the parameter list.  The POP template flag of k_rollout_fnn / k_rollout_rnn (the
population kernels of vs_set_policy_population, default false) is dropped from the new names, so `k_rollout_fnn<.., MF, false>`
of the new build is `k_rollout_fnn<.., MF>` of the old one.  Exits 1 on any difference.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simurlacra_amd.csrc import codeobj  # noqa: E402

DEFAULT = r"^k_rollout_(fnn|rnn|ws)<"


def kernels(obj_path):
    """{demangled name without parameters: [instructions]} of one translation unit"""
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
            if ins:
                out[cur].append(ins)
    names = list(out)
    dm = codeobj._demangle(names)
    res = {}
    for n, d in zip(names, dm):
        d = d.replace("void ", "").replace("vs::", "")
        d = re.sub(r"\(.*$", "", d)
        res[d] = out[n]
    return res


def normalise(name):
    """the new build's name of a pre-existing instantiation -> the old build's name (POP = false dropped)"""
    m = re.match(r"^(k_rollout_(fnn|rnn))<(.*)>$", name)
    if not m:
        return name
    args = [a.strip() for a in re.split(r",(?![^<]*>)", m.group(3))]
    want = 7 if m.group(2) == "fnn" else 5
    if len(args) == want and args[-1] == "false":
        args = args[:-1]
    elif len(args) == want:
        return None  # a POP = true instantiation: new
    return f"{m.group(1)}<{', '.join(args)}>"


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else DEFAULT)
    units = sorted(f for f in os.listdir(old_dir) if f.endswith(".o"))
    checked = differ = missing = 0
    for u in units:
        old = {k: v for k, v in kernels(os.path.join(old_dir, u)).items() if pat.search(k)}
        new = {}
        for k, v in kernels(os.path.join(new_dir, u)).items():
            if pat.search(k):
                nk = normalise(k)
                if nk is not None:
                    new[nk] = v
        for k, ins in sorted(old.items()):
            checked += 1
            if k not in new:
                missing += 1
                print(f"MISSING {u}: {k}")
            elif new[k] != ins:
                differ += 1
                first = next((i for i, (a, b) in enumerate(zip(ins, new[k])) if a != b), min(len(ins), len(new[k])))
                print(f"DIFFERS {u}: {k} ({len(ins)} -> {len(new[k])} instructions, first difference at {first})")
        print(f"{u}: {len(old)} kernels compared", flush=True)
    print(f"{checked} kernels, {differ} differ, {missing} missing")
    sys.exit(1 if differ or missing else 0)


if __name__ == "__main__":
    main()
