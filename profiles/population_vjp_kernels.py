"""Registers and LDS of the population instantiations of the reverse-mode kernels, from the object files of an in-tree build (no GPU
needed):

    python profiles/population_vjp_kernels.py > profiles/population_vjp_kernels.txt
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simurlacra_amd.csrc import codeobj
d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "simurlacra_amd", "csrc", "build")
rows = []
for u in sorted(os.listdir(d)):
    if not u.endswith(".o"):
        continue
    ks = codeobj.kernels_of(os.path.join(d, u))
    names = codeobj._demangle([k["name"] for k in ks])
    for k, n in zip(ks, names):
        n = n.replace("void ", "").replace("vs::", "").split("(")[0]
        if ("Pop" in n and (n.startswith("k_rollout_vjp_") or "param_grad" in n)) or n.startswith("k_pop_param_reduce"):
            rows.append((n, k))
print("Registers and LDS of the population instantiations of the reverse-mode kernels (python profiles/population_vjp_kernels.py; gfx950 code")
print("objects of this build; vgpr is the unified total of which agpr; spills VGPR/SGPR; scratch and lds in bytes).")
print(f"{'kernel':58s} {'vgpr':>5s} {'agpr':>5s} {'sgpr':>5s} {'spills':>8s} {'scratch':>8s} {'lds':>7s}")
for n, k in rows:
    spills = f"{k['vgpr_spill_count']}/{k['sgpr_spill_count']}"
    print(f"{n:58s} {k['vgpr_count']:5d} {k['agpr_count']:5d} {k['sgpr_count']:5d} {spills:>8s} {k['private_segment_fixed_size']:8d} "
          f"{k['group_segment_fixed_size']:7d}")
