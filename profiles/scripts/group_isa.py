#!/usr/bin/env python3
"""The ISA condition of the global-fit kernels, checked by cross-compiling: for every instantiation of
k_group_expand, k_group_gather and k_group_jac and of the shared k_wrap_iota, no private segment and no spilled VGPR; the vector
loads and stores and the scalar loads are counted and printed beside them.  Compiles nonlin_amd/csrc/nlh_group.hip for gfx950 to
assembly (needs hipcc, no GPU), prints the summary that is committed as profiles/group_isa.txt, and exits 1 when a kernel
breaks the condition.
    python profiles/scripts/group_isa.py > profiles/group_isa.txt"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950"]        # nonlin_amd/csrc/Makefile's


def main():
    src = os.path.join(ROOT, "nonlin_amd", "csrc", "nlh_group.hip")
    asm = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", "-o", "-", src], check=True, capture_output=True, text=True).stdout
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                      for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "sgpr_count",
                                "group_segment_fixed_size", "kernarg_segment_size")}
    bad = False
    print("global-fit kernels, gfx950, flags: " + " ".join(FLAGS))
    for name in sorted(n for n in meta if "k_group_" in n or "k_wrap_iota" in n):
        body = asm[asm.index(name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        ins = [ln.split()[0] for ln in body.splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]
        count = lambda pre: sum(1 for i in ins if i.startswith(pre))
        m = meta[name]
        ok = m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
        bad |= not ok
        print(f"{name}")
        print(f"  .private_segment_fixed_size {m['private_segment_fixed_size']}  .vgpr_spill_count {m['vgpr_spill_count']}  "
              f".sgpr_spill_count {m['sgpr_spill_count']}  .vgpr_count {m['vgpr_count']}  .sgpr_count {m['sgpr_count']}  "
              f".kernarg_segment_size {m['kernarg_segment_size']}  .group_segment_fixed_size {m['group_segment_fixed_size']}")
        print(f"  instructions {len(ins)}: global_store {count('global_store')}, flat_store {count('flat_store')}, buffer_store "
              f"{count('buffer_store')}, global_load {count('global_load')}, s_load {count('s_load')}")
        print(f"  condition {'met' if ok else 'BROKEN'}")
    return 1 if bad or not any("k_group_" in n for n in meta) else 0


if __name__ == "__main__":
    sys.exit(main())
