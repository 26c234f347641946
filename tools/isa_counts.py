"""Compiler resources and instruction-class counts of the kernels in a device assembly listing (hipcc ... --cuda-device-only -S):
per kernel VGPRs, SGPRs, spills, scratch bytes, LDS bytes and the static number of MFMA, LDS-read, LDS-write, buffer-load,
buffer-store, global-load, global-store, flat and barrier instructions.  Used to set a changed kernel next to its parent (profiles/wgrad_stagger_measured.json).
usage: python tools/isa_counts.py FILE.s [name filter]   (prints one JSON object)"""
import json
import re
import sys

CLASSES = {"mfma": r"v_mfma_", "ds_read": r"ds_read_", "ds_write": r"ds_write", "buffer_load": r"buffer_load_",
           "buffer_store": r"buffer_store_", "global_load": r"global_load_", "global_store": r"global_store_", "flat": r"flat_", "barrier": r"s_barrier\b", "valu": r"v_(?!mfma_)", "salu": r"s_(?!barrier|waitcnt|nop)",
           "waitcnt": r"s_waitcnt\b"}
META = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def parse(path, flt=""):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if flt in name:
            ins = [ln.strip().split()[0] for ln in body.splitlines() if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
            out[name] = {k: sum(1 for i in ins if re.match(v, i)) for k, v in CLASSES.items()}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target|\Z)", text, re.S | re.M):
        blk = m.group(0)
        nm = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if nm in out:
            for k in META:
                out[nm][k] = int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
    return out


if __name__ == "__main__":
    print(json.dumps(parse(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""), indent=1))
