#!/bin/bash
# Register / spill summary of the kernels of any translation unit of the library whose mangled name matches a pattern:
#   tools/kernel_resources_unit.sh axvs_matching.hip 'matcher|lsap_rect' [extra hipcc flags]
# prints one line per kernel: name, VGPRs, AGPRs, spilled VGPRs / SGPRs, scratch bytes per lane, occupancy, static LDS bytes.
R=$(cd "$(dirname "$0")/.." && pwd)
UNIT=${1:?translation unit under axial_vs_amd/csrc}; PAT=${2:-.}; shift 2
cd "$R/axial_vs_amd/csrc" && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c "$@" \
  -Rpass-analysis=kernel-resource-usage -o /dev/null "$UNIT" 2>&1 |
python3 -c '
import re, sys
pat = re.compile(sys.argv[1])
keys = [("vgpr", "VGPRs"), ("agpr", "AGPRs"), ("vspill", "VGPRs Spill"), ("sspill", "SGPRs Spill"), ("scratch", "ScratchSize [bytes/lane]"),
        ("occ", "Occupancy [waves/SIMD]"), ("lds", "LDS Size [bytes/block]")]
name, vals = None, {}
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        name, vals = m.group(1), {}
        continue
    for short, key in keys:
        m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
        if m:
            vals[short] = int(m.group(1))
    if "LDS Size" in line and name:
        if pat.search(name):
            print(name, " ".join("%s %s" % (k, vals.get(k)) for k, _ in keys))
        name = None
' "$PAT"
