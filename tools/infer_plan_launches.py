#!/usr/bin/env python3
"""Reduce a `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/infer_plan_record.py --mark` trace to the ordered
list of the library's launches per case of tests/infer_plan_cases.py: kernel name with its template arguments, grid, workgroup size,
LDS bytes.  Two libraries launch the same kernels iff the two texts are identical.

    python3 tools/infer_plan_launches.py DIR > launches.txt
"""
import csv, glob, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import infer_plan_cases as ipc

MARK = "complex<double>"      # the marker in front of every case: a fill of a complex128 tensor, which nothing else in the run launches


def short(name):
    """the kernel's name without its parameter list"""
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                return name[:i].replace("void ", "")
    return name


def main(trace_dir):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cols = rows[0].keys()
    grid = [c for c in cols if c.startswith("Grid_Size")]
    wg = [c for c in cols if c.startswith("Workgroup_Size")]
    lds = [c for c in cols if "LDS" in c]
    names, case = list(ipc.CASES), -1
    print("# case, kernel, grid:", *grid, "wg:", *wg, "lds:", *lds)
    for r in rows:
        n = r["Kernel_Name"]
        if MARK in n:
            case += 1
        elif "axvs::" in n and case >= 0:
            print(names[case], short(n), "grid", *[r[c] for c in grid], "wg", *[r[c] for c in wg], "lds", *[r[c] for c in lds])
    assert case == len(names) - 1, f"{case + 1} markers for {len(names)} cases"


if __name__ == "__main__":
    main(sys.argv[1])
