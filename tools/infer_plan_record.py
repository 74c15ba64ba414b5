"""Record of the inference planner's cases (tests/infer_plan_cases.py): every case runs once; per case one line with the stage names the
library reports and one SHA-256 per output tensor.  Two libraries choose the same stages and compute the same bits iff their outputs
are the same text:

    AXVS_LIB_PATH=tools/ab/parent.so python3 tools/infer_plan_record.py > a.txt;  python3 tools/infer_plan_record.py > b.txt;  cmp a.txt b.txt

Under `rocprofv3 --kernel-trace -- python3 tools/infer_plan_record.py --mark` every case is preceded by a launch of a marker kernel
(a fill of one complex128 element, which nothing else launches), so that tools/infer_plan_launches.py can cut the trace into cases.  Arguments: case names (default: all)."""
import hashlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import infer_plan_cases as ipc


def sha(x):
    return hashlib.sha256(x.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--mark"]
    for name in args or list(ipc.CASES):
        if "--mark" in sys.argv:
            torch.empty(1, device="cuda", dtype=torch.complex128).fill_(1)
        outs, names = ipc.run(name)
        print(f"{name} stages {','.join(names)}", flush=True)
        for k, v in outs.items():
            print(f"{name} {k} {sha(v)}", flush=True)
