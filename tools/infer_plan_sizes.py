"""Every workspace size the inference layer tiers report, over a grid of shapes and planner options: one line per (option, shape)
with the value of each size query, plus axvs_axial_layer_strided_ok.  Needs no GPU.  Two libraries carve the same workspaces iff
their outputs are the same text:

    AXVS_LIB_PATH=tools/ab/parent.so python3 tools/infer_plan_sizes.py > a.txt;  python3 tools/infer_plan_sizes.py > b.txt;  cmp a.txt b.txt
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from axial_vs_amd import _lib

BS = (1, 2)
TS = (1, 2, 4, 5, 8, 9, 12, 13)
HWS = ((4, 132), (8, 8), (16, 16), (25, 43), (32, 32), (40, 51), (40, 52), (49, 85), (64, 64), (96, 112))
CFGS = ((256, 8), (128, 8), (64, 8))
FS = (96, 256, 512, 1024, 2048, 4352)
OPTIONS = [("none", None, 0), ("generic_only", b"generic_only", 1), ("no_attn_fusion", b"no_attn_fusion", 1), ("no_ffn_fusion", b"no_ffn_fusion", 1),
           ("ffn_gelu", b"ffn_gelu", 1)] + [(f"plan_force={v}", b"plan_force", v) for v in (1, 2, 4, 8, 16, 32, 64)]


def main():
    L = _lib.lib()
    for tag, key, value in OPTIONS:
        if key:
            _lib.check(L.axvs_set_option(key, value), "axvs_set_option")
        try:
            for C, heads in CFGS:
                for F in FS:
                    print(f"{tag} C={C} F={F} strided_ok={L.axvs_axial_layer_strided_ok(C, heads, F)}")
                    for B in BS:
                        for T in TS:
                            for H, W in HWS:
                                a = (B, T, H, W, C, heads, F)
                                ex = [L.axvs_axial_layer_workspace_bytes_ex(*a, maps, sine) for maps in (0, 1) for sine in (0, 1)]
                                strided = [L.axvs_axial_layer_workspace_bytes_strided(*a, s) for s in (H * W, H * W + 37, 21504)]
                                M = B * T * H * W
                                print(tag, *a, "layer", L.axvs_axial_layer_workspace_bytes(*a), "ex", *ex, "strided", *strided,
                                      "sine3d", L.axvs_axial_layer_sine3d_workspace_bytes(*a),
                                      "traj_attn", L.axvs_traj_attn_workspace_bytes(B * W, T, H, C, heads), L.axvs_traj_attn_workspace_bytes(B * H, T, W, C, heads),
                                      "traj_layer", L.axvs_traj_layer_workspace_bytes(B, T, H * W, C, heads, F), "ffn", L.axvs_ffn_workspace_bytes(M, C, F),
                                      "cc_layer", L.axvs_cc_layer_workspace_bytes(B, H, T), "cc_module", L.axvs_cc_module_workspace_bytes(B, H, T, 2))
        finally:
            if key:
                L.axvs_set_option(key, 0)


if __name__ == "__main__":
    main()
