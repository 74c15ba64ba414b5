"""Training step (forward + backward) of one deformable encoder layer (MSDeformAttnTransformerEncoderLayer) at config 3's pyramid:
N = 4 frames, levels 64^2, 32^2, 16^2 (S = 5376), C 256, 8 heads, 4 points, d_ffn 1024, dropout 0.1.  Median ms per step over
n steps (default 20) and peak memory, for the library's training tier (recompute off / on) and for the torch composition it
replaced: the module's nn.Linear / LayerNorm / dropout layers around `deformable_sample` (the HIP core op under autograd)."""
import os, statistics, sys, time
import torch
import torch.nn.functional as F_
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import axial_vs_amd as ax
from axial_vs_amd.msda import deformable_sample

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20
N, C, F, M, P = 4, 256, 1024, 8, 4
shapes = [(64, 64), (32, 32), (16, 16)]
S = sum(h * w for h, w in shapes)


def timed(step):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 30


torch.manual_seed(0)
layer = ax.MSDeformAttnTransformerEncoderLayer(C, F, dropout=0.1, n_levels=len(shapes), n_heads=M, n_points=P).cuda().train()
src = torch.randn(N, S, C, device="cuda").requires_grad_(True)
pos = (torch.randn(N, S, C, device="cuda") * 0.5).requires_grad_(True)
ref = ax.MSDeformAttnTransformerEncoder.get_reference_points(shapes, N, "cuda")
ss = torch.as_tensor(shapes, device="cuda")
g = torch.randn(N, S, C, device="cuda")


def tier_step():
    layer(src, pos, ref, ss, None, None).backward(g)


def torch_step():     # the layer's forward as the torch composition (WC/msdeformattn.py:203-216 under autograd)
    a = layer.self_attn
    sampled = deformable_sample(a.value_proj, a.sampling_offsets, a.attention_weights, src + pos, src, ref, shapes, None, None, M, P, a.im2col_step)
    x = layer.norm1(src + layer.dropout1(a.output_proj(sampled)))
    out = layer.norm2(x + layer.dropout3(layer.linear2(layer.dropout2(F_.relu(layer.linear1(x))))))
    out.backward(g)


for recompute in (False, True):
    layer.recompute = recompute
    ms, gib = timed(tier_step)
    print(f"training tier, recompute={recompute}: fwd+bwd {ms:.3f} ms/step (median of {n}), peak {gib:.2f} GiB", flush=True)
ms, gib = timed(torch_step)
print(f"torch composition around the HIP core op: fwd+bwd {ms:.3f} ms/step (median of {n}), peak {gib:.2f} GiB", flush=True)
