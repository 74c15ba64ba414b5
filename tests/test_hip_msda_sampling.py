"""GPU: the deformable-attention sampling kernels, element by element against the float64 reference and band of tests/msda_cases.py
(location convention, band and its derivation: that file's docstring).

msda_core_kernel / msda_core_bwd_kernel<SHFL> through the C-ABI (axvs_msda_core_fwd / _bwd) on every case family: samples on exact pixel
centres, half-way points and the strict bounds -1 < x < W, in the one-pixel bands where corners fall off the map, 1 x W / H x 1 / 1 x 1
maps, L = 1 and 8, every head dim of the shuffle and of the atomic reduction with partly dead last blocks, thousands of queries adding into
four value rows, unnormalised signed weights, and the sizes the within-clip module and the Tube-Link plugin really run (N = 4).
msda_gather_kernel<false, 4> / <false, 0> through axvs_msda_sample_fwd (fp32 rows out) and through MSDeformAttn.eval() (split 16-bit rows
out, then output_proj) with identity projections, zero offset weights and inputs that are exact in 16 bits, so that sampling_offsets.bias
decides the locations and the gather's fp32 accumulation is the only rounding left.  The identity output_proj is NOT exact on either
GEMM path -- below 2048 rows the gather hands over fp16 hi + lo pieces (22 bits, lo underflows below 2^-14), from 2048 rows on the 128 x 128
kernel splits the fp32 rows into two bf16 pieces (16 bits) -- so the band is asserted on axvs_msda_sample_fwd, and the module output is
held to the band plus that hand-over's rounding (2^-22 |ref| + 2^-24, or 2^-16 |ref|).
Every test prints the worst |got - ref| / band per tensor; test_zz_report lists them (profiles/msda_sampling_element_parity.txt is that
list from an MI355X)."""
import ctypes as C
import os

import pytest
import torch

import __graft_entry__ as ge
import msda_cases as mc

pytestmark = pytest.mark.gpu

LOG = []


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


@pytest.fixture(scope="module")
def refs():
    """family -> [(case, reference)], each computed once per module (real_sizes at N = 4, forward and backward), by torch in float64
    on the device (msda_cases.reference)"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = [(c, mc.reference(c, device="cuda")) for c in mc.FAMILIES[name]()]
        return cache[name]
    return get


def raw_core(case):
    """both entry points through _lib on NaN-filled output buffers, the way msda.py calls them -> (rc, dict of device tensors)"""
    from axial_vs_amd import _lib
    N, S, M, D, Lq, L, P = case.dims
    v, loc, aw, go = (x.cuda() for x in (case.value, case.loc, case.aw, case.gout))
    arr = (C.c_int * (2 * L))(*[x for hw in case.shapes for x in hw])
    nan = float("nan")
    out = torch.full((N, Lq, M * D), nan, device="cuda")
    gv, gl, ga = torch.full_like(v, nan), torch.full_like(loc, nan), torch.full_like(aw, nan)
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib().axvs_msda_core_fwd(v.data_ptr(), arr, loc.data_ptr(), aw.data_ptr(), out.data_ptr(), N, S, M, D, Lq, L, P, st)
    if rc == 0:
        rc = _lib.lib().axvs_msda_core_bwd(v.data_ptr(), arr, loc.data_ptr(), aw.data_ptr(), go.data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(),
                                           N, S, M, D, Lq, L, P, st)
    torch.cuda.synchronize()
    return rc, {"out": out, "grad_value": gv, "grad_sampling_loc": gl, "grad_attn_weight": ga}


def hold(case, got, ref, path):
    rep = mc.ratios(got, ref)
    line = mc.report_line(case, rep, path)
    print(line)
    LOG.append(line)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (case, k, "non-finite")
    assert mc.inside(rep), line
    if "grad_attn_weight" in got:       # samples outside the map come back as exactly 0.0
        dead = ref["dead"]
        assert bool((got["grad_attn_weight"].to(dead.device)[dead] == 0).all()) and bool((got["grad_sampling_loc"].to(dead.device)[dead] == 0).all()), case


def path_of(case):
    D = case.dims[3]
    return "core-shfl" if D <= 64 and D & (D - 1) == 0 else "core-atomic"


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_core_forward_and_backward_per_element(name, refs):
    import axial_vs_amd as ax
    for case, ref in refs(name):
        v, loc, aw, go = (x.cuda() for x in (case.value, case.loc, case.aw, case.gout))
        out = ax.ms_deform_attn_forward(v, case.shapes, None, loc, aw, 64)
        gv, gl, ga = ax.ms_deform_attn_backward(v, case.shapes, None, loc, aw, go, 64)
        hold(case, {"out": out, "grad_value": gv, "grad_sampling_loc": gl, "grad_attn_weight": ga}, ref, path_of(case))


@pytest.mark.parametrize("name", ["lattice", "head_dims", "degenerate_maps", "border_bands"])
def test_outputs_fully_written_over_nan_and_reproducible(name, refs):
    """NaN-filled output buffers (the shuffle path does not clear grad_sampling_loc / grad_attn_weight: the d == 0 lane of every sample
    must store) come back finite and inside the band; a second call gives the same bits in out and, on the shuffle path, in
    grad_sampling_loc and grad_attn_weight (grad_value is atomic adds: not asked)."""
    for case, ref in refs(name):
        rc, got = raw_core(case)
        assert rc == 0, case
        hold(case, got, ref, path_of(case) + "-nan")
        rc, again = raw_core(case)
        assert rc == 0 and torch.equal(got["out"], again["out"]), case
        if path_of(case) == "core-shfl":
            assert torch.equal(got["grad_sampling_loc"], again["grad_sampling_loc"]) and torch.equal(got["grad_attn_weight"], again["grad_attn_weight"]), case


def test_lattice_samples_on_the_strict_bounds_give_exactly_zero(refs):
    case, ref = [cr for cr in refs("lattice") if cr[0].name == "on_the_strict_bounds_all_zero"][0]
    rc, got = raw_core(case)
    assert rc == 0
    for k in mc.TENSORS:
        assert bool((ref[k].ref == 0).all()) and bool((got[k] == 0).all()), k


def test_nine_levels_is_an_argument_error_and_launches_nothing():
    from axial_vs_amd import _lib
    shapes = [(1, 1)] * 9
    g = torch.Generator().manual_seed(3)
    case = mc._from_px("L9", "degenerate_maps", shapes, mc._uniform_px(g, shapes, 1, 3, 2, 1, 0.1), 8, 4)
    rc, got = raw_core(case)
    assert rc == -1 and b"n_levels=9" in _lib.lib().axvs_last_error()          # AXVS_ERR_ARG (include/axvs.h)
    assert all(bool(torch.isnan(x).all()) for x in got.values())
    import axial_vs_amd as ax
    with pytest.raises(RuntimeError, match="n_levels=9"):
        ax.ms_deform_attn_forward(case.value.cuda(), shapes, None, case.loc.cuda(), case.aw.cuda(), 64)


@pytest.mark.parametrize("name,which", [("lattice", "centres_and_halfway_L4_P4"), ("border_bands", "bands_D16_L3")])
def test_autograd_function_binds_the_direct_calls(name, which, refs):
    import axial_vs_amd as ax
    case, ref = [cr for cr in refs(name) if cr[0].name == which][0]
    v, loc, aw = (x.cuda().requires_grad_(True) for x in (case.value, case.loc, case.aw))
    out = ax.MSDeformAttnFunction.apply(v, torch.as_tensor(case.shapes), None, loc, aw, 64)
    out.backward(case.gout.cuda())
    gv, gl, ga = ax.ms_deform_attn_backward(v.detach(), case.shapes, None, loc.detach(), aw.detach(), case.gout.cuda(), 64)
    assert torch.equal(out.detach(), ax.ms_deform_attn_forward(v.detach(), case.shapes, None, loc.detach(), aw.detach(), 64))
    assert torch.equal(loc.grad, gl) and torch.equal(aw.grad, ga)          # D = 8 / 16: the shuffle path, fixed order
    hold(case, {"grad_value": v.grad}, ref, "autograd")


# ---- the 16-bit gather at chosen locations ------------------------------------------------------------------------------------------
def exact16(g, *shape):
    return torch.randint(-64, 65, shape, generator=g).float() / 64.0       # 7 bits: exact in fp16 and bf16


def gather_case(name, shapes, ref_dim, P, M, N, Lq, seed, lattice):
    """-> (module, query, reference_points, input_flatten, mask, Case).  lattice: power-of-two maps, reference points on pixel centres
    (some off the map), dyadic pixel offsets -- the kernel's (rx + off sx) W - 0.5 is exact.  Otherwise reference point 0 and boxes of
    about 2 P / W: loc = off * ((rw * 0.5) / P) in fp32, repeated here operation by operation, lands in and around the border bands."""
    import axial_vs_amd as ax
    g = torch.Generator().manual_seed(seed)
    L, S, D, Cm = len(shapes), sum(h * w for h, w in shapes), 32, 32 * M
    mod = ax.MSDeformAttn(Cm, n_levels=L, n_heads=M, n_points=P, mfma_dtype="f16")
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32)                      # [L, 2] = (W, H)
    ref = torch.zeros(N, Lq, L, ref_dim)
    if lattice:
        e = 2.0 ** -10
        pool = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, e, -e, 1 - e, e - 1, 2.0, -2.0, 0.25, 3.0, -3.0])
        off = pool[torch.randint(0, len(pool), (M, L, P, 2), generator=g)]
        for l, (H, W) in enumerate(shapes):
            ref[:, :, l, 0] = (torch.randint(-2, W + 2, (N, Lq), generator=g) + 0.5) / W
            ref[:, :, l, 1] = (torch.randint(-2, H + 2, (N, Lq), generator=g) + 0.5) / H
        if ref_dim == 4:
            ref[..., 2:] = 2.0 * P / wh            # sx = rw * 0.5 / P = 1 / W: offsets in pixels (P = 4: exact)
            scale = ref[..., 2:] * 0.5 / P
        else:
            scale = (1.0 / wh).view(1, 1, L, 2).expand(N, Lq, L, 2)
        loc = ref[:, :, None, :, None, :2] + off[None, None] * scale[:, :, None, :, None, :]
    else:
        assert ref_dim == 4
        off = (mc._band_px(g, shapes, 1, 1, M, P)[0, 0] + 0.5).float()                    # [M, L, P, 2] pixel position + 0.5
        ref[..., 2:] = 2.0 * P / wh * (1 + (torch.rand(N, Lq, L, 2, generator=g) - 0.5) / wh)
        scale = ref[..., 2:] * 0.5 / P
        loc = off[None, None] * scale[:, :, None, :, None, :]
    with torch.no_grad():
        mod.sampling_offsets.weight.zero_()
        mod.sampling_offsets.bias.copy_(off.reshape(-1))
        mod.attention_weights.weight.zero_()
        mod.attention_weights.bias.zero_()
        for lin in (mod.value_proj, mod.output_proj):
            lin.weight.copy_(torch.eye(Cm))
            lin.bias.zero_()
    src, query = exact16(g, N, S, Cm), exact16(g, N, Lq, Cm)
    mask = torch.rand(N, S, generator=g) < 0.2
    value = src.masked_fill(mask[..., None], 0.0).view(N, S, M, D)
    aw = (torch.ones(1) / float(L * P)).expand(N, Lq, M, L, P)               # softmax of equal logits: fl(1 / LP)
    case = mc.Case(name, "gather", shapes, value, loc, aw, torch.zeros(N, Lq, Cm), exact=lattice)
    return mod.cuda().eval(), query, ref, src, mask, case


def sample_fwd(mod, query, ref, src, mask, shapes):
    """axvs_msda_sample_fwd (what == 1: the gather's fp32 rows, no output_proj), called the way tube_link.py calls it"""
    from axial_vs_amd import _lib
    from axial_vs_amd.modules import _workspace
    L = _lib.lib()
    N, Lq, Cm = query.shape
    S = src.shape[1]
    q, r, x, mk = query.cuda(), ref.cuda().contiguous(), src.cuda(), mask.to(torch.uint8).cuda()
    packed = mod._pack()
    st = torch.cuda.current_stream().cuda_stream
    ws = _workspace(q.device, L.axvs_msda_workspace_bytes(N, Lq, S, Cm, mod.n_heads, mod.n_levels, mod.n_points))
    arr = (C.c_int * (2 * len(shapes)))(*[v for hw in shapes for v in hw])
    out = torch.full((N, Lq, Cm), float("nan"), device="cuda")
    _lib.check(L.axvs_msda_sample_fwd(q.data_ptr(), None, r.data_ptr(), r.shape[-1], x.data_ptr(), mk.data_ptr(), arr, out.data_ptr(), packed.data_ptr(),
                                      N, Lq, S, Cm, mod.n_heads, mod.n_levels, mod.n_points, _lib.DTYPES["f16"], ws.data_ptr(), ws.numel(), st),
               "axvs_msda_sample_fwd")
    torch.cuda.synchronize()
    return out


POW2, RAGGED = [(8, 16), (4, 4), (1, 8)], [(7, 9), (25, 43)]
GATHER = [("lattice_ref2_P4", POW2, 2, 4, 2, 2, 150, True), ("lattice_ref4_P4", POW2, 4, 4, 2, 2, 150, True),
          ("lattice_ref2_P1", POW2, 2, 1, 1, 1, 333, True), ("lattice_ref2_P3", POW2, 2, 3, 2, 1, 77, True),
          ("lattice_ref2_P5", POW2, 2, 5, 2, 2, 50, True), ("lattice_ref2_P4_rows2100", [(32, 64), (8, 16)], 2, 4, 2, 1, 2100, True),
          ("bands_ref4_P4", RAGGED, 4, 4, 4, 2, 120, False), ("bands_ref4_P3", RAGGED, 4, 3, 2, 1, 65, False),
          ("bands_ref4_P4_rows2100", [(49, 85)], 4, 4, 2, 1, 2100, False)]


@pytest.mark.parametrize("name,shapes,ref_dim,P,M,N,Lq,lattice", GATHER, ids=[g[0] for g in GATHER])
def test_gather_kernel_at_chosen_locations(name, shapes, ref_dim, P, M, N, Lq, lattice):
    mod, query, ref, src, mask, case = gather_case(name, shapes, ref_dim, P, M, N, Lq, 200 + len(name), lattice)
    r = mc.reference(case, backward=False)
    sampled = sample_fwd(mod, query, ref, src, mask, shapes)
    hold(case, {"out": sampled}, r, "gather-PT4" if P == 4 else "gather-runtimeP")
    # the whole module: the same rows after the hand-over to output_proj (identity) -- see the file's docstring for the two roundings
    with torch.no_grad():
        out = mod(query.cuda(), ref.cuda(), src.cuda(), torch.as_tensor(shapes).cuda(), None, mask.cuda()).cpu().double()
    hand_over = 2.0 ** -16 * r["out"].ref.abs() if N * Lq >= 2048 else 2.0 ** -22 * r["out"].ref.abs() + 2.0 ** -24
    err = (out - r["out"].ref).abs()
    worst = float((err / (r["out"].band() + hand_over).clamp_min(1e-300)).max())       # (a zero bound asks for a zero error)
    LOG.append(f"module {case.family}/{name}: out n={err.numel()} worst={worst:.3f} (band + output_proj hand-over)")
    print(LOG[-1])
    assert bool(torch.isfinite(out).all()) and worst <= 1.0, LOG[-1]


def test_zz_report():
    """Last in the file: the measured ratios of this run, one line per case (written to $AXVS_MSDA_PARITY_OUT when that is set)."""
    print("\n".join(LOG))
    path = os.environ.get("AXVS_MSDA_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(LOG) + "\n")
