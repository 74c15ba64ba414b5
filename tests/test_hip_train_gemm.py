"""GPU: the training tier's split-precision GEMMs, one call at a time through the host dispatch (axvs_test_train_gemm, include/axvs.h):
tr_gemm_nt_kernel (forward and input-gradient form, every epilogue, split-K, the affine loader), tr_gemm_tn_kernel (weight-gradient
partials and the mask einsum with its tile statistics and grouped rows), the deterministic partial reducers and the transpose of dgrad.
Every result is held against the same operation in float64 on the CPU, ELEMENT BY ELEMENT:

    |C - C64| <= tol * ((|A| |B|^T) + |epilogue terms|)        (the bound scaled by the element's own magnitudes)

where A is the loaded operand (|x| + |pos| for the addend, |c0 x| + |c1 y| + |c2| for the affine loader), the product term is scaled by
|mul| and the dropout factor, and beta C, res, res2 enter with their magnitudes.  16-bit outputs add their own rounding (2^-11 |C64| for
f16, 2^-8 for bf16).  tol is per arithmetic class -- which class a call ran in is read off the instantiation the dispatch launched:

    class   arithmetic                                        worst ratio measured on an MI355X   tol     (per-product worst case)
    ns3     three bf16 pieces per operand (exact forwards)    3.86e-7                             1e-6    (~6e-7: 2^-24 pieces, six fp32 adds)
    gelu    ns3 with an exact-GELU epilogue (relu = 2 / 3)    3.16e-7                             1e-6    (as ns3; see below)
    ns2     two pieces (input and weight gradients, einsum)   2.57e-5                             5e-5    (3 * 2^-16 = 4.6e-5)
    f16     one fp16 piece (train_amp = 2)                    8.44e-4                             2e-3    (2^-10 = 9.8e-4)
    bf16    one bf16 piece (train_amp = 1)                    7.35e-3                             1.6e-2  (2^-7 = 7.8e-3)

The worst ratios come from K = 1 .. 4, where one product is all an element holds (the header's "NS=2 ~ 1.5e-5 relative" is the
typical product; the worst one is 2^-16 per operand residual plus the dropped lo.lo term).  Every bound is at most 4x its measured
worst ratio and at least the per-product worst case, and test_bounds_reject_the_next_coarser_arithmetic shows each one rejects the
arithmetic one class coarser on the same inputs (K = 1: ns2 2.1e-5 against the ns3 bound, f16 8.4e-4 against ns2's, bf16 7.3e-3
against f16's).
The gelu class: the kernel applies 0.5 x (1 + erf(x / sqrt 2)) to an ns3 result x.  |gelu'| <= 1.129, so the error of x, at most tol times
the element's magnitude term, comes out at most 1.13 times larger: the magnitude term of everything in front of the GELU is multiplied by
1.13 (GELU_SLOPE) and the ns3 tol carries over.  The device erff's own error is not derived but measured: it is part of the 3.16e-7 above
(against float64 erf, relative to the scaled magnitude), and 1e-6 is within 4x of that and not below ns3's per-product worst case.
Output buffers carry NaN guards (rows past M, columns past N inside the row stride, the slot past the last split-K partial, rows between
output groups, unwritten statistics slots): they must come back bit-identical, and NaN operand padding turns any read outside an
operand's extent into a NaN in the result."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import axvs_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"ns3": 1e-6, "gelu": 1e-6, "ns2": 5e-5, "f16": 2e-3, "bf16": 1.6e-2}      # (the table above)
U16 = {1: (2.0 ** -11, 2.0 ** -25), 2: (2.0 ** -8, 1e-38)}   # kind16 -> (rounding unit, absolute floor) of the 16-bit output
MEASURED = {k: 0.0 for k in TOL}
SEEN = []          # (variant launched, variant the dispatch rules give, case) of every call in this file


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def lib():
    from axial_vs_amd import _lib
    return _lib.lib()


# ---- instantiation ids (AxvsTestGemm::variant) and the dispatch rules of Gemm (axvs_train.hip) --------------------------------------
def nt_var(ns, gen=False, add=False, f16=False, aff=False, act=False, sum_=False):
    return 0x100 | ns | gen << 2 | add << 3 | f16 << 4 | aff << 5 | act << 6 | sum_ << 7


SUM_STEPS = 64      # three pieces: more 32-wide k-steps than this in one accumulator take the step sums (kNtSumSteps, csrc/axvs_gemm_nt.hip)


def deep(K, ksteps=0):
    """an accumulator's k-steps (of one split-K partial) are past SUM_STEPS"""
    nk = (K + 31) // 32
    return (min(ksteps, nk) if ksteps else nk) > SUM_STEPS


def tn_var(gen, amp=0, stats=False, grp=False):
    return 0x200 | gen | amp << 1 | stats << 3 | grp << 4


def vname(v):
    if v >> 8 == 1:
        flags = [n for n, b in (("GEN", 4), ("ADD", 8), ("F16", 16), ("AFF", 32), ("ACT", 64), ("SUM", 128)) if v & b]
        return f"nt<{v & 3}{''.join(',' + f for f in flags)}>"
    if v >> 8 == 2:
        flags = [n for n, b in (("GEN", 1), ("STATS", 8), ("GRP", 16)) if v & b]
        return f"tn<AMP={(v >> 1) & 3}{''.join(',' + f for f in flags)}>"
    return f"none({v})"


def vclass(v):
    if v >> 8 == 1:
        ns = v & 3
        if v & 64:
            return "gelu"
        return "ns3" if ns == 3 else "ns2" if ns == 2 else ("f16" if v & 16 else "bf16")
    amp = (v >> 1) & 3
    return "ns2" if amp == 0 else "bf16" if amp == 1 else "f16"


def registered():
    """Every instantiation the dispatch rules of Gemm can reach (expect_nt, expect_wgrad and expect_tn below state the same rules per
    call), as variant ids."""
    out = set()
    for gen, add in ((False, False), (True, False), (False, True)):      # the general loader takes the addend at run time: no GEN + ADD
        out |= {nt_var(ns, gen, add) for ns in (2, 3)}                   # split precision: two pieces, or three when exact
        out |= {nt_var(1, gen, add, f16) for f16 in (False, True)}       # train_amp 1 (bf16) / 2 (fp16): one piece
    out |= {nt_var(2, gen, aff=True) for gen in (False, True)}           # the affine loader: two pieces, no addend
    out |= {nt_var(3, act=True)}                                         # the GELU epilogues: three pieces, 16-byte loader, no addend
    out |= {nt_var(3, gen, add, sum_=True) for gen, add in ((False, False), (True, False), (False, True))} | {nt_var(3, act=True, sum_=True)}      # past SUM_STEPS
    out |= {tn_var(False, amp) for amp in (0, 1, 2)}                     # weight gradient: 16-byte loader, follows train_amp
    for gen in (False, True):                                            # einsum: plain, with statistics, or grouped output rows
        out |= {tn_var(gen), tn_var(gen, stats=True), tn_var(gen, grp=True)}
    return out


def amp_mode():
    from axial_vs_amd import _lib
    return _lib.current_amp()


def expect_nt(K, exact, al_a=4, al_b=4, a2=False, aff=False, gelu=0, ksteps=0):
    """K % 4 != 0 or a row alignment below 16 bytes: the general loader; the addend without it: ADD; the affine loader: two pieces
    whatever `exact` and train_amp; train_amp: one 16-bit piece whatever `exact`; else three pieces iff exact.  relu = 2 / 3 (the
    GELU epilogues): the one ACT instantiation -- any other combination with them is refused (test_train_gemm_cpu.py).  Three pieces over
    more than SUM_STEPS k-steps per accumulator: the same instantiation with step sums."""
    gen = al_a != 4 or al_b != 4 or K % 4 != 0
    if gelu:
        return nt_var(3, act=True, sum_=deep(K, ksteps))
    if aff:
        return nt_var(2, gen, aff=True)
    amp = amp_mode()
    if amp:
        return nt_var(1, gen, a2 and not gen, amp == 2)
    return nt_var(3 if exact else 2, gen, a2 and not gen, sum_=bool(exact) and deep(K, ksteps))


def amp(mode):
    from axial_vs_amd import _lib
    return _lib.train_amp(mode)


# ---- NaN-guarded device buffers ---------------------------------------------------------------------------------------------------
class Mat:
    """rows x cols fp32 with row stride ld, starting `off` floats into a NaN-filled device buffer: the guards around it are NaN."""

    def __init__(self, data, ld=None, off=0, tail=16):
        self.rows, self.cols = data.shape
        self.ld, self.off = ld or self.cols, off
        host = torch.full((off + self.rows * self.ld + tail,), float("nan"))
        self.view(host)[:] = data
        self.before = host.clone()
        self.buf = host.cuda()

    def view(self, flat):
        return flat[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def get(self):
        return self.view(self.buf.cpu()).double()

    def assert_guards(self, written=True):
        """Every float outside the sub-matrix (all of them when not `written`) is bit-identical to what was there."""
        now = self.buf.cpu().view(torch.int32)
        keep = torch.ones(now.numel(), dtype=torch.bool)
        if written:
            self.view(keep)[:] = False
        bad = (now != self.before.view(torch.int32)) & keep
        assert not bool(bad.any()), f"{int(bad.sum())} guard floats overwritten, first at flat index {int(bad.nonzero()[0])}"


def rnd(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def nan(rows, cols):
    return torch.full((rows, cols), float("nan"))


def layout(K, al, i=0):
    """(row stride, offset) of an operand whose rows start at `al` floats: 4 aligned (optionally padded), 2 / 1 unaligned"""
    if al == 4:
        return ((K + 3) // 4 * 4 + 4 * (i % 2), 0)
    if al == 2:
        return (K + K % 2 + 2, 2)
    return (K + 3, 1)


def check(out, ref, mag, cls, what, u16=None):
    """Element-wise bound; records the worst ratio of the class."""
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite output"
    err = (out - ref).abs()
    if u16 is not None:                 # the 16-bit rounding of the result is not the arithmetic's error
        u, floor = u16
        err = (err - u * ref.abs() - floor).clamp_min(0.0) / (1.0 + u)
    ratio = float((err / (mag + 1e-30)).max())
    MEASURED[cls] = max(MEASURED[cls], ratio)
    assert ratio <= TOL[cls], f"{what}: worst |C - C64| / bound-magnitude = {ratio:.3e} > {TOL[cls]:.1e} ({cls})"
    return ratio


def call(op, M, N, K, A, B, Cm, expect, what, scratch_min=0, **kw):
    from axial_vs_amd import _lib
    t = _lib.AxvsTestGemm()
    t.op = _lib.TEST_GEMM_OPS[op]
    t.a, t.b, t.c = A.ptr, B.ptr, Cm.ptr
    t.M, t.N, t.K = M, N, K
    t.lda, t.ldb, t.ldc = A.ld, B.ld, Cm.ld
    t.al_a = t.al_b = t.al_c = 4
    t.mul = t.drop_scale = 1.0
    t.zsplits = 1
    for k, v in kw.items():
        setattr(t, k, v)
    nbytes = lib().axvs_test_train_gemm_scratch_bytes(C.byref(t))
    scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    rc = lib().axvs_test_train_gemm(C.byref(t), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"{what}: {lib().axvs_last_error().decode()}"
    torch.cuda.synchronize()
    SEEN.append((t.variant, expect, what))
    assert t.variant == expect, f"{what}: launched {vname(t.variant)}, the dispatch rules give {vname(expect)}"
    return t.variant


def drop_factors(M, N, p, seed, site):
    """Kernel dropout of element row * N + col: orc.dropout_keep's mask times the fp32 scale the library passes"""
    keep = orc.dropout_keep(seed, site, M * N, p).view(M, N) != 0
    return keep.double() * float(np.float32(1.0 / (1.0 - p)))


# ---- nt / fwd / dgrad --------------------------------------------------------------------------------------------------------------
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


GELU_SLOPE = 1.13      # |gelu'| <= 1.129: an error of the argument comes out at most this much larger


def nt_case(M, N, K, exact=1, seed=0, op="nt", al_a=4, al_b=4, ldc_pad=0, stride=0, a2=False, aff_rows=0, bias=False, mul=1.0, relu=False,
            p_drop=0.0, beta=0.0, res=False, res2=False, kind16=0, zero_rows=False, ksteps=0, zsplits=1, gelu=0):
    """gelu (AxvsTestGemm::relu): 2 = exact GELU in the ReLU's place, 3 = exact GELU after the sums"""
    g = torch.Generator().manual_seed(1000 + seed)
    what = (f"{op} M={M} N={N} K={K} exact={exact} al={al_a}/{al_b} ldc+{ldc_pad} a2={a2} aff={aff_rows} bias={bias} mul={mul} relu={relu} gelu={gelu} "
            f"p={p_drop} beta={beta} res={res}/{res2} out16={kind16} ksteps={ksteps}x{zsplits} amp={amp_mode()}")
    a, b = rnd(g, M, K), rnd(g, N, K)
    lda, offa = layout(K, al_a, stride)
    ldb, offb = layout(K, al_b, stride + 1)
    if op == "fwd":
        lda, offa, ldb, offb, ldc_pad = K, 0, K, 0, 0
    A, B = Mat(a, lda, offa), Mat(b, ldb, offb)
    ldc = N + ldc_pad
    kw = dict(exact=exact, mul=mul, relu=gelu or int(relu), beta=beta)
    if op == "nt":
        kw.update(al_a=al_a, al_b=al_b)
    a64, mag_a = a.double(), a.double().abs()
    keep = []
    if a2 or aff_rows:
        x2 = rnd(g, M, K)
        A2 = Mat(x2, lda, offa)                     # the addend shares A's layout (GemmLd::a2)
        keep.append(A2)
        kw["a2"] = A2.ptr
        if aff_rows:
            G = (M + aff_rows - 1) // aff_rows
            coef = rnd(g, G, 3)
            cf = Mat(coef.reshape(1, 3 * G))
            keep.append(cf)
            kw["aff"], kw["aff_rows"] = cf.ptr, aff_rows
            rows = coef.double()[torch.arange(M) // aff_rows]
            a64 = rows[:, :1] * a64 + rows[:, 1:2] * x2.double() + rows[:, 2:3]
            mag_a = rows[:, :1].abs() * mag_a + rows[:, 1:2].abs() * x2.double().abs() + rows[:, 2:3].abs()
        else:
            a64 = a64 + x2.double()
            mag_a = mag_a + x2.double().abs()
    b64 = b.double()
    nz = zsplits if ksteps else 1
    # the product, per split-K partial z over k-steps [z ksteps, (z + 1) ksteps)
    kr = [(z * ksteps * 32, min((z + 1) * ksteps * 32, K)) if ksteps else (0, K) for z in range(nz)]
    acc = torch.stack([a64[:, k0:k1] @ b64[:, k0:k1].T if k1 > k0 else torch.zeros(M, N, dtype=torch.float64) for k0, k1 in kr])
    mag = torch.stack([mag_a[:, k0:k1] @ b64[:, k0:k1].abs().T if k1 > k0 else torch.zeros(M, N, dtype=torch.float64) for k0, k1 in kr])
    ref, magr = acc, mag
    if bias:
        bv = rnd(g, N)
        Bv = Mat(bv.reshape(1, N))
        keep.append(Bv)
        kw["bias"] = Bv.ptr
        ref, magr = ref + bv.double(), magr + bv.double().abs()
    ref, magr = ref * mul, magr * abs(mul)
    if relu:
        ref = ref.clamp_min(0.0)
    if gelu == 2:
        ref, magr = gelu64(ref), GELU_SLOPE * magr
    if p_drop:
        f = drop_factors(M, N, p_drop, 1234 + seed, 7)
        kw.update(drop_seed=1234 + seed, drop_site=7, drop_thr=int(p_drop * 2 ** 24), drop_scale=1.0 / (1.0 - p_drop))
        ref, magr = ref * f, magr * f
    c0 = rnd(g, nz * M, N) if beta else nan(nz * M, N)
    Cm = Mat(c0, ldc)
    if beta:
        ref = ref + beta * c0.double().view(nz, M, N)
        magr = magr + abs(beta) * c0.double().abs().view(nz, M, N)
    for flag, name in ((res, "res"), (res2, "res2")):
        if flag:
            r = rnd(g, M, N)
            R = Mat(r, ldc)
            keep.append(R)
            kw[name] = R.ptr
            ref, magr = ref + r.double(), magr + r.double().abs()
    if gelu == 3:
        ref, magr = gelu64(ref), GELU_SLOPE * magr
    if ksteps:
        kw.update(ksteps=ksteps, zsplits=zsplits + 1)     # one more z than the k-steps need: it must write a zero partial
        Cm = Mat(nan((nz + 1) * M, N), ldc)
        ref = torch.cat([ref, torch.zeros(1, M, N, dtype=torch.float64)])
        magr = torch.cat([magr, torch.zeros(1, M, N, dtype=torch.float64)])
        nz += 1
    o16 = None
    if kind16:
        nblk = (N + 31) // 32
        o16 = torch.full((nblk * M * 32,), -1, dtype=torch.int16, device="cuda")      # 0xFFFF: NaN in both 16-bit types
        kw.update(out16=o16.data_ptr(), kind16=kind16)
        if zero_rows:
            zr = (torch.arange(M) % 3 == 1).to(torch.uint8)
            zr_d = zr.cuda()
            keep.append(zr_d)
            kw["zero_rows"] = zr_d.data_ptr()
    expect = expect_nt(K, exact, al_a if op == "nt" else 4, al_b if op == "nt" else 4, a2 and not aff_rows, aff_rows > 0, gelu, ksteps)
    v = call(op, M, N, K, A, B, Cm, expect, what, **kw)
    cls = vclass(v)
    if kind16:
        Cm.assert_guards(written=False)                 # the fp32 rows are not touched
        raw = o16.cpu()
        r_idx = torch.arange(M).view(M, 1)
        k_idx = torch.arange(N).view(1, N)
        flat = ((k_idx // 32) * M + r_idx) * 32 + k_idx % 32
        got = raw[flat].view(torch.float16 if kind16 == 1 else torch.bfloat16).double()
        untouched = torch.ones(raw.numel(), dtype=torch.bool)
        untouched[flat.reshape(-1)] = False
        assert bool((raw[untouched] == -1).all()), f"{what}: 16-bit slots outside [M, N] written"
        ref, magr = ref[0], magr[0]
        if zero_rows:
            zero = zr.bool()
            assert bool((raw[flat][zero] == 0).all()), f"{what}: zero_rows not written as +0"
            got, ref, magr = got[~zero], ref[~zero], magr[~zero]
        return check(got, ref, magr, cls, what, U16[kind16])
    Cm.assert_guards()
    out = Cm.get().view(nz, M, N)
    if ksteps:
        assert bool((out[-1] == 0).all()), f"{what}: the split with no k-steps must write a zero partial"
        assert bool(torch.isfinite(out[:-1].sum(0)).all())
    return check(out, ref, magr, cls, what)


MS, NS, KS = [1, 127, 128, 129, 1000], [4, 124, 128, 132, 260], [1, 3, 4, 31, 32, 33, 65, 1000]
# every (M, K) pair once (5 and 8 are coprime), N cycling; layouts: aligned, padded strides, rows at +2 and +1 floats
SHAPES = [(MS[i % 5], NS[(3 * i + i // 5) % 5], KS[i % 8], i) for i in range(40)]
ALIGN = [(4, 4), (4, 4), (2, 4), (1, 1), (4, 2), (1, 4)]


@pytest.mark.parametrize("M,N,K,i", SHAPES, ids=[f"M{m}_N{n}_K{k}" for m, n, k, _ in SHAPES])
def test_nt_shapes_and_layouts(M, N, K, i):
    al_a, al_b = ALIGN[i % len(ALIGN)]
    for exact in (1, 0):
        nt_case(M, N, K, exact, seed=i, al_a=al_a, al_b=al_b, stride=i, ldc_pad=8 * (i % 3))


EPILOGUES = [dict(), dict(bias=True), dict(mul=-0.75), dict(relu=True), dict(p_drop=0.25), dict(beta=1.0), dict(res=True),
             dict(res2=True), dict(bias=True, mul=1.5, relu=True, p_drop=0.25, beta=1.0, res=True, res2=True)]


@pytest.mark.parametrize("shape", [(129, 132, 33, 1), (1000, 260, 64, 0), (127, 4, 1000, 0)], ids=["gen", "aligned", "narrow"])
@pytest.mark.parametrize("e", range(len(EPILOGUES)), ids=["plain", "bias", "mul", "relu", "drop", "beta", "res", "res2", "all"])
def test_nt_epilogue_terms(shape, e):
    M, N, K, exact = shape
    nt_case(M, N, K, exact, seed=50 + e, ldc_pad=12, stride=1, **EPILOGUES[e])


@pytest.mark.parametrize("gelu", [2, 3], ids=["in_relus_place", "after_residual"])
@pytest.mark.parametrize("M,N,K", [(m, n, k) for m in (1, 129) for n in (4, 132) for k in (4, 36)])
def test_nt_gelu_epilogues(M, N, K, gelu):
    """The ACT instantiation (the query decoders' Linear layers): out = gelu((A B^T + bias) mul) + res, or gelu(... + res), against
    float64 0.5 x (1 + erf(x / sqrt 2)); one partial tile in each dimension."""
    nt_case(M, N, K, 1, seed=40 + gelu, gelu=gelu, bias=True, mul=1.5, res=True, ldc_pad=8, stride=1)
    nt_case(M, N, K, 1, seed=42 + gelu, gelu=gelu, mul=-0.75)
    nt_case(M, N, K, 1, seed=44 + gelu, gelu=gelu, bias=True, beta=1.0, res=True, res2=True, p_drop=0.25)


@pytest.mark.parametrize("K", [64, 33, 1000])
@pytest.mark.parametrize("exact", [1, 0])
def test_nt_addend_on_both_loaders(K, exact):
    nt_case(200, 132, K, exact, seed=K, a2=True, ldc_pad=4, stride=1, bias=True)
    nt_case(200, 132, K, exact, seed=K + 1, a2=True, al_a=1, al_b=2)


@pytest.mark.parametrize("K", [64, 33])
def test_nt_affine_loader_with_groups_not_dividing_the_tile(K):
    nt_case(300, 132, K, 1, seed=5, aff_rows=100, ldc_pad=4)        # two pieces whatever `exact`
    nt_case(257, 128, K, 0, seed=6, aff_rows=100, al_a=1, beta=1.0)


@pytest.mark.parametrize("K,ksteps,splits", [(1000, 11, 3), (999, 8, 4), (65, 1, 3), (4200, 70, 2)])      # (the last: partials past SUM_STEPS)
def test_nt_split_k_partials(K, ksteps, splits):
    nt_case(129, 132, K, 1, seed=K, ksteps=ksteps, zsplits=splits, ldc_pad=8)
    nt_case(300, 128, K, 0, seed=K + 1, ksteps=ksteps, zsplits=splits, aff_rows=100)


@pytest.mark.parametrize("kind16", [1, 2], ids=["f16", "bf16"])
def test_nt_out16_blocked_with_zero_rows(kind16):
    nt_case(129, 100, 64, 1, seed=kind16, kind16=kind16, zero_rows=True, bias=True, relu=True)
    nt_case(200, 260, 33, 0, seed=kind16 + 2, kind16=kind16, mul=0.5, p_drop=0.25)
    nt_case(1, 4, 1, 1, seed=kind16 + 4, kind16=kind16)


def test_fwd():
    nt_case(200, 132, 64, 1, seed=11, op="fwd", a2=True, bias=True, relu=True, beta=1.0)
    nt_case(129, 124, 36, 1, seed=12, op="fwd", p_drop=0.25)
    nt_case(1, 4, 1000, 0, seed=13, op="fwd", res=True)


@pytest.mark.parametrize("mode", [1, 2], ids=["bf16", "f16"])
def test_nt_under_amp_ignores_exact(mode):
    with amp(mode):
        nt_case(129, 132, 64, 1, seed=20 + mode, bias=True)
        nt_case(129, 132, 64, 0, seed=22 + mode, a2=True)
        nt_case(129, 132, 33, 1, seed=24 + mode, a2=True, p_drop=0.25)
        nt_case(127, 124, 64, 1, seed=26 + mode, al_a=2, beta=1.0)
        nt_case(300, 128, 64, 1, seed=28 + mode, aff_rows=100)       # the affine loader stays two-piece under AMP
        nt_case(129, 132, 64, 1, seed=30 + mode, kind16=mode)
        dgrad_case(129, 132, 68, 1, seed=32 + mode)


def dgrad_case(M, N, K, exact, seed, beta=0.0, mul=1.0, res=False, res2=False, ldy_pad=0):
    """dX[M,K] = beta dX + mul dY[M,N] W[N,K] + res + res2"""
    g = torch.Generator().manual_seed(2000 + seed)
    what = f"dgrad M={M} N={N} K={K} exact={exact} beta={beta} mul={mul} res={res}/{res2} ldy+{ldy_pad} amp={amp_mode()}"
    dy, w = rnd(g, M, N), rnd(g, N, K)
    A, B = Mat(dy, N + ldy_pad), Mat(w)
    c0 = rnd(g, M, K) if beta else nan(M, K)
    Cm = Mat(c0)
    ref, mag = (dy.double() @ w.double()) * mul, (dy.double().abs() @ w.double().abs()) * abs(mul)
    kw, keep = dict(exact=exact, beta=beta, mul=mul), []
    if beta:
        ref, mag = ref + beta * c0.double(), mag + abs(beta) * c0.double().abs()
    for flag, name in ((res, "res"), (res2, "res2")):
        if flag:
            r = rnd(g, M, K)
            R = Mat(r)
            keep.append(R)
            kw[name] = R.ptr
            ref, mag = ref + r.double(), mag + r.double().abs()
    v = call("dgrad", M, N, K, A, B, Cm, expect_nt(N, exact), what, **kw)
    Cm.assert_guards()
    B.assert_guards(written=False)
    return check(Cm.get(), ref, mag, vclass(v), what)


@pytest.mark.parametrize("exact", [1, 0])
def test_dgrad(exact):
    dgrad_case(129, 132, 68, exact, seed=1, beta=1.0, mul=0.5, res=True, res2=True, ldy_pad=4)
    dgrad_case(1000, 36, 260, exact, seed=2)
    dgrad_case(1, 4, 4, exact, seed=3, res=True)
    dgrad_case(127, 260, 132, exact, seed=4, beta=1.0)


# ---- wgrad --------------------------------------------------------------------------------------------------------------------------
def wgrad_case(M, N, K, seed, mul=1.0, ldy_pad=0, ldx_pad=0, db=True):
    g = torch.Generator().manual_seed(3000 + seed)
    what = f"wgrad M={M} N={N} K={K} mul={mul} ldy+{ldy_pad} ldx+{ldx_pad} db={db} amp={amp_mode()}"
    dy, x = rnd(g, M, N), rnd(g, M, K)
    j0 = N // 3                              # a column of dY whose sum is exactly zero: +v, -v pairs (and a zero for odd M)
    col = torch.zeros(M)
    h = rnd(g, M // 2)
    col[0:2 * (M // 2):2], col[1:2 * (M // 2):2] = h, -h
    dy[:, j0] = col
    A, X = Mat(dy, N + ldy_pad), Mat(x, K + ldx_pad)
    results = []
    for rep in range(2):
        W = Mat(nan(N, K))
        D = Mat(nan(1, N))
        v = call("wgrad", M, N, K, A, X, W, tn_var(False, amp_mode()), what, mul=mul, db=D.ptr if db else None)
        W.assert_guards()
        D.assert_guards(written=db)
        results.append((W.buf.cpu(), D.buf.cpu()))
    # no atomics: a second call gives the same bits
    assert torch.equal(results[0][0].view(torch.int32), results[1][0].view(torch.int32)), f"{what}: dW not bit-reproducible"
    assert torch.equal(results[0][1].view(torch.int32), results[1][1].view(torch.int32)), f"{what}: db not bit-reproducible"
    ref = (dy.double().T @ x.double()) * mul
    mag = (dy.double().abs().T @ x.double().abs()) * abs(mul)
    check(W.get(), ref, mag, vclass(v), what)
    if db:
        # the bias gradient is an fp32 sum (not split): within 1e-6 of sum |dY| per column, also where it cancels to exactly zero
        got = D.get()[0]
        refb = dy.double().sum(0) * mul
        scale = dy.double().abs().sum(0) * abs(mul)
        err = (got - refb).abs()
        assert bool((err <= 1e-6 * scale).all()), f"{what}: db off by {float((err / scale).max()):.2e} of sum |dY|"
        assert float(err[j0]) <= 1e-6 * float(scale[j0]), f"{what}: the cancelling column's db = {float(got[j0]):.3e}"


@pytest.mark.parametrize("M", [1, 31, 32, 33, 2048, 2049, 200_001])
def test_wgrad(M):
    if M > 10_000:
        wgrad_case(M, 24, 40, seed=M, mul=-1.5, ldy_pad=4, ldx_pad=8)
    else:
        wgrad_case(M, 136, 72, seed=M, ldy_pad=4 * (M % 3), ldx_pad=8 * (M % 2))
        wgrad_case(M, 8, 264, seed=M + 1, mul=0.25, db=M % 2 == 1)


@pytest.mark.parametrize("mode", [1, 2], ids=["bf16", "f16"])
def test_wgrad_under_amp(mode):
    with amp(mode):
        wgrad_case(2049, 136, 72, seed=40 + mode, ldy_pad=4)
        wgrad_case(33, 8, 8, seed=42 + mode)


# ---- tn_direct: the mask einsum --------------------------------------------------------------------------------------------------
def tn_case(Mc, N, K, al, seed, grp=0, stats=False):
    """P[N, K] = A[Mc, N]^T X[Mc, K]; rows of X and P at `al` floats; grp: rows in groups of `grp` at a wide group stride;
    stats: the per-tile (x - shift) sums and sums of squares, stat_rows = 256 (two 128-row tiles in the first group, one in the second)"""
    g = torch.Generator().manual_seed(4000 + seed)
    what = f"tn_direct Mc={Mc} N={N} K={K} al={al} grp={grp} stats={stats}"
    a, x = rnd(g, Mc, N), rnd(g, Mc, K)
    A = Mat(a, N + 4)
    ldx, offx = (K, 1) if al == 1 else ((K + 3) // 4 * 4, 0)
    X = Mat(x, ldx, offx)
    ldo = K + 2 if al == 1 else (K + 3) // 4 * 4 + 4
    ref = a.double().T @ x.double()
    mag = a.double().abs().T @ x.double().abs()
    kw = dict(al_b=al, al_c=al)
    if grp:
        ngrp = N // grp
        grp_ld = grp * ldo + 3 * ldo + (1 if al == 1 else 0)       # a gap of three rows (and a float) between groups
        P = Mat(nan(ngrp, grp_ld), grp_ld, 1 if al == 1 else 0)
        kw.update(grp_rows=grp, grp_ld=grp_ld, ldc=ldo)
    else:
        P = Mat(nan(N, K), ldo, 1 if al == 1 else 0)
    keep = []
    if stats:
        tiles_k = (K + 127) // 128
        blk0, nblk = 2, 2 + 2 * tiles_k + 1
        sp = Mat(nan(1, 2 * nblk * 2))
        shift = Mat(torch.tensor([[0.37]]))
        keep += [sp, shift]
        kw.update(stat_part=sp.ptr, stat_shift=shift.ptr, stat_nblk=nblk, stat_blk0=blk0, stat_rows=256)
    gen = not (al == 4 and K % 4 == 0)
    v = call("tn_direct", Mc, N, K, A, X, P, tn_var(gen, 0, stats, grp > 0), what, **kw)
    if grp:
        got = torch.full((N, K), float("nan"), dtype=torch.float64)
        flat = P.buf.cpu()
        written = torch.zeros(flat.numel(), dtype=torch.bool)
        for n in range(N):
            s = P.off + (n // grp) * grp_ld + (n % grp) * ldo
            got[n] = flat[s:s + K].double()
            written[s:s + K] = True
        bad = (flat.view(torch.int32) != P.before.view(torch.int32)) & ~written
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} floats outside the output groups written"
    else:
        P.assert_guards()
        got = P.get()
    check(got, ref, mag, vclass(v), what)
    if stats:
        # the statistics are of the tile the kernel wrote: float64 sums of its own fp32 output, tile by tile
        raw = sp.buf.cpu().view(-1, 2)
        d = got - float(np.float32(0.37))
        written = set()
        for n0 in range(0, N, 128):
            grp_i, qt = n0 // 256, (n0 % 256) // 128
            for kt in range(tiles_k):
                slot = grp_i * nblk + blk0 + kt + tiles_k * qt
                written.add(slot)
                t = d[n0:n0 + 128, kt * 128:(kt + 1) * 128]
                s1, s2 = float(t.sum()), float((t * t).sum())
                assert abs(float(raw[slot, 0]) - s1) <= 2e-6 * float(t.abs().sum()), f"{what}: tile ({n0}, {kt}) sum {float(raw[slot, 0])} vs {s1}"
                assert abs(float(raw[slot, 1]) - s2) <= 2e-6 * s2, f"{what}: tile ({n0}, {kt}) sum of squares {float(raw[slot, 1])} vs {s2}"
        for slot in range(raw.shape[0]):
            if slot not in written:
                assert bool(torch.isnan(raw[slot]).all()), f"{what}: statistics slot {slot} written"


@pytest.mark.parametrize("K", [1075, 65_041])
@pytest.mark.parametrize("Mc", [128, 100, 1])
def test_tn_direct_unaligned_pixel_rows(Mc, K):
    tn_case(Mc, 132, K, 1, seed=Mc + K)


def test_tn_direct_aligned():
    tn_case(128, 132, 1024, 4, seed=1)
    tn_case(100, 4, 1076, 4, seed=2)


@pytest.mark.parametrize("K,al", [(1075, 1), (1024, 4)])
def test_tn_direct_grouped_rows(K, al):
    tn_case(128, 200, K, al, seed=3 + al, grp=100)


@pytest.mark.parametrize("K,al", [(1075, 1), (1024, 4)])
def test_tn_direct_tile_statistics(K, al):
    tn_case(128, 384, K, al, seed=5 + al, stats=True)


# ---- how the three-piece GEMM's error grows with the depth of the contraction ------------------------------------------------------------
# The element-wise bound above is per product: it scales with sum |a| |b| and says nothing about how the error of one accumulator grows
# with the number of fp32 additions into it (six MFMAs per 32-wide k-step, so 1152 at K = 6144, ConvNeXt-L's last pwconv2).  The
# backbones' tests hold every tensor to 8 x the error of a float32 restatement against float64 in max-norm; this is that bound on the
# GEMM alone, at the backbones' depths and epilogues.
DEEP_KS = (512, 2048, 3072, 4608, 6144)
DEEP_EPILOGUES = {"bias": 0, "gelu": 2, "relu_after_res": 4}      # name -> AxvsTestGemm::relu; every one carries a bias
DEEP_M, DEEP_N = 130, 160      # a part tile in both directions; 20800 elements
FLOOR = 2.0 ** -24             # one float32 rounding relative to the tensor's largest value (attention_edge_cases.bound)


def deep_case(K, epi, operand):
    """C = epilogue(A B^T + bias) through the forward dispatch with three pieces.  A ~ N(0, 1) ("normal") or gelu(1.5 N(0, 1)) ("hidden":
    the one-sided mean of a hidden activation), B ~ N(0, 1 / K).  -> (max |C - C64|, the bound, the float32 operation's own error)"""
    relu = DEEP_EPILOGUES[epi]
    g = torch.Generator().manual_seed(5000 + K + 7 * relu + (operand == "hidden"))
    M, N = DEEP_M, DEEP_N
    a = rnd(g, M, K)
    if operand == "hidden":
        a = torch.nn.functional.gelu(1.5 * a)
    b, bv = rnd(g, N, K, scale=K ** -0.5), rnd(g, N, scale=0.1)
    r = rnd(g, M, N) if relu == 4 else None
    what = f"deep fwd M={M} N={N} K={K} epilogue={epi} A={operand}"

    def op(a_, b_, bv_, r_):      # the same operation in the operands' type
        y = torch.nn.functional.linear(a_, b_, bv_)
        if relu == 2:
            return torch.nn.functional.gelu(y)
        return torch.relu(y + r_) if relu == 4 else y
    ref = op(a.double(), b.double(), bv.double(), r.double() if relu == 4 else None)
    own = op(a, b, bv, r).double()
    mag = a.double().abs() @ b.double().abs().T + bv.double().abs()
    if relu == 2:
        mag = GELU_SLOPE * mag
    A, B, Bv, Cm = Mat(a), Mat(b), Mat(bv.reshape(1, N)), Mat(nan(M, N))
    kw = dict(exact=1, relu=relu, bias=Bv.ptr)
    if relu == 4:
        R = Mat(r)
        kw["res"] = R.ptr
        mag = mag + r.double().abs()      # (a ReLU does not enlarge an error)
    v = call("fwd", M, N, K, A, B, Cm, nt_var(3, act=relu > 1, sum_=deep(K)), what, **kw)
    Cm.assert_guards()
    for m in (A, B, Bv):
        m.assert_guards(written=False)
    out = Cm.get()
    check(out, ref, mag, vclass(v), what)
    e, e32, top = float((out - ref).abs().max()), float((own - ref).abs().max()), float(ref.abs().max())
    floor = e32 < FLOOR * top
    bound = 8 * (FLOOR * top if floor else e32)
    print(f"[deep-gemm] K={K} {epi} A={operand}: max |device - float64| {e:.3e}, float32 on the CPU {e32:.3e}{' (below one rounding: floor)' if floor else ''}, "
          f"bound {bound:.3e}, ratio to the float32 error {8 * e / bound:.2f}")
    return e, bound, e32


@pytest.mark.parametrize("epi", list(DEEP_EPILOGUES))
@pytest.mark.parametrize("K", DEEP_KS)
def test_deep_contraction_error_growth(K, epi):
    """The three-piece forward GEMM at the backbones' contraction depths (ConvNeXt-L's pwconv2: 3072 and 6144; its downsample layers: up to
    3072; R-50's 1x1 convolutions: up to 2048) and with their three epilogues, so on both three-piece 16-byte instantiations: besides the
    element-wise bound, max |C - C64| <= 8 x the max-norm error of the same operation in float32 on the CPU (8 x 2^-24 max |C64| where
    that error is below one rounding).  The printed ratios per K are the growth curve (profiles/deep_contraction_parity.txt)."""
    got = {operand: deep_case(K, epi, operand) for operand in ("normal", "hidden")}      # (every figure is printed before any is held to its bound)
    for operand, (e, bound, _) in got.items():
        assert e <= bound, f"K={K} {epi} A={operand}: {e:.3e} > {bound:.3e}"


# ---- the bounds discriminate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4])
def test_bounds_reject_the_next_coarser_arithmetic(K):
    """The same inputs in every class: each bound rejects the next coarser arithmetic, by at least 4x at this K."""
    r = {}
    TOL_SAVED = dict(TOL)
    try:
        for k in TOL:
            TOL[k] = float("inf")          # measure only: the ratios are compared below
        r["ns3"] = nt_case(128, 128, K, 1, seed=77)
        r["ns2"] = nt_case(128, 128, K, 0, seed=77)
        with amp(2):
            r["f16"] = nt_case(128, 128, K, 1, seed=77)
        with amp(1):
            r["bf16"] = nt_case(128, 128, K, 1, seed=77)
    finally:
        TOL.update(TOL_SAVED)
    print(f"\n[train-gemm] K={K} worst ratios on identical inputs:", {k: f"{v:.3e}" for k, v in r.items()})
    for cls in r:
        assert r[cls] <= TOL[cls], (cls, r, TOL)
    for fine, coarse in (("ns3", "ns2"), ("ns2", "f16"), ("ns2", "bf16"), ("f16", "bf16")):
        assert r[coarse] > TOL[fine], f"the {fine} bound {TOL[fine]:.1e} accepts {coarse} arithmetic ({r[coarse]:.3e})"
    assert r["ns2"] >= 4 * r["ns3"] and r["bf16"] >= 4 * r["ns2"], r


# ---- coverage of the instantiations and of the dispatch rules --------------------------------------------------------------------
def test_zz_every_registered_instantiation_was_launched_by_its_rule():
    """Last in the file: every instantiation Gemm::init registers was launched, and every call of the file launched the one the
    dispatch rules document (K % 4 != 0 or unaligned rows -> GEN; an addend without GEN -> ADD; AMP -> one piece whatever `exact`, F16
    iff fp16; the affine loader -> two pieces; relu = 2 / 3 -> ACT; three pieces past 64 k-steps -> SUM; wgrad -> the 16-byte tn loader; tn_direct -> GEN unless 16-byte rows and K % 4 == 0).
    Small calls of each rule run here too, so the test stands alone when the file is run in part."""
    nt_case(1, 4, 4, 1, seed=90)
    nt_case(1, 4, 4, 0, seed=89)
    nt_case(1, 4, 3, 0, seed=91, a2=True)
    nt_case(1, 4, 4, 0, seed=92, a2=True)
    nt_case(1, 4, 4, 1, seed=93, a2=True)
    nt_case(1, 4, 4, 1, seed=94, al_a=1)
    nt_case(1, 4, 4, 0, seed=95, aff_rows=1)
    nt_case(1, 4, 5, 1, seed=96, aff_rows=1)
    nt_case(1, 4, 4, 1, seed=107, gelu=2)
    nt_case(1, 4, 2080, 1, seed=108)                 # 65 k-steps: the step sums, on each loader and with the GELU epilogue
    nt_case(1, 4, 2049, 1, seed=109)
    nt_case(1, 4, 2080, 1, seed=110, a2=True)
    nt_case(1, 4, 2080, 1, seed=111, gelu=3, res=True)
    for mode in (1, 2):
        with amp(mode):
            nt_case(1, 4, 4, 1, seed=97)
            nt_case(1, 4, 4, 0, seed=98, a2=True)
            nt_case(1, 4, 4, 1, seed=99, al_b=2, a2=True)
            wgrad_case(1, 8, 8, seed=100)
    wgrad_case(1, 8, 8, seed=101)
    tn_case(1, 4, 7, 1, seed=102)
    tn_case(1, 128, 1024, 4, seed=103, grp=64)
    tn_case(1, 128, 7, 1, seed=104, grp=64)
    tn_case(1, 128, 128, 4, seed=105, stats=True)
    tn_case(1, 128, 9, 1, seed=106, stats=True)
    wrong = [(vname(v), vname(e), w) for v, e, w in SEEN if v != e]
    assert not wrong, wrong[:5]
    reached = {v for v, _, _ in SEEN}
    want = registered()
    assert len(want) == 27, sorted(map(vname, want))
    missing = sorted(map(vname, want - reached))
    assert not missing, f"registered but never launched: {missing}"
    assert reached <= want, f"launched but not registered: {sorted(map(vname, reached - want))}"
    print("\n[train-gemm] instantiations reached:", " ".join(sorted(map(vname, reached))))
    print("[train-gemm] worst |C - C64| / magnitude:", {k: f"{v:.3e}" for k, v in MEASURED.items()}, "bounds:", TOL)
