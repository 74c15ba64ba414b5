"""GPU: the three eval-forward attention kernels (m2f_attn_kernel with m2f_attn_combine_kernel, kmax_attn_kernel,
kpix_axial_attn_kernel) and the mask head (m2f_logits_kernel) on the cases of tests/attention_edge_cases.py: attention masks built by
hand, the key-chunk cap, mask-head rows with one open key, and a softmax from uniform to almost one-hot.  Every number is compared with the
float64 restatement of the kernel's own case module within 8 x the float32 restatement's own max-norm error on the same inputs (at least
8 * 2^-24 * max|float64 output|), and must be finite; test_attention_edges_cpu.py shows that these bounds tell the wrong forms apart.

Measured on an MI355X (profiles/attention_edges_parity.txt): every compared tensor sits inside its bound."""
import os

import pytest
import torch

import __graft_entry__ as ge
import attention_edge_cases as ec
import m2f_decoder_cases as mc
from test_hip_kmax_decoder import make_decoder as make_kmax
from test_hip_kmax_pixel_decoder import make_decoder as make_kpix
from test_hip_m2f_decoder import make_decoder as make_m2f


@pytest.fixture(scope="session", autouse=True)
def built():
    ge.build()


_DEVICE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_state():
    """the decoders shared by this module's tests are dropped when its tests are done, so that tests which measure peak device memory see
    what they saw before"""
    yield
    _DEVICE.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def shared(key, make):
    if key not in _DEVICE:
        _DEVICE[key] = make()
    return _DEVICE[key]


def check(got, item, what, want=None):
    """device error, bound, ratio to the float32 restatement's error -- printed, then asserted"""
    want = item["want"] if want is None else want
    assert tuple(got.shape) == tuple(want.shape), what
    assert bool(torch.isfinite(got).all()), what
    e = ec.err(got, want)
    line = (f"{what}: device error {e:.3e}, float32 restatement {item['own']:.3e}, bound {item['tol']:.3e}, ratio {8 * e / item['tol']:.2f}"
            + (" (floor: the float32 restatement's error is below 2^-24 x the largest output)" if item["floor"] else ""))
    print(line)
    if os.environ.get("AXVS_WRITE_PARITY"):
        with open(os.environ["AXVS_WRITE_PARITY"], "a") as f:
            f.write(line + "\n")
    assert e <= item["tol"], what


# ---- A: hand-built masks --------------------------------------------------------------------------------------------------------------------------
def m2f_layer(dec, x_in, memory, masked, i):
    """layer i on float64 queries [Q,N,C] under `masked` [N,Q,S] -> [Q,N,C] on the host"""
    from axial_vs_amd.clip_decoder import pack_mask_bits
    bits = pack_mask_bits(masked).cuda()
    flags = (~masked.all(-1)).int().cuda()
    return dec.layer(x_in.transpose(0, 1).float().cuda(), memory, bits, flags, i).cpu().transpose(0, 1)


def case_e():
    def make():
        st = mc.study(mc.BY_NAME["e"])
        return st, make_m2f(st["case"], st["params"]), [m.cuda() for m in st["mems"]]
    return shared("m2f e", make)


@pytest.mark.gpu
@pytest.mark.parametrize("layer", [0, 1, 2])
def test_m2f_layer_under_hand_built_masks(layer):
    """Layers 0..2 of case e (24, 70 and 598 keys: the last in three chunks of 224, the third partial) on the float64 chain's queries.
    Rows whose keys are all masked attend to all keys: bit-equal to the rows of no mask at all."""
    st = ec.m2f_mask_study(layer)
    _, dec, mems = case_e()
    got = {}
    for name, it in st["items"].items():
        got[name] = m2f_layer(dec, st["x_in"], mems[layer % 3], it["masked"], layer)
        check(got[name], it, f"m2f layer {layer} ({st['S']} keys) mask {name}")
    assert torch.equal(got["all_masked"], got["all_open"])


@pytest.mark.gpu
def test_m2f_layer_at_the_key_chunk_cap():
    """16928 keys in one clip: past 64 x 256, where the key chunks grow instead of their number (59 chunks of 288, the last partial): one
    open key (the last key among them), one live chunk (the first, chunk 30, the last), and a seeded mask of one half."""
    st = ec.m2f_cap_study()
    dec = make_m2f(ec.CAP, st["params"])
    memory = st["mems"][0].cuda()
    for name, it in st["items"].items():
        check(m2f_layer(dec, st["x_in"], memory, it["masked"], 0), it, f"m2f cap ({st['S']} keys, {st['nchunk']} chunks of {st['chunk']}) mask {name}")


# ---- B: the mask head -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2])
def test_m2f_mask_head_on_sparse_rows(level):
    """Rows with one open key (key 0, the last key, the last word), none and all, every |logit| far outside the band: every bit equals
    float64's, the flags say "a key is open", bits past the row's end are zero."""
    from axial_vs_amd.clip_decoder import unpack_mask_bits
    st = ec.sparse_rows_study(level)
    base, dec, _ = case_e()
    S = st["S"]
    bits, flags = dec.attention_mask(st["x_in"].transpose(0, 1).float().cuda(), st["mf"].cuda(), base["case"].levels[level], level)
    got = unpack_mask_bits(bits, S).cpu()
    diff = got != st["masked"]
    print(f"m2f mask head level {level} ({S} keys): {int(diff.sum())} of {diff.numel()} bits differ; band {st['band']:.2e}, min |logit| {float(st['logits'].abs().min()):.4f}")
    assert not bool(diff.any())
    assert torch.equal(flags.cpu() != 0, (~st["masked"]).any(-1))
    assert bits.shape[-1] == (S + 31) // 32
    if S % 32:
        assert int((bits[..., -1].cpu().to(torch.int64) & 0xFFFFFFFF).bitwise_right_shift(S % 32).abs().max()) == 0


# ---- C: sharp and uniform softmax -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("g,a", ec.m2f_variants(), ids=lambda v: str(v))
@pytest.mark.parametrize("name", ec.M2F_SHARP_CASES)
def test_m2f_layer_sharp_and_uniform(name, g, a):
    """every layer of the case with float64's own bits, the scores of the cross-attention (a = 0) or the self-attention (a = 1) times g"""
    st = ec.m2f_sharp_study(name, g, a)
    base = st["st"]
    dec = make_m2f(base["case"], st["params"])
    mems = [m.cuda() for m in base["mems"]]
    for i, (l, it) in enumerate(zip(base["layers"], st["layers"])):
        check(m2f_layer(dec, l["x_in"], mems[i % 3], l["masked"], i), it, f"m2f case {name} g {g} attention {a} layer {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", ec.kmax_classes())
@pytest.mark.parametrize("name", ec.KMAX_SHARP_CASES)
def test_kmax_layer_sharp_and_uniform(name, cls):
    """layer 0 under the hand map p % L, the similarity norm's gain times g; class bias50: its bias + 50, which cancels in the softmax"""
    st = ec.kmax_sharp_study(name, cls)
    dec = make_kmax(st["case"], st["params"])
    got = dec.layer(st["q_in"].transpose(1, 2).float().contiguous().cuda(), st["x"].cuda(), st["index"].int().cuda(), 0)
    check(got, st, f"kmax case {name} class {cls}", st["want"].transpose(1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("g", ec.classes("kpix"))
@pytest.mark.parametrize("spec", ec.KPIX_SHARP_CASES, ids=lambda s: "x".join(map(str, s)))
def test_kpix_axial_attn_sharp_and_uniform(spec, g):
    """one axis pass of each axis on the float64 chain's qkv rows, the q channels times g (class 0: the similarity norms' gains at 0)"""
    st0 = ec.kpix_sharp_study(spec, g, 0)
    dec = shared(("kpix", spec, g == 0), lambda: make_kpix(st0["case"], st0["params"]))
    for axis in (0, 1):
        st = ec.kpix_sharp_study(spec, g, axis)
        check(dec.axial_attn(st["qkv"].float().contiguous().cuda(), 0, 0, axis), st, f"kpix {spec} g {g} axis {'hw'[axis]}")


@pytest.mark.gpu
@pytest.mark.parametrize("spec", ec.KPIX_SHARP_CASES, ids=lambda s: "x".join(map(str, s)))
def test_kpix_similarity_offsets_cancel(spec):
    """the similarity norm's bias and running mean only shift all scores of a row: the kernel takes the gains alone, bit for bit"""
    st = ec.kpix_sharp_study(spec, 1, 0)
    dec = shared(("kpix", spec, False), lambda: make_kpix(st["case"], st["params"]))
    moved = make_kpix(st["case"], ec.kpix_params(spec, "offsets"))
    for axis in (0, 1):
        for g in (1, ec.SHARP["kpix"]):
            qkv = ec.kpix_sharp_study(spec, g, axis)["qkv"].float().contiguous().cuda()
            assert torch.equal(moved.axial_attn(qkv, 0, 0, axis), dec.axial_attn(qkv, 0, 0, axis)), (axis, g)
