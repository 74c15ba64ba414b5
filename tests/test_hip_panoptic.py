"""GPU: video panoptic post-processing (axial_vs_amd.video_panoptic_inference) against the float64 restatement of the reference's two
functions and against the reference's stored results (tests/panoptic_cases.py, fixtures tests/golden/g20_panoptic_*.npz).

The outputs are discrete and compared EXACTLY: the cases are screened (tests/test_panoptic_cpu.py) so that no decision lies within 8x
the reference's own fp32 error of its threshold."""
import pytest
import torch

import __graft_entry__ as ge
import axial_vs_amd.panoptic  # noqa: F401  (the module under test)
import panoptic_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def _name(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


def _run(c, inputs, sf, setting, dtype=torch.float32, **kw):
    import axial_vs_amd as ax
    mp, cls, emb = inputs
    things, stuff = pc.ids_of(c[6])
    thr, ov, ct, cs, rc, rm = setting
    post = ax.VideoPanopticPostProcessor(things, stuff, pc.LABEL_DIVISOR, ct, cs, thr, ov, rc, rm)
    g = pc.geometry(c, sf)
    return post(cls.cuda(), mp.cuda().to(dtype), emb.cuda(), g.ac, g.image_h, g.image_w, g.sf, g.scaled_h, g.scaled_w, g.height, g.width, **kw)


def _check_dict(d, ref):
    assert list(d) == list(ref) and [len(v) for v in d.values()] == [len(v) for v in ref.values()]
    for v, r in zip(d.values(), ref.values()):
        assert float((torch.stack(v).double().cpu() - torch.stack(r).double()).abs().max()) <= 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=_name)
@pytest.mark.parametrize("sf", pc.SCALES, ids=lambda v: f"sf{v}")
@pytest.mark.parametrize("c", pc.CASES, ids=_name)
def test_map_tables_and_dict_equal_the_float64_restatement(c, sf, dtype):
    """for every setting: the device map equals the float64 restatement at EVERY pixel; the slot tables (final id, merge rank, class
    label, exact area per slot; the accepted things in acceptance order) equal it; the dict has its keys in order, its list lengths
    and its embeddings to 1e-6"""
    N = c[0]
    for setting in pc.SETTINGS:
        m64, d64, i64 = pc.restated(c, sf, setting)
        seg, d = _run(c, pc.inputs_of(c), sf, setting, dtype)
        assert seg.dtype == torch.int32 and seg.is_cuda and seg.shape == m64.shape
        wrong = int((seg.cpu() != m64).sum())
        print(f"[panoptic] {pc.case_name(c)} sf={sf} {setting} {_name(dtype)}: {wrong} of {m64.numel()} pixels differ from float64")
        assert wrong == 0
        _check_dict(d, d64)
        _, tb = _run(c, pc.inputs_of(c), sf, setting, dtype, return_tables=True)
        tb = {k: v.cpu() for k, v in tb.items()}
        assert torch.equal(tb["area"].long(), i64.area) and torch.equal(tb["label"].long(), i64.labels)
        assert torch.equal(tb["final_id"].long(), i64.final_id)
        rank = torch.empty(N, dtype=torch.long)
        rank[i64.order] = torch.arange(N)
        assert torch.equal(tb["rank"].long(), rank)
        n = len(i64.things)
        assert tb["counts"].tolist() == [n, i64.segments, int(((i64.scores > setting[0]).sum(0) >= 2).sum()), 0]
        got = list(zip(tb["thing_slot"][:n].tolist(), tb["thing_category"][:n].tolist(), tb["thing_ii"][:n].tolist()))
        assert got == i64.things and bool((tb["thing_slot"][n:] == -1).all())
        assert float((tb["class_score"].double() - i64.cls_scores).abs().max()) <= 1e-6
        assert float((tb["reorder_score"].double() - i64.reorder).abs().max()) <= 1e-5


@pytest.mark.parametrize("c", pc.FIXTURE_CASES, ids=_name)
def test_fixtures_match_exactly(c):
    """the reference's own results (its two methods run in fp32 on the CPU): the map exactly, the dict's keys, lengths and embeddings"""
    meta, inputs, ref = pc.load_fixture(c)
    for sf in pc.SCALES:
        for ti, setting in enumerate(pc.SETTINGS):
            rm, keys, embs = ref[(sf, ti)]
            seg, d = _run(c, inputs, sf, setting)
            assert torch.equal(seg.cpu(), rm), (sf, ti)
            _check_dict(d, {k: list(e) for k, e in zip(keys, embs)})


def test_two_runs_are_bit_equal():
    c = pc.MULTI_WG
    for sf in pc.SCALES:
        a, ta = _run(c, pc.inputs_of(c), sf, pc.SETTINGS[1], return_tables=True)
        b, tb = _run(c, pc.inputs_of(c), sf, pc.SETTINGS[1], return_tables=True)
        assert torch.equal(a, b)
        for k in ta:
            assert torch.equal(ta[k].view(torch.int32), tb[k].view(torch.int32)), k


def test_bf16_logits_against_float64_on_the_rounded_values():
    """bf16 input: the stored logits rounded to bf16 are other numbers, so the float64 restatement is taken on the rounded values and
    the comparison is made at the pixels whose decision is clear there (no score within 8x the fp32 error of the threshold)"""
    c, sf, setting = pc.CASES[1], 1.0, pc.SETTINGS[1]
    mp, cls, emb = pc.inputs_of(c)
    rounded = (mp.bfloat16().float(), cls, emb)
    _, tb = _run(c, rounded, sf, setting, torch.bfloat16, return_tables=True)
    _, _, i64 = pc.restate(c, rounded, sf, setting)
    _, _, i32 = pc.restate(c, rounded, sf, setting, torch.float32)
    band = 8.0 * float((i32.scores.double() - i64.scores).abs().max())
    if not bool(((i64.scores - setting[0]).abs() <= band).any()):
        assert torch.equal(tb["area"].cpu().long(), i64.area)
    _, tf = _run(c, rounded, sf, setting, torch.float32, return_tables=True)
    for k in tb:
        assert torch.equal(tb[k].view(torch.int32), tf[k].view(torch.int32)), k      # the same values as fp32 input: the same bits out


def test_return_tables_does_not_synchronise():
    c = pc.CASES[2]
    args = (c, pc.inputs_of(c), 0.7, pc.SETTINGS[0])
    ref, _ = _run(*args)
    import axial_vs_amd as ax
    mp, cls, emb = (x.cuda() for x in pc.inputs_of(c))
    things, stuff = pc.ids_of(c[6])
    thr, ov, ct, cs, rc, rm = pc.SETTINGS[0]
    post = ax.VideoPanopticPostProcessor(things, stuff, pc.LABEL_DIVISOR, ct, cs, thr, ov, rc, rm)
    g = pc.geometry(c, 0.7)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        seg, tb = post(cls, mp, emb, g.ac, g.image_h, g.image_w, g.sf, g.scaled_h, g.scaled_w, g.height, g.width, return_tables=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(seg, ref) and int(tb["counts"][1]) > 0


def test_peak_memory_of_the_multi_workgroup_case():
    """peak allocation during the call, beyond the inputs and the output map: at most 8 bytes per output pixel + 16 MiB (the
    reference's composition holds the fp32 scores and the mask product: at least 8 N bytes per pixel)"""
    import axial_vs_amd as ax
    from axial_vs_amd import modules
    c = pc.MULTI_WG
    mp, cls, emb = (x.cuda() for x in pc.inputs_of(c))
    things, stuff = pc.ids_of(c[6])
    thr, ov, ct, cs, rc, rm = pc.SETTINGS[0]
    post = ax.VideoPanopticPostProcessor(things, stuff, pc.LABEL_DIVISOR, ct, cs, thr, ov, rc, rm)
    g = pc.geometry(c, 0.7)
    modules._workspaces.clear()                     # the scratch buffer is allocated inside the measured call
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    seg, d = post(cls, mp, emb, g.ac, g.image_h, g.image_w, g.sf, g.scaled_h, g.scaled_w, g.height, g.width)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - seg.numel() * 4
    print(f"[panoptic] peak beyond inputs and map: {extra} bytes = {extra / seg.numel():.2f} per output pixel ({seg.numel()} pixels)")
    assert extra <= 8 * seg.numel() + (16 << 20)
    assert extra < 8 * c[0] * seg.numel() / 4       # and far below the reference's 8 N bytes per pixel
