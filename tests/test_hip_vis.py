"""GPU: video instance post-processing (axial_vs_amd.video_instance_inference) against the float64 restatement of the reference's op
sequence and against the reference's stored results (tests/vis_cases.py, fixtures tests/golden/g21_vis_*.npz).

The discrete outputs (masks, areas, boxes, candidates, selection) are compared EXACTLY: the cases are screened
(tests/test_vis_cpu.py) so that no decision lies within 8x the reference's own fp32 error of its threshold.  The scores are compared
within 8x the fp32 restatement's own error against float64, measured per case (the ratios printed here are kept in
profiles/vis_parity.txt)."""
import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import axial_vs_amd.instances  # noqa: F401  (the module under test)
import vis_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()
    assert torch.cuda.is_available()


def _name(v):
    return v.name if isinstance(v, vc.Case) else str(v).replace("torch.", "")


def _run(c, inputs, dtype=torch.float32, **kw):
    import axial_vs_amd as ax
    cls, mp = inputs
    return ax.video_instance_inference(cls.cuda(), mp.cuda().to(dtype), batch_input_shape=c.bi, img_shape=c.img, ori_shape=c.ori,
                                       num_things_classes=c.things, num_frames=c.F, max_per_image=c.K, keep_per_frame=c.Ko, **kw)


def _err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max()) if len(a) else 0.0


def _check(c, masks, tb, r64, r32, tag):
    """device results (numpy) against the float64 restatement `r64`; score bounds from the fp32 restatement `r32`"""
    n = len(r64.query)
    assert tb["counts"].tolist() == [n, len(set(r64.query.tolist()))]
    assert np.array_equal(tb["cand_query"][:n], r64.query.numpy()) and np.array_equal(tb["cand_label"][:n], r64.label.numpy())
    assert (tb["cand_query"][n:] == -1).all() and (tb["cand_label"][n:] == -1).all() and (tb["cand_cls_score"][n:] == -1).all()
    ref = dict(cls=_err(r32.cls_score, r64.cls_score), ms=max(_err(a.mask_score, b.mask_score) for a, b in zip(r32.frames, r64.frames)),
               det=max(_err(a.det_score, b.det_score) for a, b in zip(r32.frames, r64.frames)))
    dev = dict(cls=_err(tb["cand_cls_score"][:n], r64.cls_score), ms=0.0, det=0.0)
    cnt = min(n, c.Ko)
    assert masks.shape[:2] == (c.F, c.Ko) and masks.shape[2:] == tuple(c.ori)
    for t, f in enumerate(r64.frames):
        sel = f.sel.numpy()
        assert np.array_equal(tb["area"][t, :n], f.area.numpy()), (tag, t)
        assert np.array_equal(tb["cand_bbox"][t, :n], f.bbox.numpy()), (tag, t)
        assert np.array_equal(tb["bbox"][t, :cnt], f.bbox.numpy()[sel])
        wrong = int((masks[t, :cnt] != f.binary.numpy()[sel]).sum())
        assert wrong == 0, (tag, t, wrong)
        assert (tb["area"][t, n:] == -1).all() and (tb["det_score"][t, n:] == -1).all() and not masks[t, cnt:].any()
        assert tb["count"][t] == cnt and np.array_equal(tb["track_id"][t, :cnt], sel + 1)
        assert np.array_equal(tb["label"][t, :cnt], r64.label.numpy()[sel]) and np.array_equal(tb["query"][t, :cnt], r64.query.numpy()[sel])
        assert (tb["track_id"][t, cnt:] == -1).all() and (tb["score"][t, cnt:] == -1).all() and (tb["bbox"][t, cnt:] == -1).all()
        assert np.array_equal(tb["score"][t, :cnt], tb["det_score"][t, :n][sel])
        dev["ms"] = max(dev["ms"], _err(tb["mask_score"][t, :n], f.mask_score))
        dev["det"] = max(dev["det"], _err(tb["det_score"][t, :n], f.det_score))
    ratio = lambda k: f"{dev[k] / ref[k]:.2f}" if ref[k] > 0 else "-"
    print(f"[vis parity] {tag}: " + ", ".join(f"{k} {dev[k]:.2e} / fp32 restatement {ref[k]:.2e} = {ratio(k)}" for k in ("cls", "ms", "det")))
    for k in ("cls", "ms", "det"):
        assert dev[k] <= 8.0 * ref[k], (tag, k, dev[k], ref[k])


# every case with fp32 logits and with 16-bit logits of the type whose values it stores (fp16 values, or bf16 values in case b16)
_RUNS = [(c, d) for c in vc.CASES for d in (torch.float32, torch.bfloat16 if c.bf16 else torch.float16)]


@pytest.mark.parametrize("c,dtype", _RUNS, ids=[f"{c.name}-{_name(d)}" for c, d in _RUNS])
def test_masks_tables_and_selection_equal_the_float64_restatement(c, dtype):
    """masks at EVERY pixel, areas, boxes, the candidate list and each frame's selection equal the float64 restatement; class, mask and
    detection scores lie within 8x the fp32 restatement's own distance from float64 (the stored logits are values of the 16-bit type:
    both input types carry the same numbers).  Case b16 is case b's geometry on screened bf16 values; case h runs three tiles per
    workgroup; case k keeps its candidate keys in global memory."""
    masks, tb = _run(c, vc.inputs_of(c), dtype)
    _check(c, masks, tb, vc.restated(c), vc.restated(c, torch.float32), f"{c.name} {_name(dtype)}")


def test_bf16_and_fp32_loaders_give_the_same_bits():
    c = vc.BY_NAME["b16"]
    mb, tb = _run(c, vc.inputs_of(c), torch.bfloat16)
    mf, tf = _run(c, vc.inputs_of(c), torch.float32)
    assert np.array_equal(mb, mf)
    for k in tb:
        assert np.array_equal(tb[k].view(np.int32), tf[k].view(np.int32)), k


@pytest.mark.parametrize("c", [vc.BY_NAME[n] for n in "abeh"], ids=_name)
def test_bits_unpack_to_the_uint8_masks(c):
    import axial_vs_amd as ax
    m8, t8 = _run(c, vc.inputs_of(c))
    words, tw = _run(c, vc.inputs_of(c), mask_format="bits")
    W = c.ori[1]
    assert words.dtype == np.int64 and words.shape == (c.F, c.Ko, c.ori[0], (W + 63) // 64)
    assert np.array_equal(ax.unpack_bits(words, W), m8.astype(bool))
    if W % 64:
        assert not (words[..., -1].view(np.uint64) >> np.uint64(W % 64)).any()       # the bits past the row's end
    for k in t8:
        assert np.array_equal(t8[k].view(np.int32), tw[k].view(np.int32)), k
    dev_words, _ = _run(c, vc.inputs_of(c), mask_format="bits", return_tables=True)
    assert torch.equal(ax.unpack_bits(dev_words, W).cpu(), torch.from_numpy(m8.astype(bool)))


@pytest.mark.parametrize("c", vc.FIXTURE_CASES, ids=_name)
def test_fixtures_of_the_reference(c):
    """the reference's own results (its methods run in fp32 on the CPU), keyed by (query, label) since its candidate order is open: the
    rows with a non-zero score agree in rank, key, box and mask exactly and in score within 9x the fp32 error (8x for the device
    against float64, 1x for the reference itself); the remaining rows are empty masks on both sides"""
    meta, inputs, frames = vc.load_fixture(c)
    masks, tb = _run(c, inputs)
    r64, r32 = vc.restated(c), vc.restated(c, torch.float32)
    bound = 9.0 * max(_err(a.det_score, b.det_score) for a, b in zip(r32.frames, r64.frames))
    for t, ref in enumerate(frames):
        cnt = int(tb["count"][t])
        nz = int((ref.rows[:, 7] != 0).sum())
        m = min(cnt, nz)
        assert m > 0 and cnt == min(c.Ko, len(ref.rows))
        assert np.array_equal(tb["query"][t, :m], ref.rows[:m, 1]) and np.array_equal(tb["label"][t, :m], ref.rows[:m, 2])
        assert np.array_equal(tb["bbox"][t, :m], ref.rows[:m, 3:7])
        assert _err(tb["score"][t, :m], ref.rows[:m, 7]) <= bound
        assert np.array_equal(masks[t, :m].astype(bool), ref.masks[:m])
        assert not masks[t, m:].any() and not tb["bbox"][t, m:cnt].any() and not tb["score"][t, m:cnt].any()
        assert not ref.masks[nz:].any()


@pytest.mark.parametrize("c", vc.NUDGED, ids=_name)
def test_two_calls_are_bit_equal(c):
    a, ta = _run(c, vc.inputs_of(c), return_tables=True)
    b, tb = _run(c, vc.inputs_of(c), return_tables=True)
    assert torch.equal(a, b)
    for k in ta:
        assert torch.equal(ta[k].view(torch.int32), tb[k].view(torch.int32)), k      # fixed-point sums: the scores' bits too


def test_return_tables_does_not_synchronise():
    import axial_vs_amd as ax
    c = vc.BY_NAME["d"]
    ref, rt = _run(c, vc.inputs_of(c))
    cls, mp = (x.cuda() for x in vc.inputs_of(c))
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        masks, tb = ax.video_instance_inference(cls, mp, batch_input_shape=c.bi, img_shape=c.img, ori_shape=c.ori, num_things_classes=c.things,
                                                num_frames=c.F, max_per_image=c.K, keep_per_frame=c.Ko, return_tables=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert masks.is_cuda and all(v.is_cuda for v in tb.values())
    assert np.array_equal(masks.cpu().numpy(), ref) and np.array_equal(tb["track_id"].cpu().numpy(), rt["track_id"])


def test_post_processor_gives_the_reference_s_per_class_lists():
    """case c through `VideoInstancePostProcessor`: per frame `(bbox_results, mask_results)` as `TubeLinkVideoVIS.simple_test` holds them
    before `encode_mask_results` -- the fixture's rows per class (box exact, score within 9x the fp32 error, masks exact), the ids
    those of the float64 restatement"""
    import axial_vs_amd as ax
    c = vc.BY_NAME["c"]
    meta, inputs, frames = vc.load_fixture(c)
    cls, mp = (x.cuda() for x in inputs)
    post = ax.VideoInstancePostProcessor(c.things, c.K, c.Ko)
    metas = [[dict(batch_input_shape=c.bi, img_shape=c.img + (3,), ori_shape=c.ori + (3,)) for _ in range(c.F)]]
    results = post(cls[None], mp[None], metas, c.F)
    r64, r32 = vc.restated(c), vc.restated(c, torch.float32)
    bound = 9.0 * max(_err(a.det_score, b.det_score) for a, b in zip(r32.frames, r64.frames))
    assert len(results) == 1 and len(results[0]) == c.F
    for t, ref in enumerate(frames):
        bbox_results, mask_results = results[0][t]["ins_results"]
        assert len(bbox_results) == len(mask_results) == c.things and (ref.rows[:, 7] != 0).all()
        ids = (r64.frames[t].sel + 1).numpy()
        for k in range(c.things):
            rows = ref.rows[ref.rows[:, 2] == k]
            got = bbox_results[k]
            assert got.shape == (len(rows), 6) and got.dtype == np.float32 and len(mask_results[k]) == len(rows)
            assert np.array_equal(got[:, 0], ids[ref.rows[:, 2] == k]) and np.array_equal(got[:, 1:5], rows[:, 3:7])
            assert _err(got[:, 5], rows[:, 7]) <= bound
            for mine, theirs in zip(mask_results[k], ref.masks[ref.rows[:, 2] == k]):
                assert mine.dtype == bool and np.array_equal(mine, theirs)


def test_refusals_leave_the_library_usable():
    import axial_vs_amd as ax
    c = vc.BY_NAME["a"]
    cls, mp = vc.inputs_of(c)
    kw = dict(batch_input_shape=c.bi, img_shape=c.img, ori_shape=c.ori, num_things_classes=c.things)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ax.video_instance_inference(cls, mp, max_per_image=c.K, keep_per_frame=c.Ko, **kw)
    with pytest.raises(RuntimeError, match="512"):
        ax.video_instance_inference(torch.zeros(513, 3).cuda(), torch.zeros(1, 513, 4, 5).cuda(), max_per_image=4, keep_per_frame=3, **kw)
    with pytest.raises(RuntimeError, match="max_per_image"):
        ax.video_instance_inference(cls.cuda(), mp.cuda(), max_per_image=c.Q * c.C + 1, keep_per_frame=3, **kw)
    with pytest.raises(RuntimeError, match="keep_per_frame"):
        ax.video_instance_inference(cls.cuda(), mp.cuda(), max_per_image=4, keep_per_frame=5, **kw)
    masks, tb = _run(c, vc.inputs_of(c))
    _check(c, masks, tb, vc.restated(c), vc.restated(c, torch.float32), "a after refusals")
