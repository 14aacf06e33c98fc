"""Device: decode_kernel's production branch alone (ctpn_debug_proposals_from_heads) -- the in-kernel pair softmax on chosen logits, the
head_ld = 64 addressing, the per-image im_info selects and their publication, the ragged filter -- on the cases of tests/decode_heads_cells.py.

Exact: rpn_bbox_pred (the rows' first 40 columns), ties (0.5), saturated pairs (1.0 / 0.0), NaN pairs, decode x1 / x2, the boxes of non-finite
deltas (fmaxf(fminf(v, lim), 0)), the keep flag and key (recomputed from the device's boxes and probabilities), im_info on the device. Every
other probability is the float32 restatement's bits for exponentials at most one float away from float32(exp(float64(s - mx))) -- measured:
profiles/decode_heads_cells.txt -- and so inside the interval of decode_heads_cells.softmax_interval. Behind the keys the branch is held by
equality of bytes with ctpn_proposals_from_host on the device's own probabilities, which tests/test_gpu_proposal_kernels.py checks stage by stage."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import decode_heads_cells as D
import ragged_ref as R
import util

pytestmark = pytest.mark.gpu
FETCHED = ("boxes4", "sorted_keys", "sorted_boxes", "sorted_scores", "sorted_anchor", "valid_counts", "keep_idx", "keep_counts", "mw_scratch", "im_info")


def _fetch(ctx, n, hf, wf, info, rois, anchors):
    got = {k: ctx.proposal_fetch(k, n, hf, wf, D.PRE, D.POST) for k in FETCHED}
    plan = B.proposal_plan(n, hf, wf, pre=D.PRE, post=D.POST, thresh=D.THRESH, nms_columns=ctx.get_option("nms_columns"),
                           nms_prefix=ctx.get_option("nms_prefix"), im_widths=info[:, 1])
    if plan.nms == "groups":
        got["colid"] = ctx.proposal_fetch("colid", n, hf, wf, D.PRE, D.POST)
    got["keep"] = [got["keep_idx"][i, : got["keep_counts"][i]] for i in range(n)]
    got["rois"], got["anchors"] = rois, anchors
    return got


def _heads_call(ctx, c, inputs=None):
    heads, info, vr = D.case_inputs(c)[:3] if inputs is None else inputs
    rois, anchors, cls, bbox = ctx.proposals_from_heads(heads, info, vr, D.PRE, D.POST, D.THRESH, c.min_size)
    got = _fetch(ctx, heads.shape[0], c.hf, c.wf, info, rois, anchors)
    got["cls_prob"], got["bbox_pred"] = cls, bbox
    return got


def _host_call(ctx, c, cls, bbox, info):
    rois, anchors = ctx.proposals_from_host(cls, bbox, info, D.PRE, D.POST, D.THRESH, c.min_size, want_anchors=True)
    return _fetch(ctx, cls.shape[0], c.hf, c.wf, info, rois, anchors)


def _ctx(n, hf, wf, **options):
    opts = {"nms_check": 1}
    opts.update(options)
    return ctpn_amd.Context(0, n, hf * 16, wf * 16, postproc_only=True, options=opts)


def _fresh(c, inputs=None, **options):
    with _ctx(c.n if inputs is None else inputs[0].shape[0], c.hf, c.wf, **options) as ctx:
        return _heads_call(ctx, c, inputs)


def _defined_bytes(got, i, colid=True):
    """what a call defines of image i, as bytes (rows of the sorted tensors behind valid_counts are stale; colid: only the multi-workgroup NMS
    writes column ids, and a batch and its images alone need not take the same form)"""
    v = int(got["valid_counts"][i])
    parts = [got["boxes4"][i], got["sorted_keys"][i], got["sorted_boxes"][i][:v], got["sorted_scores"][i][:v], got["sorted_anchor"][i][:v],
             got["valid_counts"][i], got["keep"][i], got["rois"][i], got["anchors"][i], got["im_info"][i], got["mw_scratch"][i]]
    if colid and "colid" in got:
        parts.append(got["colid"][i][:v])
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def _invalid_below(cls, vr):
    """the from-host side of a ragged call: the cells below an image are not the image's (ragged_ref: its valid rows at level 4) -- their fg
    probability becomes NaN, which the tested branch turns into KEY_INVALID"""
    out = cls.copy()
    if vr is not None:
        for i, v in enumerate(vr):
            out[i, int(v):, :, 1::2] = np.nan
    return out


@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_case_stage_by_stage(case):
    report = []
    got = _fresh(case)
    try:
        D.check(case, got, report)
    finally:
        for name, pairs, floats, off, frac, ulps in report:
            print("CASE %-18s n %d map %d x %d  %4d measured pairs: exp off by <= %d float on %d of them, |p - softmax64| at most %.3f of the interval, %.2f ulp of p"
                  % (name, case.n, case.hf, case.wf, pairs, floats, off, frac, ulps))
    assert not got["mw_scratch"].any()
    for i in range(case.n):
        assert len(got["rois"][i]) == got["keep_counts"][i] == len(got["anchors"][i])


@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_production_branch_equals_the_tested_branch_on_its_own_probabilities(case):
    heads, info, vr = D.case_inputs(case)[:3]
    prod = _fresh(case)
    if vr is not None:
        assert [R.valid_rows(int(h), 4) for h in info[:, 0]] == vr.tolist()      # im_info heights and feature rows belong together
    with _ctx(case.n, case.hf, case.wf) as ctx:
        host = _host_call(ctx, case, _invalid_below(prod["cls_prob"], vr), prod["bbox_pred"], info)
    for i in range(case.n):
        assert _defined_bytes(prod, i) == _defined_bytes(host, i), "%s image %d" % (case.name, i)
    assert ("colid" in prod) == ("colid" in host)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_every_image_is_decoded_on_its_own_im_info_row(n):
    """the four select arms (n <= 4) and the device copy (n = 5): the case's first n images, each against the image alone"""
    c = D.BY_NAME["five_device_rows"]
    heads, info, _ = D.case_inputs(c)[:3]
    sub = c._replace(n=n, name="first_%d_images" % n)
    batch = _fresh(sub, (heads[:n], info[:n], None))
    assert np.array_equal(batch["im_info"], info[:n])
    for i in range(n):
        want = D.decode_restated(heads[i, :, :, :40].reshape(-1, 4), info[i], c.hf, c.wf)
        assert np.array_equal(batch["boxes4"][i][:, 0::2], want[:, 0::2]), i
        fin = D.case_inputs(c)[4][i].reshape(-1) == 0
        ref4, tol, ys = D.C.decode_ref(np.where(fin[:, None], heads[i, :, :, :40].reshape(-1, 4), np.float32(0)).reshape(-1), info[i], c.hf, c.wf)
        assert D.C.exp_ulps_of(batch["boxes4"][i], ys)[fin].max() <= D.C.EXP_ULPS, i
        for j in range(n):                                       # ... and on no other image's row
            if j != i:
                other = D.decode_restated(heads[i, :, :, :40].reshape(-1, 4), info[j], c.hf, c.wf)
                assert not np.array_equal(batch["boxes4"][i][:, 0::2], other[:, 0::2]), (i, j)
        alone = _fresh(sub._replace(n=1), (heads[i: i + 1], info[i: i + 1], None))
        a, b = _defined_bytes(alone, 0, colid=False), _defined_bytes(batch, i, colid=False)
        assert a == b, "image %d" % i
        assert alone["cls_prob"][0].tobytes() == batch["cls_prob"][i].tobytes()


@pytest.fixture(scope="module")
def weights():
    return util.stress_arena("biased")


def _pad64(heads60):
    out = np.full(heads60.shape[:3] + (64,), np.nan, np.float32)
    out[..., :60] = heads60
    return out


def _hook_equals_production(ctx, info, vr):
    """ctx: behind a forward. ctpn_proposals on it, then the forward's heads through the hook on a post-processing ctx"""
    n, hf, wf = ctx.feat_shape()
    rois, anchors = ctx.proposals(info, D.PRE, D.POST, D.THRESH, 8.0, want_anchors=True)
    cls, bbox = ctx.get_tensor("rpn_cls_prob_reshape"), ctx.get_tensor("rpn_bbox_pred")
    heads = _pad64(ctx.get_tensor("heads"))
    assert heads.shape == (n, hf, wf, 64) and sum(len(r) for r in rois) > 0
    with ctpn_amd.Context(0, n, hf * 16, wf * 16, postproc_only=True) as post:
        rois2, anchors2, cls2, bbox2 = post.proposals_from_heads(heads, info, vr, D.PRE, D.POST, D.THRESH, 8.0)
    for i in range(n):
        assert rois[i].tobytes() == rois2[i].tobytes() and anchors[i].tobytes() == anchors2[i].tobytes(), i
    assert cls.tobytes() == cls2.tobytes() and bbox.tobytes() == bbox2.tobytes()


@pytest.mark.parametrize("n,h,w", [(1, 32, 48), (3, 48, 32)])
def test_the_hook_runs_what_production_runs(weights, n, h, w):
    imgs = ctpn_amd.weights.synthetic_images(n, h, w, 7)
    info = np.array([[h - 3 * i, w - 2 * i, (1.0, 1.5, 0.75)[i]] for i in range(n)], np.float32)
    with ctpn_amd.Context(0, n, h, w, "fp32") as ctx:
        ctx.load_weights(weights)
        ctx.forward(imgs)
        _hook_equals_production(ctx, info, None)


def test_the_hook_runs_what_production_runs_on_a_ragged_canvas(weights):
    canvas, heights = R.canvas_of(R.images(), R.HC)
    info = np.array([[h, R.W, 1.0] for h in heights], np.float32)
    vr = np.array([R.valid_rows(h, 4) for h in heights], np.int32)
    with ctpn_amd.Context(0, len(heights), R.HC, R.W, "fp32") as ctx:
        ctx.load_weights(weights)
        ctx.forward_ragged(canvas, heights)
        _hook_equals_production(ctx, info, vr)


def test_one_ctx_through_a_sequence_of_calls_equals_fresh_ones():
    """a heads call, a from-host call and a smaller heads call on one ctx: everything a call defines equals a fresh ctx's; the rows of
    cls_prob / bbox_pred behind a call's cells are stale and not looked at (the hook hands out the call's cells only)"""
    big, ragged, small = D.BY_NAME["seams_3x5x7"], D.BY_NAME["ragged_6_3_1"], D.BY_NAME["four_selects"]
    ref_ragged = _fresh(ragged)
    host_cls = _invalid_below(ref_ragged["cls_prob"], D.case_inputs(ragged)[2])
    with ctpn_amd.Context(0, 4, 6 * 16, 7 * 16, postproc_only=True, options={"nms_check": 1}) as ctx:
        for step in (big, "host", ragged, small, big):
            if step == "host":
                got = _host_call(ctx, ragged, host_cls, ref_ragged["bbox_pred"], D.case_inputs(ragged)[1])
                ref, c = ref_ragged, ragged
            else:
                got, ref, c = _heads_call(ctx, step), _fresh(step), step
                assert got["cls_prob"].tobytes() == ref["cls_prob"].tobytes() and got["bbox_pred"].tobytes() == ref["bbox_pred"].tobytes(), c.name
            for i in range(c.n):
                assert _defined_bytes(got, i) == _defined_bytes(ref, i), "%s image %d" % (c.name, i)


def test_hook_argument_checks():
    c = D.BY_NAME["four_selects"]
    heads, info, _ = D.case_inputs(c)[:3]
    with _ctx(2, c.hf, c.wf) as ctx:
        with pytest.raises(B.CtpnError) as e:
            ctx.proposals_from_heads(heads, info)                               # four images on a ctx for two
        assert e.value.code == B.CTPN_ERR_CAPACITY
        with pytest.raises(B.CtpnError) as e:
            ctx.proposals_from_heads(np.concatenate([heads[:1], heads[:1]], axis=1), info[:1])      # a taller map
        assert e.value.code == B.CTPN_ERR_CAPACITY
        with pytest.raises(B.CtpnError) as e:
            ctx.proposals_from_heads(heads[:1], info[:1], pre_nms_topn=12001)
        assert e.value.code == B.CTPN_ERR_CAPACITY
        rois, anchors, cls, bbox = ctx.proposals_from_heads(heads[:2], info[:2])
        assert cls.shape == (2, c.hf, c.wf, 20) and len(rois) == 2
