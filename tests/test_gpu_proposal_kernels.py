"""Device: the proposal layer's kernels one at a time -- every cell of tests/proposal_cell_cases.py, every stage against the oracle operation on the
device's previous tensor (ctpn_debug_proposal_fetch), the sort alone on raw keys (ctpn_debug_sort_keys), batches against their images alone and one
ctx through a sequence of calls against fresh ones.

Exact: decode x1 / x2, the keep flag and key (recomputed from the device's boxes4), the sorted keys, everything the gather writes over the valid
ranks, keep lists (oracle NMS predicate on the device's sorted boxes), rois, anchors, the multi-workgroup NMS's scratch (zero after every call).
Decode y1 / y2 are the float32 restatement's bits for an exp at most one float away from float32(exp(float64(dh))) -- measured: 0 or 1 on every
anchor of every cell -- and so inside 0.5 (ulp(exp) x height + ulp(pred_h)) + ulp(y) (proposal_cells.decode_ref; the shorter form 0.5 ulp(pred_h) +
ulp(y) is passed 1.33-fold on the 2 x 256 map with exp one ulp off: one ulp of exp is up to two of pred_h). Per cell: profiles/proposal_kernel_cells.txt. Every call of the table runs with nms_check = 1, which must stay silent."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import proposal_cells as C
from proposal_cell_cases import CASES

pytestmark = pytest.mark.gpu
FETCHED = ("boxes4", "sorted_keys", "sorted_boxes", "sorted_scores", "sorted_anchor", "valid_counts", "keep_idx", "keep_counts", "mw_scratch")
BY_NAME = {c.name: c for _, c in CASES}


def _call(ctx, c, inputs=None):
    """one ctpn_proposals_from_host call of case c on ctx -> the dict proposal_cells.check_stages reads"""
    cls, bbox, info = C.case_inputs(c) if inputs is None else inputs
    n = cls.shape[0]
    rois, anchors = ctx.proposals_from_host(cls, bbox, info, c.pre, c.post, c.thresh, c.min_size, want_anchors=True)
    got = {k: ctx.proposal_fetch(k, n, c.hf, c.wf, c.pre, c.post) for k in FETCHED}
    plan = B.proposal_plan(n, c.hf, c.wf, pre=c.pre, post=c.post, thresh=c.thresh, nms_columns=ctx.get_option("nms_columns"),
                           nms_prefix=ctx.get_option("nms_prefix"), im_widths=info[:, 1])
    if plan.nms == "groups":
        got["colid"] = ctx.proposal_fetch("colid", n, c.hf, c.wf, c.pre, c.post)
    got["keep"] = [got["keep_idx"][i, : got["keep_counts"][i]] for i in range(n)]
    got["rois"], got["anchors"] = rois, anchors
    return got


def _fresh(c, inputs=None, check=1, **options):
    n = c.n if inputs is None else inputs[0].shape[0]
    opts = {"nms_columns": c.cols, "nms_prefix": c.prefix, "nms_check": check}
    opts.update(options)
    with ctpn_amd.Context(0, n, c.hf * 16, c.wf * 16, postproc_only=True, options=opts) as ctx:
        return _call(ctx, c, inputs)


def _valid_bytes(got, i):
    """what a call defines of image i, as bytes (rows of the sorted tensors behind valid_counts are stale)"""
    v = int(got["valid_counts"][i])
    parts = [got["boxes4"][i], got["sorted_keys"][i], got["sorted_boxes"][i][:v], got["sorted_scores"][i][:v], got["sorted_anchor"][i][:v],
             got["valid_counts"][i], got["keep"][i], got["rois"][i], got["anchors"][i]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


@pytest.mark.parametrize("cell,case", CASES, ids=[c.name for _, c in CASES])
def test_cell_stage_by_stage(cell, case):
    report = []
    got = _fresh(case)
    try:
        C.check_stages(case, got, report)
    finally:
        for name, i, ratio, ulps, off in report:
            print("CELL %-40s %-34s image %2d  decode y: %.3f of its bound, exp off by <= %d ulp on %d of %d anchors"
                  % (cell, name, i, ratio, ulps, off, case.hf * case.wf * 10))


FORM_CASES = ("kept_60x3_groups", "kept_100x2_groups", "kept_mid_groups", "tall_groups_12000", "tall_groups_4097", "pre_7000", "info_zero", "sort_4100_edge",
              "nms_1020", "sort_4130_all_valid", "batch_32")


@pytest.mark.parametrize("name", FORM_CASES)
def test_every_form_gives_the_same_bytes(name):
    c = BY_NAME[name]
    forms = {}
    for cols in (0, 1, 2, 3):
        for prefix in (0, 1):
            got = _fresh(c, check=1 if cols else 0, nms_columns=cols, nms_prefix=prefix)
            plan = B.proposal_plan(c.n, c.hf, c.wf, pre=c.pre, post=c.post, thresh=c.thresh, nms_columns=cols, nms_prefix=prefix,
                                   im_widths=C.case_inputs(c)[2][:, 1])
            forms[(plan.sort, plan.nms, plan.prefix)] = b"".join(_valid_bytes(got, i) for i in range(c.n))
            assert not got["mw_scratch"].any()
    assert len(forms) >= 3 and len(set(forms.values())) == 1, sorted(forms)


# ---- the sort alone ---------------------------------------------------------------------------------------------
SORT_PER_IMG = (1, 10, 64, 960, 961, 4080, 4096, 4097, 4098, 4099, 4100, 4130, 5120, 32760, 32768, 32770)


def _raw_keys(recipe, n_img, per_img):
    rng = np.random.default_rng(per_img * 8 + n_img)
    hi = rng.integers(0, 0xFFFFFFFF, (n_img, per_img), dtype=np.uint64)          # every digit value in all four score bytes; never the invalid word
    if recipe == "digits":
        hi[:, ::7] &= np.uint64(0xFF0000FF)
        hi[:, 1::5] = np.uint64(0xFFFFFFFE)
    elif recipe == "sorted":
        hi = np.sort(hi, axis=1)
    elif recipe == "reversed":
        hi = np.sort(hi, axis=1)[:, ::-1]
    elif recipe == "one_valid":                                                 # one valid key, somewhere; the rest is the invalid tail's ties
        pos = rng.integers(0, per_img, n_img)
        keys = np.full((n_img, per_img), C.KEY_INVALID, np.uint64)
        keys[np.arange(n_img), pos] = (hi[np.arange(n_img), pos] << np.uint64(32)) | pos.astype(np.uint64)
        return keys
    elif recipe == "invalid_runs":                                              # invalid keys in every segment, valid ones between them
        keys = (hi << np.uint64(32)) | np.arange(per_img, dtype=np.uint64)
        keys[:, rng.random(per_img) < 0.4] = C.KEY_INVALID
        return keys
    return (np.ascontiguousarray(hi) << np.uint64(32)) | np.arange(per_img, dtype=np.uint64)


@pytest.mark.parametrize("per_img", SORT_PER_IMG)
def test_sort_alone_on_raw_keys(per_img):
    """launch_sort_keys on keys the layer cannot produce; both forms where both exist, and the same bytes from them. (The segmented form's last
    segment cannot be shorter than 65 keys -- per_img 4097, then 66, 67: one key, two, three behind a full wave, not multiples of MG_SP.)"""
    npad = C.next_pow2(per_img)
    for n_img in (1, 3):
        for recipe in ("digits", "sorted", "reversed", "one_valid", "invalid_runs"):
            keys = _raw_keys(recipe, n_img, per_img)
            want = np.sort(keys, axis=1)
            one = B.debug_sort_keys(keys, False)
            assert np.array_equal(one[:, :per_img], want), (recipe, n_img, "one workgroup")
            assert np.all(one[:, per_img:] == np.uint64(B.SORT_POISON)), (recipe, n_img, "one workgroup: wrote behind the image's keys")
            if 4096 < per_img <= 32768:
                seg = B.debug_sort_keys(keys, True)
                assert np.array_equal(seg[:, :per_img], want), (recipe, n_img, "segmented", np.argwhere(seg[:, :per_img] != want)[:3])
                assert np.all(seg[:, per_img:] == C.KEY_INVALID), (recipe, n_img, "segmented: the merged buffer's padding")
                assert seg[:, :per_img].tobytes() == one[:, :per_img].tobytes()
    assert npad >= per_img


def test_sort_hook_refuses_the_segmented_form_outside_its_domain():
    for n_img, per_img in ((1, 4096), (1, 32769), (5, 5000), (1, 10)):
        with pytest.raises(B.CtpnError) as e:
            B.debug_sort_keys(np.zeros((n_img, per_img), np.uint64), True)
        assert e.value.code == -1


def test_negative_zero_ranks_behind_positive_zero_on_the_device():
    """pinned outside the oracle comparison (the oracle calls -0.0 and +0.0 a tie): the key orders the bits"""
    c = C.Case("neg_zero", 1, 2, 3, 12000, 1000, 0.7, 8.0, 1, 1, "uniform", "tall", "same")
    cls, bbox, info = (a.copy() for a in C.case_inputs(c))
    s = cls.reshape(-1, 2)
    s[:, 1] = np.where(np.arange(s.shape[0]) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    s[7, 1] = 0.5
    got = _fresh(c, (cls, bbox, info), check=0)
    keys = C.keys_ref(got["boxes4"][0], s[:, 1], info[0], c.min_size)
    assert np.array_equal(got["sorted_keys"][0], C.sort_ref(keys, 64))
    anchors = got["sorted_anchor"][0][: got["valid_counts"][0]]
    assert got["valid_counts"][0] == 60 and anchors[0] == 7
    assert np.all(anchors[1:30] % 2 == 1) and np.all(np.diff(anchors[1:30]) > 0) and np.all(anchors[30:] % 2 == 0)
    assert np.array_equal(got["sorted_scores"][0][:60].view(np.uint32), s[anchors, 1].view(np.uint32))


# ---- batches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sort_n4_seg", "sort_n5_one", "batch_8", "batch_32", "batch_32_groups", "info_zero", "info_narrow"])
def test_image_of_a_batch_equals_the_image_alone(name):
    """images that differ in h, w and scale: decode_kernel's per-image im_info selects (kernel arguments up to four images, the device copy above)"""
    c = BY_NAME[name]
    cls, bbox, info = C.case_inputs(c)
    batch = _fresh(c)
    for i in range(c.n):
        alone = _fresh(c, (cls[i: i + 1], bbox[i: i + 1], info[i: i + 1]))
        assert _valid_bytes(alone, 0) == _valid_bytes(batch, i), "image %d" % i


# ---- one ctx through a sequence of calls ------------------------------------------------------------------------------
def test_one_ctx_through_a_sequence_of_calls_equals_fresh_ones():
    """What a call leaves behind for the next: the multi-workgroup NMS's mask, ticket and flag word, keys_tmp behind a smaller map's keys, the
    sorted tensors' stale rows, the dirty mark of an error return and of an option change."""
    full = C.Case("state_full_map", 1, 64, 50, 12000, 1000, 0.7, 8.0, 1, 1, "uniform", "normal", "same")
    seq = [full, BY_NAME["sort_4100_edge"], BY_NAME["tall_groups_12000"], BY_NAME["post_below"], "refused", BY_NAME["sort_n4_seg"], BY_NAME["sort_4130_odd"],
           ("nms_columns", 3), BY_NAME["batch_8"]._replace(n=4, name="state_cols3"), ("nms_columns", 1), BY_NAME["kept_60x3_groups"], full]
    with ctpn_amd.Context(0, 4, 64 * 16, 50 * 16, postproc_only=True, options={"nms_columns": 1, "nms_prefix": 1}) as ctx:
        for step in seq:
            if step == "refused":
                c = BY_NAME["post_below"]
                with pytest.raises(B.CtpnError) as e:
                    _call(ctx, c._replace(pre=12001))
                assert e.value.code == B.CTPN_ERR_CAPACITY
                continue
            if not isinstance(step, C.Case):
                ctx.set_option(*step)
                continue
            got = _call(ctx, step)
            ref = _fresh(step, check=0, nms_columns=ctx.get_option("nms_columns"), nms_prefix=1)
            for i in range(step.n):
                assert _valid_bytes(got, i) == _valid_bytes(ref, i), "%s image %d" % (step.name, i)
            assert not got["mw_scratch"].any(), step.name


def test_fetch_hook_errors():
    c = BY_NAME["sort_3x5_differ"]
    with ctpn_amd.Context(0, 3, c.hf * 16, c.wf * 16, postproc_only=True, options={"nms_columns": 2}) as ctx:
        with pytest.raises(B.CtpnError) as e:
            ctx.proposal_fetch("boxes4", c.n, c.hf, c.wf, c.pre, c.post)
        assert e.value.code == -3                                   # no call yet
        _call(ctx, c)
        with pytest.raises(B.CtpnError) as e:
            ctx.proposal_fetch("colid", c.n, c.hf, c.wf, c.pre, c.post)
        assert e.value.code == -3                                   # the one-workgroup form writes no column ids
        with pytest.raises(B.CtpnError) as e:
            ctx.proposal_fetch("boxes4", c.n, c.hf, c.wf - 1, c.pre, c.post)
        assert e.value.code == B.CTPN_ERR_CAPACITY
