"""GPU: RPN_POST_NMS_TOP_N above 1000 -- ctpn_reserve_proposals, the proposal layer up to 4096 rows, the connector's NMS and the large
connector (connect_large_kernel) above 1024 rows, on the dense pages of tests/dense_pages.py; and that a ctx with a larger capacity returns
what a fresh one returns. tests/test_dense_pages.py holds the CPU side.

Tolerance against the oracle: the existing tests' -- proposals: scores equal, boxes within 1e-3 (exp() to the last ulp), anchors (the keep
list) exactly; lines: equal counts and order, scores bit-equal, coordinates within rtol 3e-7 / atol 1e-5. Device forms against each other and
against the host connector: byte-equal."""
import gc

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import dense_pages as D
import ragged_ref as R
import util

pytestmark = pytest.mark.gpu

COUNTS = (1000, 1001, 1024, 1025, 2047, 2048, 4095, 4096)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_close_to_oracle(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, 8], want[:, 8]), what
    assert np.allclose(got[:, :8], want[:, :8], rtol=3e-7, atol=1e-5), (what, np.abs(got - want).max())


# ---- refusals and reserve ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_reserve(arena):
    with ctpn_amd.Context(0, 2, 64, 96, "fp32") as c:
        c.load_weights(arena)
        assert c.proposal_capacity == 1000
        with pytest.raises(B.CtpnError) as e:
            c.set_param("RPN_POST_NMS_TOP_N", 1280)
        assert e.value.code == -1
        for bad in (999, 4097):
            with pytest.raises(B.CtpnError) as e:
                B._check(c._lib.ctpn_reserve_proposals(c._h, bad))
            assert e.value.code == -1
        assert c.proposal_capacity == 1000
        c.detect_submit(ctpn_amd.weights.synthetic_images(2, 64, 96, 3), slot=0)
        with pytest.raises(B.CtpnError) as e:
            c.reserve_proposals(4096)
        assert e.value.code == -3 and c.proposal_capacity == 1000
        c.detect_collect(0)
        c.reserve_proposals(4096)
        assert c.proposal_capacity == 4096
        c.set_param("RPN_POST_NMS_TOP_N", 1280)
        assert c.get_param("RPN_POST_NMS_TOP_N") == 1280
        with pytest.raises(B.CtpnError) as e:
            c.reserve_proposals(1000)                     # below the current parameter
        assert e.value.code == -1 and c.proposal_capacity == 4096
        with pytest.raises(B.CtpnError) as e:
            c.set_param("RPN_POST_NMS_TOP_N", 4097)
        assert e.value.code == -1
        c.set_param("RPN_POST_NMS_TOP_N", 1000)
        c.reserve_proposals(1000)
        assert c.proposal_capacity == 1000
        with pytest.raises(B.CtpnError):
            c.set_param("RPN_POST_NMS_TOP_N", 1001)


# ---- the proposal layer up to 4096 rows --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pctx():
    with ctpn_amd.Context(0, 5, 65 * 16, 64 * 16, postproc_only=True) as c:
        with pytest.raises(B.CtpnError) as e:            # a fresh ctx refuses 1001, as ever
            c.proposals_from_host(*D.page("24x48")[:2], D.page("24x48")[2].reshape(1, 3), post_nms_topn=1001)
        assert e.value.code == B.CTPN_ERR_CAPACITY
        c.reserve_proposals(4096)
        yield c


def run_pages(ctx, names, post=4096, **options):
    for k, v in options.items():
        ctx.set_option(k, v)
    cls = np.concatenate([D.page(n)[0] for n in names])
    box = np.concatenate([D.page(n)[1] for n in names])
    info = np.stack([D.page(n)[2] for n in names])
    return ctx.proposals_from_host(cls, box, info, post_nms_topn=post, want_anchors=True)


def check_pages(names, rois, anchors, post=4096):
    for i, n in enumerate(names):
        want = D.oracle_rois(n)[:post]
        assert anchors[i].shape[0] == want.shape[0] and np.array_equal(anchors[i], D.oracle_anchors(n)[:post]), n
        assert rois[i].shape == want.shape and np.array_equal(rois[i][:, 0], want[:, 0]) and np.abs(rois[i] - want).max() < 1e-3, n
        if n in D.GOLDEN_PAGES and post == 4096:      # ... and the reference's own proposal_layer at RPN_POST_NMS_TOP_N = 4096
            # (rows of equal score: the reference leaves their order to numpy's unstable argsort, the oracle and the library order them by index)
            ref, got = util.canon_rows(D.golden()["rois_" + n]), util.canon_rows(rois[i])
            assert got.shape == ref.shape and np.array_equal(got[:, 0], ref[:, 0]) and np.abs(got - ref).max() < 1e-3, n


@pytest.mark.parametrize("names", [("24x48",), ("40x64",), ("64x64",), ("65x64",), ("40x64", "40x64/2"), ("40x64", "40x64/2", "40x64/4", "40x64/2", "40x64")],
                         ids=lambda v: "+".join(v))
def test_proposals_equal_the_oracle(pctx, names):
    rois, anchors = run_pages(pctx, names, nms_columns=1, nms_prefix=1, nms_check=1)
    check_pages(names, rois, anchors)
    if names == ("64x64",):
        assert rois[0].shape[0] == 4096 and rois[0][-1, 0] > 0.9                 # exactly the capacity, every row a line slice
    if names == ("65x64",):
        assert rois[0].shape[0] == 4096 and D.page("65x64")[0].shape[1] == 65    # more survivors than the capacity: the first 4096 in rank order


@pytest.mark.parametrize("names", [("64x64",), ("40x64", "40x64/2")], ids=lambda v: "+".join(v))
def test_every_nms_form_and_prefix_setting_keeps_the_same_rows(pctx, names):
    first = None
    for cols in (0, 1, 2, 3):
        for prefix in (0, 1):
            rois, anchors = run_pages(pctx, names, nms_columns=cols, nms_prefix=prefix, nms_check=1)
            if first is None:
                first = (rois, anchors)
                check_pages(names, rois, anchors)
            assert all(same(a, b) for a, b in zip(rois + anchors, first[0] + first[1])), (cols, prefix)
    pctx.set_option("nms_columns", 1)
    pctx.set_option("nms_prefix", 1)
    for post in (1000, 1001, 1024, 1025):                   # the seams of the prefix choice: a prefix of the 4096-row answer
        rois, anchors = run_pages(pctx, names, post=post)
        assert all(same(a, b[:post]) for a, b in zip(rois + anchors, first[0] + first[1])), post


# ---- the text-line tail at capacity 4096 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tctx():
    with ctpn_amd.Context(0, 8, 1024, 1024, postproc_only=True) as c:
        c.reserve_proposals(4096)
        yield c


def tail(ctx, counts, mode="H", connect_device=1, nms_columns=1, nms_check=0, post=4096):
    for k, v in (("connect_device", connect_device), ("nms_columns", nms_columns), ("nms_check", nms_check)):
        ctx.set_option(k, v)
    ctx.set_param("RPN_POST_NMS_TOP_N", post)
    r = D.oracle_rois("64x64")
    return ctx.debug_text_lines([r[:c] for c in counts], (1024, 1024), None, mode, 2048)


def test_every_count_in_one_batch(tctx):
    """rois of the 64 x 64 page truncated to the counts around 1024 and up to the capacity, one image of every count in one call: the large
    connector equals the host connector byte for byte and the oracle; the keep lists do not depend on the NMS form"""
    assert B.text_line_plan(8, 64, 4096, connect_device=1) == ("one_wg_large", "buckets", 0)
    for mode in "HO":
        dev, keep = tail(tctx, COUNTS, mode, connect_device=1, nms_check=1)
        host, keep_h = tail(tctx, COUNTS, mode, connect_device=0)
        for i, c in enumerate(COUNTS):
            assert same(dev[i], host[i]) and same(keep[i], keep_h[i]), (mode, c)
            if mode == "H" or c in (1025, 4096):
                assert_close_to_oracle(dev[i], D.oracle_lines("64x64", c, mode), (mode, c))
        assert dev[-1].shape[0] == 64 and keep[-1].shape[0] == 4096
        for cols in (0, 2, 3):
            _, keep_c = tail(tctx, COUNTS, mode, connect_device=1, nms_columns=cols, nms_check=1)
            assert all(same(a, b) for a, b in zip(keep, keep_c)), cols


@pytest.mark.parametrize("count", COUNTS)
def test_every_count_as_the_parameter(tctx, count):
    """RPN_POST_NMS_TOP_N = count (the rows per image on the device, odd strides among them), a lone image: up to 1024 rows the forms a fresh
    ctx launches, above them the large ones -- as the plan says -- and the lines of the batch above"""
    large = count > 1024
    assert B.text_line_plan(1, 64, count, connect_device=1) == (("one_wg_large", "buckets", 0) if large else ("column_groups", "all_pairs", 16))
    assert B.text_line_plan(1, 64, count, connect_device=1, nms_columns=2)[0] == ("one_wg_large" if large else "one_wg")
    want = D.oracle_lines("64x64", count, "H")
    for cols in (1, 2):
        dev, keep = tail(tctx, (count,), "H", connect_device=1, nms_columns=cols, nms_check=1, post=count)
        host, keep_h = tail(tctx, (count,), "H", connect_device=0, nms_columns=cols, post=count)
        assert same(dev[0], host[0]) and same(keep[0], keep_h[0])
        assert_close_to_oracle(dev[0], want, count)
    with pytest.raises(B.CtpnError) as e:                    # one row more than the parameter
        tctx.debug_text_lines([D.oracle_rois("64x64")[:count]], (1024, 1024), roi_counts=[count + 1])
    assert e.value.code == -1


def test_pages_of_different_kinds_and_scales_in_one_batch(tctx):
    """the recipe's pages (2560, 1280, 1152 line slices) and an empty image in one call at 4096 rows, scale 1 and 2 (boxes / scale: the
    column id comes from x1 * scale)"""
    names = ["40x64", "40x64/2", "24x48"]
    rois = [D.oracle_rois(n) for n in names] + [np.zeros((0, 5), np.float32)]
    for k in ("nms_columns", "nms_check"):
        tctx.set_option(k, 1)
    tctx.set_param("RPN_POST_NMS_TOP_N", 4096)
    for scale in (1.0, 2.0):
        sc = [scale] * 4
        scaled = [np.hstack([r[:, :1], r[:, 1:] * np.float32(scale)]).astype(np.float32) for r in rois]
        tctx.set_option("connect_device", 1)
        dev, keep = tctx.debug_text_lines(scaled, (int(1024 * scale), int(1024 * scale)), sc, "H", 2048)
        tctx.set_option("connect_device", 0)
        host, keep_h = tctx.debug_text_lines(scaled, (int(1024 * scale), int(1024 * scale)), sc, "H", 2048)
        assert all(same(a, b) for a, b in zip(dev + keep, host + keep_h)), scale
        assert [d.shape[0] for d in dev] == [40, 20, 24, 0]
        if scale == 1.0:
            for i, n in enumerate(names):
                # (the oracle's lines at the page's own size: the size only bounds the clipping and the column table, which no box of these reaches)
                assert_close_to_oracle(dev[i], D.oracle_lines(n, 4096, "H"), n)
                if n in D.GOLDEN_PAGES:
                    assert_close_to_oracle(dev[i], D.golden()["recs_H_" + n], n)      # the reference's own TextDetector


# ---- invariance: a larger capacity changes nothing --------------------------------------------------------------------------------------
def whole_path(ctx):
    """ctpn_detect on 2 x 64 x 96, submit / collect on two slots, ctpn_detect_ragged on the 82-wide canvas -> a flat list of arrays"""
    ims = ctpn_amd.weights.synthetic_images(2, 64, 96, 21)
    out = []
    for mode in "HO":
        lines, rois = ctx.detect(ims, mode=mode, want_rois=True)
        out += lines + rois
    ctx.detect_submit(ims, slot=0)
    ctx.detect_submit(ims[::-1], slot=1)
    for slot in (0, 1):
        lines, rois = ctx.detect_collect(slot, want_rois=True)
        out += lines + rois
    canvas, heights = R.canvas_of(R.images(11, R.W, R.HEIGHTS), R.HC)
    lines, rois = ctx.detect_ragged(canvas, heights, want_rois=True)
    return out + lines + rois


@pytest.fixture(scope="module")
def fresh_results(arena):
    with ctpn_amd.Context(0, 5, 96, 96, "fp32") as c:
        c.load_weights(arena)
        return whole_path(c)


def test_a_larger_capacity_changes_no_result(arena, fresh_results):
    assert sum(a.shape[0] for a in fresh_results) > 0
    assert max(a.shape[0] for a in fresh_results) < 1000                       # fewer than 1000 survivors on these inputs
    with ctpn_amd.Context(0, 5, 96, 96, "fp32") as c:
        c.load_weights(arena)
        c.reserve_proposals(4096)
        got = whole_path(c)                                                    # RPN_POST_NMS_TOP_N = 1000 in 4096-row arrays
        assert len(got) == len(fresh_results) and all(same(a, b) for a, b in zip(got, fresh_results))
        c.set_param("RPN_POST_NMS_TOP_N", 4096)
        got = whole_path(c)                                                    # the valid rows are the same
        assert all(same(a, b) for a, b in zip(got, fresh_results))
        c.set_option("connect_device", 1)
        got = whole_path(c)
        assert all(same(a, b) for a, b in zip(got, fresh_results))


def test_reserve_up_up_and_down_on_one_ctx_and_nothing_is_left(arena, fresh_results):
    gc.collect()
    base = B.live_resources()
    with ctpn_amd.Context(0, 5, 96, 96, "fp32") as c:
        c.load_weights(arena)
        for _ in range(2):      # what the paths create or grow on use exists now: forward set 1, the ragged sets, BOTH staging buffers at the canvas's size
            assert all(same(a, b) for a, b in zip(whole_path(c), fresh_results))
        at_1000 = B.live_resources()
        for cap in (2048, 4096, 1000):
            c.reserve_proposals(cap)
            assert c.proposal_capacity == cap
            got = whole_path(c)
            assert all(same(a, b) for a, b in zip(got, fresh_results)), cap
        live = B.live_resources()
        assert live == at_1000                                                 # back at 1000 rows: the bytes, events and streams of before
    assert B.live_resources() == base
    with ctpn_amd.Context(0, 2, 640, 1024, postproc_only=True) as c:
        c.reserve_proposals(4096)
        rois, anchors = run_pages(c, ("40x64",), nms_check=1)
        check_pages(("40x64",), rois, anchors)
        c.reserve_proposals(2048)
        with pytest.raises(B.CtpnError):                                       # the earlier call's anchors went with its buffers
            c._anchors(1, 4096, [0])
    assert B.live_resources() == base
