"""GPU: pages in tiles on the device -- the cut kernel (ctpn_page_cut), the page form of the column NMS (ctpn_page_nms) and the whole path
(ctpn_amd.detect_page over a ctx's two slots), each against tests/page_ref.py's restatement and the library's own single-image calls:
  * cut: bytes equal to the restatement for a page that is the tile itself, a 9-tile page and a page smaller than the tile; host and device
    sources and destinations; a pitch of 3 w + 5 with the page 1, 2 and 3 bytes into its buffer; first > 0; every byte of the n tiles written
    and none behind them (the buffers are poisoned in front of the call);
  * page NMS: the keep list equals ctpn_nms's and the restatement's on column-aligned boxes -- r in {0, 1, 63, 64, 65, 1000, 20000} x columns
    in {1, 2, 1024} x thresholds {0.2, 0.7}; 300 boxes in one column (more than a chunk, and more kept than the LDS holds); equal scores;
    pairs whose fp32 IoU is the threshold and the floats next to it; a box outside the domain is CTPN_ERR_ARG;
  * whole path (fp32 and bf16 ctx, max_batch 4, tile 64 x 96, overlap 32, the biased arena of tests/util.py): a page that is one tile gives
    ctpn_detect's rois and lines; a 100 x 203 page (9 tiles, 3 chunks: both slots, a short last chunk) equals, in exact bytes, the
    composition cut -> ctpn_detect per tile alone -> restatement merge -> ctpn_text_lines_cfg, for both nms_form values; twice on one ctx
    with a uniform ctpn_detect in between gives the same bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_cases as K  # noqa: E402
import page_ref as R  # noqa: E402
from util import stress_arena  # noqa: E402

import ctpn_amd  # noqa: E402
from ctpn_amd import _binding as B  # noqa: E402
from ctpn_amd import page as PG  # noqa: E402

pytestmark = pytest.mark.gpu

TH, TW, V = K.TILE_H, K.TILE_W, K.OVERLAP
POISON = 0xCD


def rand_page(h, w):
    return np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def cut_raw(page_ptr, on_dev, h, w, pitch, tiles, first, n, out_ptr, out_dev, capacity):
    lib = B.load_library()
    t = np.ascontiguousarray(tiles, np.int32)
    return lib.ctpn_page_cut(0, C.c_void_p(page_ptr), on_dev, h, w, pitch, t.ctypes.data_as(C.POINTER(C.c_int)), first, n, TH, TW, C.c_void_p(out_ptr), out_dev, capacity)


# ---- the cut ----
@pytest.mark.parametrize("shape", [(64, 96), (100, 203), (40, 50)])
def test_cut_equals_the_restatement_from_and_to_host_and_device(shape):
    import torch
    h, w = shape
    page = rand_page(h, w)
    tiles, _ = B.page_plan(h, w, TH, TW, V)
    n = len(tiles)
    want = R.cut(page, tiles, TH, TW)
    need = n * TH * TW * 3
    dpage = torch.from_numpy(page).cuda()
    for src_dev in (0, 1):
        for dst_dev in (0, 1):
            src = dpage.data_ptr() if src_dev else page.ctypes.data
            if dst_dev:
                out = torch.full((need + TH * TW * 3,), POISON, dtype=torch.uint8, device="cuda")      # one tile of room behind the n
                torch.cuda.synchronize()
                assert cut_raw(src, src_dev, h, w, 3 * w, tiles, 0, n, out.data_ptr(), 1, need) == 0
                got = out.cpu().numpy()
            else:
                got = np.full(need + TH * TW * 3, POISON, np.uint8)
                assert cut_raw(src, src_dev, h, w, 3 * w, tiles, 0, n, got.ctypes.data, 0, need) == 0
            assert np.array_equal(got[:need].reshape(want.shape), want), (src_dev, dst_dev)      # every byte written: none is the poison's by chance
            assert (got[need:] == POISON).all(), (src_dev, dst_dev)
    assert np.array_equal(B.page_cut(page, tiles, 0, n, TH, TW), want)                            # the binding's host form


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_cut_takes_any_pitch_and_any_page_alignment(shift):
    import torch
    h, w = 100, 203
    page = rand_page(h, w)
    tiles, _ = B.page_plan(h, w, TH, TW, V)
    want = R.cut(page, tiles, TH, TW)
    buf, view = K.pitched(page, 5, shift)
    assert view.ctypes.data % 4 == (buf.ctypes.data + shift) % 4 and view.strides[0] == 3 * w + 5
    assert np.array_equal(B.page_cut(view, tiles, 0, len(tiles), TH, TW), want)                   # host source
    dbuf = torch.from_numpy(buf).cuda()
    out = torch.full((len(tiles), TH, TW, 3), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert (dbuf.data_ptr() + shift) % 4 == shift % 4
    B.page_cut(None, tiles, 0, len(tiles), TH, TW, out_ptr=out.data_ptr(), page_ptr=dbuf.data_ptr() + shift, page_shape=(h, w), pitch=3 * w + 5)
    assert np.array_equal(out.cpu().numpy(), want)                                                # device source, device destination


def test_cut_of_a_later_range_of_tiles_and_its_argument_errors():
    h, w = 100, 203
    page = rand_page(h, w)
    tiles, _ = B.page_plan(h, w, TH, TW, V)
    want = R.cut(page, tiles, TH, TW)
    assert np.array_equal(B.page_cut(page, tiles, 4, 5, TH, TW), want[4:])                        # first > 0: the short last chunk of a batch-4 run
    assert np.array_equal(B.page_cut(page, tiles, 8, 1, TH, TW), want[8:])
    out = np.zeros(5 * TH * TW * 3, np.uint8)
    assert cut_raw(page.ctypes.data, 0, h, w, 3 * w, tiles, 4, 5, out.ctypes.data, 0, out.size - 1) == B.CTPN_ERR_CAPACITY
    assert cut_raw(page.ctypes.data, 0, h, w, 3 * w - 1, tiles, 4, 5, out.ctypes.data, 0, out.size) == -1      # pitch below 3 w
    bad = tiles.copy()
    bad[6, 0] += 16                                                                               # a tile whose valid part leaves the page
    assert cut_raw(page.ctypes.data, 0, h, w, 3 * w, bad, 4, 5, out.ctypes.data, 0, out.size) == -1
    assert not out.any()


# ---- the page NMS ----
def check_nms(b, thr):
    got = B.page_nms_sorted(b, thr, 0)
    assert got.tolist() == B.nms_sorted(b, thr, 0).tolist()
    assert got.tolist() == R.nms(b, thr).tolist()
    return got


@pytest.mark.parametrize("thr", [0.2, 0.7])
@pytest.mark.parametrize("ncols", [1, 2, 1024])
@pytest.mark.parametrize("r", [0, 1, 63, 64, 65, 1000, 20000])
def test_page_nms_equals_ctpn_nms_and_the_restatement(r, ncols, thr):
    b = K.column_boxes(7 * r + ncols, r, ncols, span=600.0 if ncols > 2 else 2400.0)
    keep = check_nms(b, thr)
    assert len(keep) == 0 if r == 0 else 0 < len(keep) <= r
    if r >= 1000:
        assert len(keep) < r                                                                      # something was suppressed
    if r and ncols == 1024:
        assert (b[:, 0] == 16 * 1023).any()


def test_page_nms_crowded_column_equal_scores_and_threshold_pairs():
    b = K.column_boxes(3, 340, 4, span=3000.0, crowd=(2, 300), heights=(8.0, 12.0))
    keep = check_nms(b, 0.2)
    assert (b[:, 0] == 32).sum() >= 300 and (b[keep, 0] == 32).sum() > 128                        # more than a chunk; more kept than the LDS list holds
    check_nms(K.column_boxes(9, 2000, 3, span=900.0, equal_scores=8), 0.2)
    check_nms(K.column_boxes(10, 500, 40, span=200.0, equal_scores=500), 0.7)                     # one score for all: rank order decides
    for thr in (0.2, 0.7):
        rows, survives = K.threshold_pairs(thr)
        keep = check_nms(rows, thr)
        assert [2 * k + 1 in keep for k in range(3)] == survives == [True, True, False]


def test_page_nms_refuses_a_box_outside_its_domain():
    good = K.column_boxes(1, 200, 8)
    check_nms(good, 0.2)
    bad = good.copy()
    bad[17, 2] = bad[17, 0] + 17.0                                                                # reaches into the next column
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.page_nms_sorted(bad, 0.2, 0)
    assert e.value.code == -1 and "domain" in str(e.value)
    assert B.nms_sorted(bad, 0.2, 0).tolist() == R.nms(bad, 0.2).tolist()                         # form 0 takes anything
    with pytest.raises(ctpn_amd.CtpnError):
        B.page_text_lines(bad[:, :4], bad[:, 4], (700, 128), device_id=0, nms_form=1)
    assert B.page_text_lines(bad[:, :4], bad[:, 4], (700, 128), device_id=0, nms_form=0).tobytes() == \
        B.text_lines(bad[:, :4], bad[:, 4], (700, 128), device_id=0).tobytes()


# ---- the whole path ----
@pytest.fixture(scope="module")
def biased_arena():
    return stress_arena("biased")


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def ctx(request, biased_arena):
    with ctpn_amd.Context(0, 4, TH, TW, request.param) as c:
        c.load_weights(biased_arena)
        yield c


def composition(ctx, page, mode):
    """the page path written out from public calls: cut, ctpn_detect per tile alone, restatement merge, ctpn_text_lines_cfg"""
    h, w = page.shape[:2]
    tiles, grid = R.plan(h, w, TH, TW, V)
    cut = B.page_cut(page, tiles, 0, len(tiles), TH, TW)
    cap = ctx.proposal_capacity
    rois = np.zeros((len(tiles), cap, 5), np.float32)
    counts = np.zeros(len(tiles), np.int32)
    for t in range(len(tiles)):
        _, r = ctx.detect(cut[t][None], mode=mode, want_rois=True)
        rois[t, : len(r[0])] = r[0]
        counts[t] = len(r[0])
    boxes, scores, src = R.merge(tiles, rois, counts, h, w, ctx.get_param("RPN_MIN_SIZE"))
    lines = B.text_lines(boxes, scores, (h, w), mode=mode, device_id=0, capacity=4096, config=PG.ctx_connector_config(ctx))
    return tiles, grid, rois, counts, boxes, scores, src, lines


def test_a_page_that_is_one_tile_is_ctpn_detect(ctx):
    page = ctpn_amd.weights.synthetic_images(1, TH, TW, 7)[0]
    lines, rois = ctx.detect(page[None], want_rois=True)
    for form in (0, 1):
        got = ctpn_amd.detect_page(ctx, page, overlap=V, nms_form=form)
        assert got.grid == (1, 1) and len(got.tiles) == 1
        keep = R.merge(got.tiles, rois[0][None], [len(rois[0])], TH, TW, ctx.get_param("RPN_MIN_SIZE"))      # minus what the page clip and min_size drop
        assert len(keep[0]) > 0 and np.array_equal(got.boxes, keep[0]) and np.array_equal(got.scores, keep[1]) and np.array_equal(got.src, keep[2])
        assert np.array_equal(got.boxes, rois[0][keep[2], 1:5])
        assert len(lines[0]) > 0 and got.lines.tobytes() == lines[0].tobytes()


@pytest.mark.parametrize("mode", ["H", "O"])
def test_nine_tiles_in_three_chunks_equal_the_composition(ctx, mode):
    page = ctpn_amd.weights.synthetic_images(1, 100, 203, 7)[0]
    tiles, grid, rois, counts, boxes, scores, src, lines = composition(ctx, page, mode)
    assert grid == (3, 3) and ctx.max_batch == 4                                                   # chunks of 4, 4 and 1: both slots, a short last chunk
    owners = np.unique(src // ctx.proposal_capacity)
    assert len(owners) >= 2                                                                        # at least two tiles contribute owned rois
    owned_only = R.merge(tiles, rois, counts, 100, 203, -1.0)[0]                                   # (no size filter: what is missing here, ownership dropped)
    assert int(counts.sum()) - len(owned_only) >= 1                                                # at least one roi is dropped by ownership
    assert len(lines) >= 1                                                                         # at least one line results
    for form in (0, 1):
        got = ctpn_amd.detect_page(ctx, page, overlap=V, mode=mode, nms_form=form)
        assert np.array_equal(got.tiles, tiles) and got.grid == grid
        assert got.boxes.tobytes() == boxes.tobytes() and got.scores.tobytes() == scores.tobytes() and got.src.tobytes() == src.tobytes()
        assert got.lines.tobytes() == lines.tobytes(), form


def test_detect_page_twice_with_a_uniform_detect_in_between(ctx):
    import torch
    page = ctpn_amd.weights.synthetic_images(1, 100, 203, 7)[0]
    other = ctpn_amd.weights.synthetic_images(2, TH, TW, 3)
    a = ctpn_amd.detect_page(ctx, page, overlap=V)
    between = ctx.detect(other)
    b = ctpn_amd.detect_page(ctx, torch.from_numpy(page).cuda(), overlap=V)                       # ... and from a page already on the device
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert len(a.lines) >= 1
    again = ctx.detect(other)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(between, again))
