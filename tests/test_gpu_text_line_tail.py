"""GPU: the text-line tail of a detection -- lines_prep_kernel, the connector's NMS 0.2 in each of its forms (nms_kernel, the one-workgroup
and the multi-workgroup column kernels with the im_info argument), connect_kernel / the host's connect_lines -- through
ctpn_debug_text_lines, which calls the function ctpn_detect_submit calls, on the generated scenes of tests/lines_scenes.py: controlled
boxes with tied scores, scales that take x1 off the 16-px grid, more than 256 and 512 kept proposals, chains past numpy's pairwise-sum
splits, batches of up to six images, uneven counts, stale scratch, a box outside the image, a full line buffer, exactly 1000 rois.
The oracle is oracle/postproc.py alone (tests/test_lines_scenes.py holds the mutants of it that these scenes catch).

Kept proposals and lines per scene, H / O: the oracle's figures, which every test below asserts the device's equal exactly. The worst
coordinate difference against the oracle is printed per scene and mode by test_records_equal_host_connector_debug_hook_and_oracle (-s) and
asserted there within rtol 3e-7 / atol 1e-5.
    scene      kept   lines H / O        scene      kept   lines H / O
    g0          133    15 / 17           full        661    89 / 101
    g1          261    36 / 36           zoom        166    17 / 17
    g2          173    28 / 28           strip       761     5 / 8      (longest chain 249)
    g3          219    32 / 35           beyond      553    10 / 11     (longest chain 263)
    g4          253    31 / 31           big_scale   123    10 / 10
    g5          158    17 / 18           low, empty    0     0 / 0
    wide        553    72 / 81           deep        300     0 / 0      (one column)
"""
import functools

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import lines_scenes as S
from oracle import postproc as P

pytestmark = pytest.mark.gpu

SCENES = {sc.name: sc for sc in S.scenes()}
NAMES = list(SCENES)


@pytest.fixture(scope="module")
def ctx():
    # a post-processing ctx: no network, no arena. 275 columns: the widest scene
    with ctpn_amd.Context(0, 6, 608, 4400, postproc_only=True) as c:
        yield c


@functools.lru_cache(maxsize=None)
def want_lines(name, mode):
    return S.oracle_lines(SCENES[name], mode)


@functools.lru_cache(maxsize=None)
def want_keep(name):
    return np.array(S.oracle_keep(SCENES[name]), np.int32)


def run(ctx, scs, mode="H", connect_device=1, nms_columns=1, nms_check=0, roi_counts=None, line_capacity=512):
    """one ctpn_debug_text_lines call on scenes of one geometry -> (lines per image, keep list per image)"""
    for k, v in (("connect_device", connect_device), ("nms_columns", nms_columns), ("nms_check", nms_check)):
        ctx.set_option(k, v)
    assert len({(sc.h, sc.w) for sc in scs}) == 1
    return ctx.debug_text_lines([sc.rois for sc in scs], (scs[0].h, scs[0].w), [sc.scale for sc in scs], mode, line_capacity, roi_counts)


_alone = {}


def alone(ctx, name, mode):
    """the scene in a call of its own, device connector, default NMS form (computed once per module)"""
    if (name, mode) not in _alone:
        lines, keeps = run(ctx, [SCENES[name]], mode)
        _alone[(name, mode)] = (lines[0], keeps[0])
    return _alone[(name, mode)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_keep_lists_of_every_nms_form_equal_the_oracle(ctx, name):
    """nms_columns 0 (nms_kernel), 1 (a lone image: one column per wave over many workgroups), 2 (one workgroup), 3 (multi-workgroup): one keep
    list, the oracle's greedy NMS on the fp32 boxes / scale of the score > 0.7 prefix; nms_check = 1 (the generic kernel behind a column form)
    stays silent. The scenes beyond 256 columns or scale 4 are outside the column forms' domain: every setting takes nms_kernel there, seen
    here as equality."""
    sc = SCENES[name]
    for nc in (0, 1, 2, 3):
        _, keeps = run(ctx, [sc], "H", nms_columns=nc, nms_check=1)
        assert np.array_equal(keeps[0], want_keep(name)), (name, nc)


def test_kept_list_past_its_lds_capacity(ctx):
    """scene "deep": one 16-px column that keeps 300 boxes, more than a wave of either column form holds in LDS (48: the one-workgroup form,
    which re-reads the rest from its spill slice; 256: the multi-workgroup form, which re-reads them from the sorted boxes by kept rank),
    and dropped candidates whose ONLY suppressor sits past those capacities -- asserted on the oracle's own keep list first, so a form that
    loses or misreads a kept box beyond its capacity keeps a candidate the oracle drops."""
    sc = SCENES["deep"]
    assert sc.scale == 1.0 and np.unique(sc.rois[:, 1]).size == 1                  # one image-scale column
    keep = S.oracle_keep(sc)
    depths = S.sole_suppressor_depths(S.prefix_dets(sc), keep, 0.2)
    print("deep: %d rois, %d kept, %d dropped by one kept box alone, %d of them at depth >= 48, %d at depth >= 256"
          % (sc.rois.shape[0], len(keep), len(depths), sum(d >= 48 for d in depths), sum(d >= 256 for d in depths)))
    assert len(keep) > 256
    assert sum(d >= 48 for d in depths) >= 8 and sum(d >= 256 for d in depths) >= 8          # as tests/test_lines_scenes.py holds the scene to
    for nc in (0, 1, 2, 3):
        _, keeps = run(ctx, [sc], "H", nms_columns=nc, nms_check=1)
        assert np.array_equal(keeps[0], want_keep("deep")), nc


def test_proposal_kept_list_past_its_lds_capacity():
    """the same for the proposal layer's instantiation of the one-workgroup column NMS (128 kept boxes per wave in LDS), through
    ctpn_proposals_from_host on crafted heads (lines_scenes.deep_heads): column 0 keeps 150 boxes, and 50 candidates are dropped by one
    kept box alone, 22 of them by a box at kept position >= 128 -- on the oracle first. Every form then returns the oracle's anchors (the
    keep list, exactly) and its boxes (to the last ulp of exp(), as decode always does)."""
    cls, box, info = S.deep_heads()
    boxes, scores, _ = P.decode(cls, box, info)
    ok = np.where((boxes[:, 2] - boxes[:, 0] + 1 >= 8) & (boxes[:, 3] - boxes[:, 1] + 1 >= 8))[0]
    order = ok[P.desc_order(scores[ok])]
    dets = np.hstack([boxes[order], scores[order][:, None]])
    keep = P.nms(dets, 0.7)
    depths = S.sole_suppressor_depths(dets, keep, 0.7)
    print("deep heads: %d candidates, %d kept, %d dropped by one kept box alone, %d of them at depth >= 128"
          % (order.size, len(keep), len(depths), sum(d >= 128 for d in depths)))
    assert len(keep) > 128 and np.all(dets[keep, 0] < 16) and len(keep) < order.size
    assert sum(d >= 128 for d in depths) >= 8
    want = P.proposal_layer(cls, box, info)
    assert np.array_equal(want[:, 1:], dets[keep, :4])
    for nc in (0, 1, 2, 3):
        with ctpn_amd.Context(0, 1, int(info[0]), int(info[1]), "fp32", postproc_only=True, options={"nms_columns": nc, "nms_check": 1}) as c:
            rois, anchors = c.proposals_from_host(cls, box, info, want_anchors=True)
        assert np.array_equal(anchors[0], order[keep]), nc
        assert rois[0].shape == want.shape and np.array_equal(rois[0][:, 0], want[:, 0]) and np.abs(rois[0] - want).max() < 1e-3, nc


@pytest.mark.parametrize("mode", ["H", "O"])
@pytest.mark.parametrize("name", NAMES)
def test_records_equal_host_connector_debug_hook_and_oracle(ctx, name, mode):
    sc = SCENES[name]
    dev, keep = alone(ctx, name, mode)
    assert np.array_equal(keep, want_keep(name))                                # the keep list of this mode's call too (the NMS runs before the mode counts)
    host = run(ctx, [sc], mode, connect_device=0)[0][0]
    assert same(dev, host)                                                      # connect_kernel == connect_lines, bit for bit
    assert same(dev, B.debug_connect(sc.rois, (sc.h, sc.w), mode, sc.scale))    # ... == the one-image hook on the generic NMS
    want = want_lines(name, mode)
    worst = float(np.abs(dev[:, :8] - want[:, :8]).max()) if dev.shape == want.shape and dev.size else 0.0
    print("%-9s %s  kept %4d  lines %3d  worst %.3g" % (name, mode, keep.size, dev.shape[0], worst))
    assert dev.shape == want.shape                                              # same count ...
    assert np.array_equal(dev[:, 8], want[:, 8])                                # ... same order, and scores are plain fp32 means
    # coordinates: np.polyfit on float32 data is LAPACK's float32 least squares, the product a double closed form rounded to fp32
    # (tests/test_properties.py::test_host_connector_equals_oracle_on_generated_proposals: the same bound for the same reason)
    assert np.allclose(dev[:, :8], want[:, :8], rtol=3e-7, atol=1e-5), worst


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6])
def test_batch_equals_its_images_alone(ctx, k):
    """k different scenes, each with its own scale, in one launch: image-strided scratch, counts and records. Up to four images take the
    column-per-wave NMS, six the one-workgroup form; both connectors; nms_columns = 3 / 2 pin the other form at the same size."""
    names = S.BATCH_NAMES[:k]
    scs = [SCENES[n] for n in names]
    for mode in "HO":
        for cd, nc in ((1, 1), (0, 1), (1, 3), (1, 2), (1, 0)):
            lines, keeps = run(ctx, scs, mode, connect_device=cd, nms_columns=nc, nms_check=1)
            for i, n in enumerate(names):
                assert same(lines[i], alone(ctx, n, mode)[0]) and same(keeps[i], alone(ctx, n, mode)[1]), (k, mode, cd, nc, n)


def test_uneven_roi_counts_with_an_empty_image_in_the_middle(ctx):
    names = ["g1", "g0", "g3", "g2", "g4"]
    counts = [SCENES["g1"].rois.shape[0], 0, 100, 1, SCENES["g4"].rois.shape[0]]
    scs = [SCENES[n] for n in names]
    for mode in "HO":
        for cd in (1, 0):
            lines, keeps = run(ctx, scs, mode, connect_device=cd, roi_counts=counts)
            for i, (n, cnt) in enumerate(zip(names, counts)):
                cut = S.Scene(n, SCENES[n].rois[:cnt], SCENES[n].h, SCENES[n].w, SCENES[n].scale)
                one_l, one_k = run(ctx, [cut], mode)
                assert same(lines[i], one_l[0]) and same(keeps[i], one_k[0]), (mode, cd, n)
                assert np.array_equal(keeps[i], np.array(S.oracle_keep(cut), np.int32))
            assert lines[1].shape[0] == 0 and keeps[1].size == 0 and keeps[3].size == 1


def test_repeated_and_smaller_calls_leave_nothing_stale(ctx):
    """the same call twice: the same bytes; a small call after a larger one (more images, more rois, more lines, another geometry): the
    bytes the small one gave before -- conn_scratch, tl_*, the records and the multi-workgroup NMS's scratch carry nothing over"""
    six = [SCENES[n] for n in S.BATCH_NAMES]
    for mode in "HO":
        for cd in (1, 0):
            small = [x[0] for x in run(ctx, [SCENES["g5"]], mode, connect_device=cd)]
            a = run(ctx, six, mode, connect_device=cd)
            b = run(ctx, six, mode, connect_device=cd)
            assert all(same(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
            run(ctx, [SCENES["full"], SCENES["wide"]], mode, connect_device=cd)
            again = [x[0] for x in run(ctx, [SCENES["g5"]], mode, connect_device=cd)]
            assert same(small[0], again[0]) and same(small[1], again[1])
            low = run(ctx, [SCENES["low"], SCENES["empty"]], mode, connect_device=cd)
            assert all(x.size == 0 for x in low[0] + low[1])


def test_full_buffers_in_the_last_image_of_a_full_batch(ctx):
    """exactly 1000 rois, all above 0.7, in every position of a max_batch call: lines_prep's look-ahead row of the last image is the rois
    buffer's last row"""
    assert SCENES["full"].rois.shape[0] == 1000 and SCENES["full"].rois[-1, 0] > np.float32(0.7)
    names = ["wide", "full", "full", "wide", "full", "full"]
    for mode in "HO":
        for cd in (1, 0):
            lines, keeps = run(ctx, [SCENES[n] for n in names], mode, connect_device=cd, nms_check=1)
            for i, n in enumerate(names):
                assert same(lines[i], alone(ctx, n, mode)[0]) and same(keeps[i], alone(ctx, n, mode)[1])


def test_box_outside_the_image_is_the_references_index_error(ctx):
    """scale 0.5: boxes / scale reach past im_w, where the reference's boxes_table[int(x1)] raises IndexError. Both connectors answer with the
    argument error that says so, alone and as one image of a batch, and the ctx works afterwards."""
    out = S.make_scene(S.OUTSIDE)
    assert (S.prefix_dets(out)[:, 0] >= out.w).any()
    for cd in (1, 0):
        for scs in ([out], [SCENES["g0"], out, SCENES["g2"]]):
            for nc in (1, 0):
                with pytest.raises(ctpn_amd.CtpnError) as e:
                    run(ctx, scs, "H", connect_device=cd, nms_columns=nc)
                assert e.value.code == -1 and "IndexError" in str(e.value)
        for mode in "HO":
            got = run(ctx, [SCENES["g0"], SCENES["g2"]], mode, connect_device=cd)
            assert same(got[0][0], alone(ctx, "g0", mode)[0]) and same(got[0][1], alone(ctx, "g2", mode)[0])


def test_line_capacity_one_short_reports_the_true_count(ctx):
    for mode in "HO":
        n_lines = alone(ctx, "g0", mode)[0].shape[0]
        assert n_lines >= 10
        for cd in (1, 0):
            with pytest.raises(ctpn_amd.CtpnError) as e:
                run(ctx, [SCENES["g0"]], mode, connect_device=cd, line_capacity=n_lines - 1)
            assert e.value.code == B.CTPN_ERR_CAPACITY and e.value.line_counts[0] == n_lines
            exact = run(ctx, [SCENES["g0"]], mode, connect_device=cd, line_capacity=n_lines)
            assert same(exact[0][0], alone(ctx, "g0", mode)[0])


def test_argument_errors(ctx):
    sc = SCENES["g0"]
    with pytest.raises(ctpn_amd.CtpnError) as e:
        run(ctx, [sc] * 7)                                                       # more images than max_batch
    assert e.value.code == B.CTPN_ERR_CAPACITY
    with pytest.raises(ctpn_amd.CtpnError) as e:
        run(ctx, [sc], roi_counts=[1001])
    assert e.value.code == -1
    assert same(run(ctx, [sc])[0][0], alone(ctx, "g0", "H")[0])
