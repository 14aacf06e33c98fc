"""GPU: the detection tail under run-time parameters (ctpn_set_param) -- lines_prep_kernel, the connector's NMS in its column forms,
connect_kernel and the collect's host connector through ctpn_debug_text_lines on the scenes and configurations of tests/tail_scenes.py
(a 12 x 20 feature map, 192 x 320 images, under 100 rois each), and the whole path on a small full ctx with the proposal layer's four
values changed as well. tests/test_tail_params.py holds the CPU side (the same configurations on the host connector against the oracle
and the reference's fixture, and the assertion that every configuration changes every scene's lines).

Tolerance against the oracle: tests/test_gpu_text_line_tail.py's -- equal counts and order, scores bit-equal, coordinates within rtol 3e-7
/ atol 1e-5. Device against host connector: byte-equal."""
import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import lines_scenes as S
import tail_scenes as T
import util

pytestmark = pytest.mark.gpu

SCENES = T.scenes()
SIZE = (T.H, T.W)
E2E_PARAMS = {"RPN_PRE_NMS_TOP_N": 300, "RPN_POST_NMS_TOP_N": 100, "RPN_NMS_THRESH": 0.5, "RPN_MIN_SIZE": 16, "LINE_MIN_SCORE": 0.0, "MIN_RATIO": 0.0,
              "TEXT_PROPOSALS_MIN_SCORE": 0.0}
E2E_H, E2E_W = 96, 160


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def set_config(ctx, config):
    """every connector parameter of the ctx: `config` over the defaults"""
    for name, v in zip(T.CFG8_NAMES, T.cfg8(config)):
        ctx.set_param(name, v)
        assert ctx.get_param(name) == v


def host_lines(sc, mode, config):
    return B.text_lines(S.divide(sc.rois[:, 1:5], sc.scale), sc.rois[:, 0], (sc.h, sc.w), mode, device_id=-1, config=T.cfg8(config))


def assert_close_to_oracle(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, 8], want[:, 8]), what
    assert np.allclose(got[:, :8], want[:, :8], rtol=3e-7, atol=1e-5), (what, np.abs(got - want).max())


@pytest.fixture(scope="module")
def pctx():
    with ctpn_amd.Context(0, 5, T.H, T.W, postproc_only=True) as c:
        yield c


@pytest.fixture()
def ctx(pctx):
    yield pctx
    set_config(pctx, {})
    pctx.set_param("RPN_POST_NMS_TOP_N", 1000)
    for k in ("connect_device", "nms_check"):
        pctx.set_option(k, 0)


def run(ctx, scs, mode, connect_device, nms_check=1):
    ctx.set_option("connect_device", connect_device)
    ctx.set_option("nms_check", nms_check)
    return ctx.debug_text_lines([sc.rois for sc in scs], SIZE, [sc.scale for sc in scs], mode)


@pytest.mark.parametrize("cfg_name", list(T.CONFIGS))
def test_tail_under_a_configuration_equals_host_connector_and_oracle(ctx, cfg_name):
    """batches of 1, 2 (the column-per-wave form of the connector's NMS) and 5 images (its one-workgroup form), device and host connector,
    option nms_check on: device records == host connector's, byte for byte; both == the oracle under the same patch"""
    config = T.CONFIGS[cfg_name]
    set_config(ctx, config)
    for mode in "HO":
        want = [T.oracle_lines(sc, mode, config) for sc in SCENES]
        host = [host_lines(sc, mode, config) for sc in SCENES]
        for k in (1, 2, 5):
            dev, keep_d = run(ctx, SCENES[:k], mode, 1)
            hst, keep_h = run(ctx, SCENES[:k], mode, 0)
            for i in range(k):
                what = (cfg_name, mode, k, i)
                assert same(dev[i], hst[i]) and same(dev[i], host[i]) and same(keep_d[i], keep_h[i]), what
                assert_close_to_oracle(dev[i], want[i], what)
                with T.patched(S.P.Cfg, config):
                    assert np.array_equal(keep_d[i], np.array(S.oracle_keep(SCENES[i]), np.int32)), what


def test_defaults_untouched_and_explicit_defaults_are_the_same_bytes():
    with ctpn_amd.Context(0, 5, T.H, T.W, postproc_only=True) as c:
        assert all(c.get_param(n) == B.param_default(n) for n in B.param_names())
        out = {}
        for tag in ("fresh", "explicit"):
            if tag == "explicit":
                for n in B.param_names():
                    c.set_param(n, B.param_default(n))
            for mode in "HO":
                for cd in (1, 0):
                    out[(tag, mode, cd)] = run(c, SCENES, mode, cd)
        for mode in "HO":
            for cd in (1, 0):
                a, b = out[("fresh", mode, cd)], out[("explicit", mode, cd)]
                assert all(same(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
                for i, sc in enumerate(SCENES):
                    assert same(a[0][i], B.text_lines(sc.rois[:, 1:5], sc.rois[:, 0], SIZE, mode, device_id=-1)) and a[0][i].shape[0] >= 5


def test_fewer_rows_per_image_than_the_buffers_hold(ctx):
    """RPN_POST_NMS_TOP_N below 1000 lays the tail's device buffers out with that stride; the caller's arrays keep 1000 rows per image"""
    config = T.CONFIGS["all"]
    set_config(ctx, config)
    base = {(m, cd): run(ctx, SCENES, m, cd) for m in "HO" for cd in (1, 0)}
    ctx.set_param("RPN_POST_NMS_TOP_N", 100)
    assert max(sc.rois.shape[0] for sc in SCENES) <= 100
    for (m, cd), (lines, keeps) in base.items():
        got = run(ctx, SCENES, m, cd)
        assert all(same(x, y) for x, y in zip(got[0] + got[1], lines + keeps)), (m, cd)
    ctx.set_param("RPN_POST_NMS_TOP_N", 64)
    with pytest.raises(ctpn_amd.CtpnError) as e:
        run(ctx, SCENES, "H", 1)                               # more rois than RPN_POST_NMS_TOP_N
    assert e.value.code == -1
    cut = [sc._replace(rois=sc.rois[:64]) for sc in SCENES]
    for cd in (1, 0):
        lines, keeps = run(ctx, cut, "O", cd)
        for i, sc in enumerate(cut):
            assert same(lines[i], host_lines(sc, "O", config)) and lines[i].shape[0] >= 3


def test_parameters_belong_to_their_ctx():
    lo, hi = dict(T.CONFIGS["line_score_0.8"]), {}
    with ctpn_amd.Context(0, 5, T.H, T.W, postproc_only=True) as a, ctpn_amd.Context(0, 5, T.H, T.W, postproc_only=True) as b:
        a.set_param("LINE_MIN_SCORE", 0.8)
        assert a.get_param("LINE_MIN_SCORE") == 0.8 and b.get_param("LINE_MIN_SCORE") == 0.9
        for cd in (1, 0):
            for order in ((a, b), (b, a), (a, b)):
                for c in order:
                    got = run(c, SCENES, "H", cd, nms_check=0)[0]
                    for i, sc in enumerate(SCENES):
                        assert same(got[i], host_lines(sc, "H", lo if c is a else hi)), (cd, i)
        assert any(host_lines(sc, "H", lo).shape != host_lines(sc, "H", hi).shape for sc in SCENES)


def test_out_of_range_and_unknown_parameters_are_argument_errors(ctx):
    bad = [("RPN_PRE_NMS_TOP_N", 0), ("RPN_PRE_NMS_TOP_N", 12001), ("RPN_POST_NMS_TOP_N", 0), ("RPN_POST_NMS_TOP_N", 1001), ("RPN_PRE_NMS_TOP_N", 300.5),
           ("RPN_NMS_THRESH", -0.1), ("RPN_NMS_THRESH", 1.1), ("TEXT_PROPOSALS_NMS_THRESH", -0.1), ("RPN_MIN_SIZE", -1.0), ("MAX_HORIZONTAL_GAP", 4097),
           ("NO_SUCH_PARAMETER", 1.0)]
    bad += [(n, float("nan")) for n in B.param_names()]
    for name, v in bad:
        with pytest.raises(ctpn_amd.CtpnError) as e:
            ctx.set_param(name, v)
        assert e.value.code == -1, (name, v)
    with pytest.raises(ctpn_amd.CtpnError):
        ctx.get_param("NO_SUCH_PARAMETER")
    assert all(ctx.get_param(n) == B.param_default(n) for n in B.param_names())      # a refused value changes nothing
    for name, v in (("RPN_PRE_NMS_TOP_N", 1), ("RPN_PRE_NMS_TOP_N", 12000), ("RPN_NMS_THRESH", 0.0), ("RPN_NMS_THRESH", 1.0), ("RPN_MIN_SIZE", 0.0)):
        ctx.set_param(name, v)
        assert ctx.get_param(name) == v
    for n in B.param_names():
        ctx.set_param(n, B.param_default(n))


# ---- the whole path -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    with ctpn_amd.Context(0, 3, E2E_H, E2E_W, "fp32") as c:
        c.load_weights(util.stress_arena("biased"))
        yield c


def e2e_images(n):
    return np.random.default_rng(77).integers(0, 256, (n, E2E_H, E2E_W, 3), dtype=np.uint8)


def stepwise(c, imgs, mode):
    """forward + proposal layer with the four values as arguments + the stateless connector seam with the configuration, on the same ctx"""
    n = imgs.shape[0]
    c.forward(imgs)
    info = np.tile(np.array([[E2E_H, E2E_W, 1.0]], np.float32), (n, 1))
    rois = c.proposals(info, 300, 100, 0.5, 16.0)
    conn = {k: v for k, v in E2E_PARAMS.items() if k in B.CONNECTOR_PARAM_NAMES}
    lines = [B.text_lines(r[:, 1:5], r[:, 0], (E2E_H, E2E_W), mode, device_id=-1, config=conn) for r in rois]
    return lines, rois


@pytest.mark.parametrize("connect_device", [0, 1])
def test_detect_reads_the_ctx_parameters_end_to_end(full, connect_device):
    """96 x 160 images (6 x 10 cells, 600 anchors), random weights with biases: with the score and ratio floors dropped lines come out
    (asserted). ctpn_detect and submit / collect through both slots == forward + ctpn_proposals(300, 100, 0.5, 16) + ctpn_text_lines_cfg,
    byte for byte, rois included; at most 100 rois per image: nms_prefix and the column forms below their usual cap."""
    c = full
    c.set_option("connect_device", connect_device)
    c.set_option("nms_check", 1)
    for k, v in E2E_PARAMS.items():
        c.set_param(k, v)
    try:
        for mode in "HO":
            want = {n: stepwise(c, e2e_images(3)[:n], mode) for n in (1, 3)}
            for n in (1, 3):
                lines, rois = c.detect(e2e_images(3)[:n], mode=mode, want_rois=True)
                wl, wr = want[n]
                print("n %d mode %s: rois %s, lines %s" % (n, mode, [r.shape[0] for r in rois], [x.shape[0] for x in lines]))
                assert all(0 < r.shape[0] <= 100 for r in rois) and sum(x.shape[0] for x in lines) >= 1
                assert all(same(a, b) for a, b in zip(lines + rois, wl + wr)), (n, mode)
            # both slots in flight: one image in slot 0, three in slot 1; then the other way round
            for first, second in (((0, 1), (1, 3)), ((0, 3), (1, 1)), ((1, 1), (0, 3))):
                for slot, n in (first, second):
                    c.detect_submit(e2e_images(3)[:n], slot=slot)
                for slot, n in (first, second):
                    lines, rois = c.detect_collect(slot, mode=mode, want_rois=True)
                    assert all(same(a, b) for a, b in zip(lines + rois, want[n][0] + want[n][1])), (slot, n, mode)
    finally:
        for n in B.param_names():
            c.set_param(n, B.param_default(n))
        c.set_option("connect_device", 0)
        c.set_option("nms_check", 0)


def test_set_param_waits_for_the_collect(full):
    c = full
    c.detect_submit(e2e_images(1), slot=0)
    with pytest.raises(ctpn_amd.CtpnError) as e:
        c.set_param("LINE_MIN_SCORE", 0.8)
    assert e.value.code == -3 and c.get_param("LINE_MIN_SCORE") == 0.9
    c.detect_collect(0)
    c.set_param("LINE_MIN_SCORE", 0.8)
    assert c.get_param("LINE_MIN_SCORE") == 0.8
    c.set_param("LINE_MIN_SCORE", 0.9)
