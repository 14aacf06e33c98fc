"""CPU: the detection tail's run-time parameters -- the ctpn_param_* table, ctpn_text_lines_cfg (the host connector under an edited
TextLineCfg) against oracle/postproc.py under the same edit and against a fixture recorded from the reference's own TextDetector,
TextDetector(config=...), and the batch demo's --connector argument. Scenes and configurations: tests/tail_scenes.py.

Tolerance of the connector-against-oracle comparisons: what tests/test_properties.py::test_host_connector_equals_oracle_on_generated_proposals
and tests/test_gpu_text_line_tail.py use for the same pair -- equal counts and order, scores bit-equal, coordinates within rtol 3e-7 /
atol 1e-5 (np.polyfit on fp32 data is LAPACK's fp32 least squares, the C++ a double closed form rounded to fp32)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import ctpn_amd  # noqa: F401
from ctpn_amd import _binding as B
import tail_scenes as T

SCENES = {sc.name: sc for sc in T.scenes()}
TABLE = [("RPN_PRE_NMS_TOP_N", 12000), ("RPN_POST_NMS_TOP_N", 1000), ("RPN_NMS_THRESH", 0.7), ("RPN_MIN_SIZE", 8),
         ("TEXT_PROPOSALS_MIN_SCORE", 0.7), ("TEXT_PROPOSALS_NMS_THRESH", 0.2), ("MAX_HORIZONTAL_GAP", 50), ("MIN_V_OVERLAPS", 0.7),
         ("MIN_SIZE_SIM", 0.7), ("MIN_RATIO", 0.5), ("LINE_MIN_SCORE", 0.9), ("MIN_LINE_WIDTH", 32)]


def host_lines(scene, mode, config=None):
    """the host connector (device_id -1: its own greedy NMS) on the scene as the tail feeds it: boxes / scale, scores, the network size"""
    import lines_scenes as S
    return B.text_lines(S.divide(scene.rois[:, 1:5], scene.scale), scene.rois[:, 0], (scene.h, scene.w), mode, device_id=-1,
                        config=None if config is None else T.cfg8(config))


def assert_lines_close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, 8], want[:, 8]), what
    assert np.allclose(got[:, :8], want[:, :8], rtol=3e-7, atol=1e-5), (what, np.abs(got - want).max())


@functools.lru_cache(maxsize=None)
def default_oracle(name, mode):
    return T.oracle_lines(SCENES[name], mode)


def test_parameter_table_names_and_defaults(golden_dir):
    lib = B.load_library()
    for sym in ("ctpn_set_param", "ctpn_get_param", "ctpn_param_count", "ctpn_param_name", "ctpn_param_default", "ctpn_text_lines_cfg"):
        assert hasattr(lib, sym), sym
    assert lib.ctpn_abi_version() == 10
    assert B.param_names() == [n for n, _ in TABLE] and lib.ctpn_param_name(12) is None and lib.ctpn_param_name(-1) is None
    for name, dflt in TABLE:
        assert B.param_default(name) == dflt, name
    # ... equal to the connector's compiled defaults (fp32 values where the connector compares in fp32) ...
    built = B.connector_constants()
    assert list(built) == list(B.CONNECTOR_CONSTANT_NAMES) and B.CONNECTOR_PARAM_NAMES == T.CFG8_NAMES
    for pname, cname in zip(B.CONNECTOR_PARAM_NAMES, B.CONNECTOR_CONSTANT_NAMES):
        d = B.param_default(pname)
        assert built[cname] in (d, float(np.float32(d))), pname
        assert T.DEFAULTS[pname] == d
    # ... and to the reference's configuration as recorded from it
    ref = json.load(open(os.path.join(golden_dir, "config.json")))
    for name in ("RPN_PRE_NMS_TOP_N", "RPN_POST_NMS_TOP_N", "RPN_NMS_THRESH", "RPN_MIN_SIZE"):
        assert B.param_default(name) == ref["TEST"][name]
    for name in B.CONNECTOR_PARAM_NAMES[1:]:
        assert B.param_default(name) == ref["TextLineCfg"][name]
    assert B.param_default("MIN_LINE_WIDTH") == ref["TextLineCfg"]["TEXT_PROPOSALS_WIDTH"] * ref["TextLineCfg"]["MIN_NUM_PROPOSALS"]
    v = C.c_double(0)
    assert lib.ctpn_param_default(b"NO_SUCH", C.byref(v)) == -1 and lib.ctpn_param_default(None, C.byref(v)) == -1
    assert lib.ctpn_set_param(None, b"MIN_RATIO", 0.5) == -1 and lib.ctpn_get_param(None, b"MIN_RATIO", C.byref(v)) == -1


@pytest.mark.parametrize("cfg_name", list(T.CONFIGS))
def test_every_configuration_changes_the_oracles_lines(cfg_name):
    """on the oracle alone: a knob that changes nothing on a scene could pass every comparison below silently"""
    for name, sc in SCENES.items():
        for mode in "HO":
            got, base = T.oracle_lines(sc, mode, T.CONFIGS[cfg_name]), default_oracle(name, mode)
            assert got.shape != base.shape or not np.array_equal(got, base), (cfg_name, name, mode)
    assert T.oracle_lines(SCENES["t1"], "H").tobytes() == default_oracle("t1", "H").tobytes()        # the patch is undone


@pytest.mark.parametrize("mode", ["H", "O"])
@pytest.mark.parametrize("cfg_name", list(T.CONFIGS))
def test_host_connector_under_a_configuration_equals_the_patched_oracle(cfg_name, mode):
    for name, sc in SCENES.items():
        assert sc.rois.shape[0] <= 300 and (sc.h, sc.w) == (192, 320)
        want = T.oracle_lines(sc, mode, T.CONFIGS[cfg_name])
        assert_lines_close(host_lines(sc, mode, T.CONFIGS[cfg_name]), want, (cfg_name, name, mode))
        assert_lines_close(host_lines(sc, mode), default_oracle(name, mode), ("default", name, mode))


def test_reference_fixture_pins_host_connector_and_patched_oracle(golden_dir):
    """tests/golden/connector_cfg_cases.npz (tools/make_connector_cfg_golden.py): the reference's TextDetector under three edited
    TextLineCfg's on these scenes, their tied scores made distinct (its sort is unstable on ties). Inputs and configuration values are
    the file's."""
    import lines_scenes as S
    g = np.load(os.path.join(golden_dir, "connector_cfg_cases.npz"))
    assert [str(n) for n in g["cfg8_names"]] == list(T.CFG8_NAMES) and len(g["config_names"]) == 3
    size = tuple(int(v) for v in g["size"])
    for cfg_name in (str(n) for n in g["config_names"]):
        cfg8 = g["cfg8_" + cfg_name]
        assert np.array_equal(cfg8, T.cfg8(T.CONFIGS[cfg_name]))
        for name in SCENES:
            rois = g["rois_" + name]
            sc = S.Scene(name, rois, size[0], size[1], 1.0)
            for mode in "HO":
                want = g["recs_%s_%s_%s" % (cfg_name, name, mode)]
                base = T.oracle_lines(sc, mode)
                assert want.shape != base.shape or not np.array_equal(want, base)                       # the edit shows in the reference's lines
                got = B.text_lines(rois[:, 1:5], rois[:, 0], size, mode, device_id=-1, config=cfg8)
                assert_lines_close(got, want, ("host", cfg_name, name, mode))
                assert_lines_close(T.oracle_lines(sc, mode, T.CONFIGS[cfg_name]), want, ("oracle", cfg_name, name, mode))


def _raw_text_lines(sc, mode, cfg8, use_cfg_entry=True):
    lib = B.load_library()
    b = np.ascontiguousarray(sc.rois[:, 1:5])
    s = np.ascontiguousarray(sc.rois[:, 0])
    recs = np.full((256, 9), -7.0)
    cnt = C.c_int(-1)
    f32 = C.POINTER(C.c_float)
    args = [b.ctypes.data_as(f32), s.ctypes.data_as(f32), b.shape[0], sc.h, sc.w, mode, -1]
    if use_cfg_entry:
        rc = lib.ctpn_text_lines_cfg(*args, None if cfg8 is None else cfg8.ctypes.data_as(C.POINTER(C.c_double)),
                                     recs.ctypes.data_as(C.POINTER(C.c_double)), 256, C.byref(cnt))
    else:
        rc = lib.ctpn_text_lines(*args, recs.ctypes.data_as(C.POINTER(C.c_double)), 256, C.byref(cnt))
    return rc, cnt.value, recs


def test_null_and_explicit_default_configuration_are_ctpn_text_lines():
    dflt = T.cfg8({})
    assert np.array_equal(dflt, np.array([B.param_default(n) for n in B.CONNECTOR_PARAM_NAMES]))
    for sc in SCENES.values():
        for mode in (0, 1):
            rc0, n0, r0 = _raw_text_lines(sc, mode, None, use_cfg_entry=False)
            assert rc0 == 0 and n0 >= 5
            for cfg8 in (None, dflt):
                rc, n, r = _raw_text_lines(sc, mode, cfg8)
                assert (rc, n) == (0, n0) and r.tobytes() == r0.tobytes()


def test_out_of_range_values_are_argument_errors():
    sc = SCENES["t1"]
    idx = {n: i for i, n in enumerate(T.CFG8_NAMES)}
    bad = [(n, float("nan")) for n in T.CFG8_NAMES] + [(n, float("inf")) for n in T.CFG8_NAMES]
    bad += [("TEXT_PROPOSALS_NMS_THRESH", -0.1), ("TEXT_PROPOSALS_NMS_THRESH", 1.5), ("MAX_HORIZONTAL_GAP", -1.0), ("MAX_HORIZONTAL_GAP", 4097.0),
            ("MAX_HORIZONTAL_GAP", 20.5), ("MIN_V_OVERLAPS", 1e39)]
    for name, v in bad:
        cfg8 = T.cfg8({})
        cfg8[idx[name]] = v
        rc, n, _ = _raw_text_lines(sc, 0, cfg8)
        assert rc == -1 and n == 0 and name.encode() in B.load_library().ctpn_last_error(), (name, v)
        with pytest.raises(B.CtpnError):
            B.text_lines(sc.rois[:, 1:5], sc.rois[:, 0], (sc.h, sc.w), "H", device_id=-1, config=cfg8)
    for name, v in (("MAX_HORIZONTAL_GAP", 0.0), ("MAX_HORIZONTAL_GAP", 4096.0), ("TEXT_PROPOSALS_NMS_THRESH", 0.0), ("TEXT_PROPOSALS_NMS_THRESH", 1.0),
                    ("LINE_MIN_SCORE", -5.0), ("MIN_LINE_WIDTH", 0.0)):
        cfg8 = T.cfg8({})
        cfg8[idx[name]] = v
        assert _raw_text_lines(sc, 0, cfg8)[0] == 0, (name, v)


def test_text_detector_with_a_configuration_of_its_own():
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.text_connector.detectors import TextDetector
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config

    class Sub(Config):
        LINE_MIN_SCORE = 0.8
        MAX_HORIZONTAL_GAP = 90
        TEXT_PROPOSALS_WIDTH = 32          # x MIN_NUM_PROPOSALS 2: a minimum width of 64

    edit = {"LINE_MIN_SCORE": 0.8, "MAX_HORIZONTAL_GAP": 90, "MIN_LINE_WIDTH": 64}
    assert np.array_equal(B.connector_cfg8(Sub), T.cfg8(edit)) and np.array_equal(B.connector_cfg8(edit), T.cfg8(edit))
    keep = cfg.USE_GPU_NMS
    cfg.USE_GPU_NMS = False
    try:
        for mode in "HO":
            cfg.TEST.DETECT_MODE = mode
            det, plain = TextDetector(config=Sub), TextDetector()
            for name, sc in SCENES.items():
                got = det.detect(sc.rois[:, 1:5], sc.rois[:, 0:1], (sc.h, sc.w))
                assert_lines_close(got, T.oracle_lines(sc, mode, edit), (name, mode))
                assert_lines_close(plain.detect(sc.rois[:, 1:5], sc.rois[:, 0:1], (sc.h, sc.w)), default_oracle(name, mode), (name, mode))
        # the module-level Config is still not a way in: the error stays, and now says where to go
        Config.LINE_MIN_SCORE = 0.8
        try:
            with pytest.raises(ValueError) as e:
                TextDetector()
            assert "compiled in" in str(e.value) and "TextDetector(config=" in str(e.value)
            TextDetector(config=Sub)                       # ... while an explicit configuration does not look at it
        finally:
            Config.LINE_MIN_SCORE = 0.9
        with pytest.raises(B.CtpnError):
            TextDetector(config={"TEXT_PROPOSALS_NMS_THRESH": -0.2})
        with pytest.raises(ValueError):
            TextDetector(config={"LINE_MIN_SCOER": 0.8})
    finally:
        cfg.USE_GPU_NMS = keep


def test_batch_demo_connector_argument(capsys):
    from ctpn_amd.ctpn import demo_batch
    ap = demo_batch.build_parser()
    assert ap.parse_args([]).connector == []
    args = ap.parse_args(["--connector", "LINE_MIN_SCORE=0.8", "--connector", "MAX_HORIZONTAL_GAP=70"])
    assert demo_batch.parse_connector_args(args.connector) == {"LINE_MIN_SCORE": 0.8, "MAX_HORIZONTAL_GAP": 70.0}
    for bad in ("LINE_MIN_SCOER=0.8", "RPN_NMS_THRESH=0.5", "LINE_MIN_SCORE", "LINE_MIN_SCORE=high"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--connector", bad])
    capsys.readouterr()
    assert demo_batch.rpn_params_from_cfg() == {"RPN_PRE_NMS_TOP_N": 12000, "RPN_POST_NMS_TOP_N": 1000, "RPN_NMS_THRESH": 0.7, "RPN_MIN_SIZE": 8.0}
    # cfg.TEST.RPN_* that differ from what the ctx is going to run with are still an error; carried in params they are not
    from ctpn_amd.lib.fast_rcnn.config import cfg
    keep = cfg.TEST.RPN_POST_NMS_TOP_N
    cfg.TEST.RPN_POST_NMS_TOP_N = 300
    try:
        with pytest.raises(ValueError):
            demo_batch._check_uint8_feed_config()
        demo_batch._check_uint8_feed_config(demo_batch.rpn_params_from_cfg())
    finally:
        cfg.TEST.RPN_POST_NMS_TOP_N = keep


def test_batch_demo_sets_the_run_parameters_on_the_ctx():
    """run(params=...) writes every tail parameter into the run's ctx (params over the defaults); a later run without params puts the
    defaults back; a net that never had parameters set is not touched"""
    from ctpn_amd.ctpn import demo_batch

    class Ctx:
        def __init__(self):
            self.calls = {}

        def set_param(self, name, value):
            self.calls[name] = value

    class Net:
        pass

    net = Net()
    net.ctx = Ctx()
    demo_batch._set_tail_params(net, None)
    assert net.ctx.calls == {}
    demo_batch._set_tail_params(net, {"RPN_POST_NMS_TOP_N": 300, "LINE_MIN_SCORE": 0.8})
    want = {n: B.param_default(n) for n in B.param_names()}
    assert net.ctx.calls == dict(want, RPN_POST_NMS_TOP_N=300, LINE_MIN_SCORE=0.8)
    net.ctx = Ctx()                                    # ensure_capacity replaced the ctx
    demo_batch._set_tail_params(net, None)
    assert net.ctx.calls == want
    net.ctx = Ctx()
    demo_batch._set_tail_params(net, None)
    assert net.ctx.calls == {}
