"""CPU: RPN_POST_NMS_TOP_N above 1000 (ctpn_reserve_proposals) before it reaches a GPU.
  (a) the dense pages of tests/dense_pages.py cross the boundaries they are meant to cross (the oracle's counts), and the launch plans
      (ctpn_debug_text_line_plan, ctpn_debug_proposal_plan: pure functions) change form exactly at the seams;
  (b) the large connector's per-thread source text (csrc/connect_dev.h), compiled with g++ under AddressSanitizer + UBSan into a stand-alone
      program (tests/connect_host.cpp) and run as a subprocess, gives csrc/text_connector.cpp's records byte for byte and the oracle's under
      the comparison of tests/test_gpu_text_line_tail.py;
  (c) the Python layer sizes its arrays by the ctx's capacity and refuses more than 4096."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_pages as D  # noqa: E402
import util  # noqa: E402

from ctpn_amd import _binding as B  # noqa: E402
from oracle import postproc as P  # noqa: E402

SEAMS = (1000, 1001, 1024, 1025, 4096)


# ---- (a) the inputs and the plans ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,slices,at_1000,at_4096", [("40x64", 2560, 171, 40), ("40x64/2", 1280, 36, 20), ("24x48", 1152, 25, 24), ("64x64", 4096, 238, 64)])
def test_the_pages_cross_the_boundaries(name, slices, at_1000, at_4096):
    """slices with score > 0.7, lines (mode H) at the cap of 1000 and at 4096, on the CPU oracle: the pages hold more than 1000 line slices,
    a top-N of 1000 breaks their lines into fragments, 4096 gives one line per text row"""
    assert D.slices_above(name) == slices
    assert D.oracle_lines(name, 1000).shape[0] == at_1000
    assert D.oracle_lines(name, 4096).shape[0] == at_4096


def test_the_page_beyond_every_capacity():
    assert D.oracle_rois("65x64").shape[0] == 4096 and D.slices_above("65x64") == 4096      # 4160 text slices: the first 4096 in rank order


@pytest.mark.parametrize("name", D.GOLDEN_PAGES)
def test_the_oracle_equals_the_reference_at_4096(name):
    """tests/golden/dense_pages.npz: the reference's own proposal_layer and TextDetector with cfg.TEST.RPN_POST_NMS_TOP_N = 4096"""
    g = D.golden()
    assert int(g["post_nms_topn"]) == 4096
    # (rows of equal score: the reference leaves their order to numpy's unstable argsort, the oracle and the library order them by index)
    want, got = util.canon_rows(g["rois_" + name]), util.canon_rows(D.oracle_rois(name))
    assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0]) and np.abs(got - want).max() < 1e-3
    for mode in "HO":
        want, got = g["recs_%s_%s" % (mode, name)], D.oracle_lines(name, 4096, mode)
        assert got.shape == want.shape and np.array_equal(got[:, 8], want[:, 8]) and np.allclose(got[:, :8], want[:, :8], rtol=3e-7, atol=1e-5)


def test_text_line_plan_at_the_seams():
    for rows in SEAMS:
        large = rows > 1024
        for n in (1, 4, 5, 32):
            spread = n <= 4
            assert B.text_line_plan(n, 64, rows)[0] == ("one_wg_large" if large else "column_groups" if spread else "one_wg"), (rows, n)
            assert B.text_line_plan(n, 64, rows, nms_columns=2)[0] == ("one_wg_large" if large else "one_wg")
            assert B.text_line_plan(n, 64, rows, nms_columns=3)[0] == ("one_wg_large" if large else "column_groups")
            assert B.text_line_plan(n, 64, rows, mw_scratch=False)[0] == ("one_wg_large" if large else "one_wg")
            assert B.text_line_plan(n, 64, rows, nms_columns=0)[0] == "generic"
            assert B.text_line_plan(n, 64, rows)[2] == (16 if spread and not large else 0)
        # the column forms' other conditions hold above 1024 rows as below: threshold, scale, columns -- the generic kernel is the fallback
        assert B.text_line_plan(1, 64, rows, thresh=0.1)[0] == "generic"
        assert B.text_line_plan(1, 64, rows, max_scale=4.5)[0] == "generic"
        assert B.text_line_plan(1, 257, rows)[0] == "generic" and B.text_line_plan(1, 256, rows)[0] != "generic"
        assert B.text_line_plan(1, 64, rows, connect_device=0)[1] == "host"
        assert B.text_line_plan(1, 64, rows, connect_device=1)[1] == ("buckets" if large else "all_pairs")
    for bad in (dict(rows=0), dict(rows=4097), dict(n=0), dict(wf=0), dict(nms_columns=4)):
        kw = dict(n=1, wf=64, rows=1000)
        kw.update(bad)
        with pytest.raises(B.CtpnError):
            B.text_line_plan(**kw)


def test_proposal_plan_at_the_seams():
    """post_nms_topn up to 4096: the plan's slots are those of post = 1000, but for slot [8] -- the prefix pass is asked for up to 1024 and
    skipped above (the 4096 best-scored ranks would rarely hold that many survivors: it would run twice)"""
    for n in (1, 4, 5, 32):
        for cols in (0, 1, 2, 3):
            base = B.proposal_plan_sweep(n, 30, 12, 40, 30, post=1000, nms_columns=cols)
            for post in SEAMS:
                got = B.proposal_plan_sweep(n, 30, 12, 40, 30, post=post, nms_columns=cols)
                assert np.array_equal(got[..., :8], base[..., :8]), (n, cols, post)
                assert np.array_equal(got[..., 8], base[..., 8] if post <= 1024 else np.zeros_like(base[..., 8])), (n, cols, post)
            assert np.array_equal(B.proposal_plan_sweep(n, 30, 12, 40, 30, post=4096, nms_columns=cols, nms_prefix=0), got)
    assert B.proposal_plan(8, 40, 64, post=1024).prefix != B.proposal_plan(8, 40, 64, post=1025).prefix


# ---- (b) the large connector's bodies on the CPU ---------------------------------------------------------------------------------------
def kept(rois, scale=1.0):
    """the connector's input for an image's rois: the score > 0.7 prefix, boxes / scale, the oracle's NMS 0.2 -- rows in rank order"""
    s = rois[:, 0]
    m = int(np.count_nonzero(s > np.float32(0.7)))
    d = np.hstack([rois[:m, 1:5] / np.float32(scale), s[:m, None]]).astype(np.float32)
    k = P.nms(d, 0.2) if m else []
    return d[k, :4].copy(), d[k, 4].copy()


def tie_page():
    """two equal scores in one pixel column: the successor of the box at x = 0 is the FIRST of them in index order (np.argmax). Each of the two
    continues in a line of its own, so the other choice gives other records. Boxes of 56 rows that overlap the 40-row box by 29 rows (0.725 of
    the smaller height, heights 40 / 56 = 0.714 alike) and each other by 18 (IoU 0.19: both survive the NMS)."""
    rows = [(0.99, 0, 100, 139), (0.98, 16, 73, 128), (0.98, 16, 111, 166), (0.97, 32, 73, 128), (0.96, 32, 111, 166), (0.95, 48, 73, 128), (0.94, 48, 111, 166)]
    return np.array([[s, x, y1, x + 15, y2] for s, x, y1, y2 in rows], np.float32), (256, 128)


def one_column_page(n=1200):
    """every proposal in one pixel column (stacked 11-row boxes): nobody has a neighbour column, no line"""
    y = 12.0 * np.arange(n)
    r = np.stack([np.linspace(0.999, 0.93, n), np.full(n, 32.0), y, np.full(n, 47.0), y + 10.0], axis=1).astype(np.float32)
    return r, (12 * n + 16, 96)


def three_column_page(lines=500):
    """`lines` lines of three slices each, 1500 proposals: many short chains (the record capacity is proposals / 2)"""
    rows = []
    for k in range(lines):
        for c in range(3):
            rows.append((0.999 - 1e-4 * (3 * k + c) / 3.0, 16.0 * c + 16.0, 12.0 * k, 16.0 * c + 31.0, 12.0 * k + 10.0))
    r = np.array(rows, np.float32)
    return r[np.argsort(-r[:, 0], kind="stable")], (12 * lines + 16, 96)


CASES = {}      # name -> (rois, (im_h, im_w), gap)


def _cases():
    if CASES:
        return CASES
    for name in ("40x64", "40x64/2", "24x48", "64x64"):
        p = D.PAGES[name]
        CASES[name] = (D.oracle_rois(name), (16 * p.hf, 16 * p.wf), 50)
    r64 = D.oracle_rois("64x64")
    CASES["n1025"] = (r64[:1025], (1024, 1024), 50)
    CASES["n4096"] = (r64[:4096], (1024, 1024), 50)
    CASES["gap0"] = (D.oracle_rois("24x48"), (384, 768), 0)
    CASES["gap4096"] = (D.oracle_rois("24x48"), (384, 768), 4096)
    CASES["tie"] = tie_page() + (50,)
    CASES["one_column"] = one_column_page() + (50,)
    CASES["three_columns"] = three_column_page() + (50,)
    CASES["empty"] = (np.zeros((0, 5), np.float32), (64, 64), 50)
    return CASES


@pytest.fixture(scope="module")
def host(root, tmp_path_factory):
    """tests/connect_host.cpp under the sanitizers, run once on every case -> (process, {name: (records H, records O)})"""
    d = tmp_path_factory.mktemp("connect_host")
    exe, fin, fout = str(d / "connect_host"), str(d / "cases.bin"), str(d / "records.bin")
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(root, "tests", "connect_host.cpp")], check=True)
    cases = _cases()
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for name, (rois, size, gap) in cases.items():
            b, s = kept(rois)
            f.write(struct.pack("<iiiif", b.shape[0], size[0], size[1], gap, 1.0))
            f.write(np.ascontiguousarray(b, np.float32).tobytes())
            f.write(np.ascontiguousarray(s, np.float32).tobytes())
    proc = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    out = {}
    if os.path.exists(fout):
        raw = open(fout, "rb").read()
        off = 0
        for name in cases:
            if off + 8 > len(raw):
                break
            ch, co = struct.unpack_from("<ii", raw, off)
            off += 8
            h = np.frombuffer(raw, np.float64, ch * 9, off).reshape(ch, 9)
            off += ch * 72
            o = np.frombuffer(raw, np.float64, co * 9, off).reshape(co, 9)
            off += co * 72
            out[name] = (h, o)
    return proc, out


def test_the_program_is_clean_and_equals_the_host_connector_byte_for_byte(host):
    proc, out = host
    assert "AddressSanitizer" not in proc.stderr and "runtime error" not in proc.stderr, proc.stderr[-3000:]
    assert proc.returncode == 0, (proc.stdout[-3000:], proc.stderr[-3000:])
    lines = proc.stdout.splitlines()
    assert len(lines) == len(_cases()) and all(ln.startswith("ok ") for ln in lines), proc.stdout[-3000:]
    sizes = {name: int(ln.split()[2]) for name, ln in zip(_cases(), lines)}
    assert sizes["n1025"] == 1025 and sizes["n4096"] == 4096 and sizes["64x64"] == 4096 and sizes["40x64"] == 2560 and sizes["empty"] == 0
    assert sizes["one_column"] == 1200 and sizes["three_columns"] == 1500


@pytest.mark.parametrize("name", ["40x64", "40x64/2", "24x48", "64x64", "n1025", "n4096", "gap0", "gap4096", "tie", "one_column", "three_columns", "empty"])
def test_records_equal_the_oracle(host, name, monkeypatch):
    """oracle.postproc.text_detect on the same rois, under the comparison of tests/test_gpu_text_line_tail.py (count, order, scores exactly;
    coordinates rtol 3e-7 / atol 1e-5: np.polyfit on float32 data is LAPACK's float32 least squares, the product a double closed form)"""
    _, out = host
    rois, size, gap = _cases()[name]
    monkeypatch.setattr(P.Cfg, "MAX_HORIZONTAL_GAP", gap)
    for m, mode in enumerate("HO"):
        want = P.text_detect(rois[:, 1:5], rois[:, 0], size, mode)
        got = out[name][m]
        assert got.shape == want.shape, (name, mode)
        assert np.array_equal(got[:, 8], want[:, 8])
        assert np.allclose(got[:, :8], want[:, :8], rtol=3e-7, atol=1e-5)
    if name in D.GOLDEN_PAGES:      # ... and the reference's own records
        for m, mode in enumerate("HO"):
            want = D.golden()["recs_%s_%s" % (mode, name)]
            assert out[name][m].shape == want.shape and np.array_equal(out[name][m][:, 8], want[:, 8])
            assert np.allclose(out[name][m][:, :8], want[:, :8], rtol=3e-7, atol=1e-5)
    expect = {"40x64": 40, "64x64": 64, "24x48": 24, "40x64/2": 20, "gap0": 0, "one_column": 0, "three_columns": 500, "empty": 0, "tie": 2}
    if name in expect:
        assert out[name][0].shape[0] == expect[name]
    if name == "tie":      # the line through the FIRST of the two equal scores starts at x = 0
        assert out[name][0][0, 0] == 0.0 and out[name][0][0, 1] < out[name][0][1, 1] and out[name][0][1, 0] == 16.0


# ---- (c) the Python layer --------------------------------------------------------------------------------------------------------------
class FakeLib:
    """the entry points Context's array-shaped methods call: records what was asked, reports `capacity` rows as valid"""

    def __init__(self, capacity):
        self.capacity, self.reserved = capacity, []

    def ctpn_proposal_capacity(self, h, out):
        out._obj.value = self.capacity
        return 0

    def ctpn_reserve_proposals(self, h, n):
        self.reserved.append(n)
        self.capacity = n
        return 0

    def ctpn_detect(self, h, ptr, on_dev, n, hh, ww, sc, mode, recs, cap, lcnt, rois, rcnt):
        for i in range(n):
            lcnt[i] = 0
            rcnt[i] = self.capacity
        return 0

    def ctpn_detect_collect(self, h, slot, mode, recs, cap, lcnt, rois, rcnt):
        lcnt[0] = 0
        rcnt[0] = self.capacity
        return 0

    def ctpn_debug_text_lines(self, h, rois, rcnt, n, im_h, im_w, sc, mode, recs, cap, lcnt, keep, kcnt):
        self.last_roi_count = rcnt[0]
        for i in range(n):
            lcnt[i] = 0
            kcnt[i] = self.capacity
        return 0

    def ctpn_destroy(self, h):
        return 0


def fake_ctx(capacity):
    c = B.Context.__new__(B.Context)
    c._lib, c._h = FakeLib(capacity), C.c_void_p(1)
    return c


@pytest.mark.parametrize("capacity", [1000, 2048, 4096])
def test_array_shapes_follow_the_capacity(capacity):
    c = fake_ctx(capacity)
    assert c.proposal_capacity == capacity
    _, rois = c.detect(np.zeros((1, 32, 32, 3), np.uint8), want_rois=True)
    assert rois[0].shape == (capacity, 5)
    c._slot_n = {0: 1}
    _, rois = c.detect_collect(0, want_rois=True)
    assert rois[0].shape == (capacity, 5)
    _, keeps = c.debug_text_lines([np.zeros((capacity, 5), np.float32)], (64, 64))      # capacity rows fit the packed array
    assert keeps[0].shape == (capacity,) and c._lib.last_roi_count == capacity


def test_more_than_4096_is_a_value_error_that_names_the_limit():
    c = fake_ctx(1000)
    for call in (lambda: c.reserve_proposals(4097), lambda: B.reserve_for(c, 5000), lambda: B.check_post_nms_topn(4097)):
        with pytest.raises(ValueError, match="4096"):
            call()
    assert c._lib.reserved == []
    B.reserve_for(c, 1000)
    assert c._lib.reserved == []                       # within the capacity: no call
    B.reserve_for(c, 1280)
    B.reserve_for(c, 1100)
    assert c._lib.reserved == [1280] and c.proposal_capacity == 1280


def test_the_mirror_proposal_layer_refuses_more_than_4096_before_it_makes_a_ctx():
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.rpn_msr.proposal_layer_tf import proposal_layer
    cls, box, info = D.page("24x48")
    saved = cfg.TEST.RPN_POST_NMS_TOP_N
    cfg.TEST.RPN_POST_NMS_TOP_N = 4097
    try:
        with pytest.raises(ValueError, match="4096"):
            proposal_layer(cls, box, info.reshape(1, 3), "TEST")
    finally:
        cfg.TEST.RPN_POST_NMS_TOP_N = saved


def test_set_tail_params_reserves_only_above_1000():
    from ctpn_amd.ctpn import demo_batch

    class Ctx:      # (no reserve_proposals, no proposal_capacity: the ctx of a run that stays at the default)
        def __init__(self):
            self.calls = []

        def set_param(self, name, value):
            self.calls.append(("set", name, value))

    class Net:
        pass

    net = Net()
    net.ctx = Ctx()
    demo_batch._set_tail_params(net, {"RPN_POST_NMS_TOP_N": 1000})
    assert net.ctx.calls and all(c[0] == "set" for c in net.ctx.calls)

    class Big(Ctx):
        proposal_capacity = 1000

        def reserve_proposals(self, n):
            self.calls.append(("reserve", n))
            self.proposal_capacity = n

    net.ctx = Big()
    demo_batch._set_tail_params(net, {"RPN_POST_NMS_TOP_N": 4096})
    assert net.ctx.calls[0] == ("reserve", 4096) and ("set", "RPN_POST_NMS_TOP_N", 4096) in net.ctx.calls
    with pytest.raises(ValueError, match="4096"):
        demo_batch._set_tail_params(net, {"RPN_POST_NMS_TOP_N": 4097})


def test_the_cli_takes_the_top_n():
    from ctpn_amd.ctpn import demo_batch
    args = demo_batch.build_parser().parse_args(["--input", "x", "--out", "y", "--rpn-post-nms-top-n", "4096"])
    assert args.rpn_post_nms_top_n == 4096
