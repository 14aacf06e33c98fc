"""CPU: the label side of training (include/ctpn_hip.h, "anchor targets and the RPN loss") without a device.
  * tests/anchor_target_ref.py, the independent numpy restatement, against tests/golden/anchor_targets.npz, which holds what the reference's
    unmodified anchor_target_layer gave (tools/make_anchor_target_golden.py): labels before sampling exact, bbox_targets dx / dy bit for bit
    and dw / dh within 1 float32 ulp (log in double may differ in its last bit between libraries), weights exact on unsampled scenes; on
    sampled scenes every anchor the reference kept carries the restatement's presample label and the counts after sampling agree; the
    restatement's sampled set obeys the splitmix rule;
  * csrc/targets_dev.h, the kernels' per-thread text, compiled with g++ under ASan + UBSan as a stand-alone program (tests/targets_host.cpp)
    and run as a subprocess over every thread of every scene, from exact-size heap blocks, against the restatement to the same bounds;
  * the four symbols in header, library and binding; ABI version 10; bad arguments refused; no device: CTPN_ERR_NODEVICE, not a CPU fallback;
    the label parser of ctpn/score_pages.py; ctpn_target_config_default equals the reference's cfg as the fixture recorded it."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import anchor_target_ref as R
import ctpn_amd
from ctpn_amd import _binding as B

GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "anchor_targets.npz"))


def scene_names(golden_dir=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")):
    return [str(s) for s in np.load(os.path.join(golden_dir, "anchor_targets.npz"))["scenes"]]


SCENES = scene_names()
SAMPLED = ("zero_overlap_box", "rows_sampled", "map_37x56", "non_integer", "two_dontcare_hard")


def scene(golden, name):
    p = name + "/"
    s = {k[len(p):]: golden[k] for k in golden.files if k.startswith(p)}
    s["hf"], s["wf"] = int(s["map"][0]), int(s["map"][1])
    s.setdefault("hard", None)
    s.setdefault("dontcare", None)
    return s


_REF = {}


def restated(golden, name, batch=None, seed=0):
    """the restatement of a scene, computed once per (scene, batch, seed) and shared; never modified"""
    key = (name, batch, seed)
    if key not in _REF:
        s = scene(golden, name)
        cfg = s["cfg12"].copy()
        if batch is not None:
            cfg[4] = batch
        _REF[key] = R.anchor_targets(s["hf"], s["wf"], s["im_info"], s["gt"], s["hard"], s["dontcare"], cfg, seed)
    return _REF[key]


def ulp_distance(a, b):
    """float32 arrays -> distance in units of the last place (ordered-integer form)"""
    def o(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(o(a) - o(b))


def check_targets_against(got, want_targets, what):
    """dx / dy bit for bit, dw / dh within 1 ulp"""
    got = np.asarray(got, np.float32).reshape(-1, 4)
    want = np.asarray(want_targets, np.float32).reshape(-1, 4)
    assert np.array_equal(got[:, :2].view(np.int32), want[:, :2].view(np.int32)), what + ": dx / dy differ in bits"
    assert ulp_distance(got[:, 2:], want[:, 2:]).max() <= 1, what + ": dw / dh differ by more than 1 ulp"


def test_fixture_is_small_and_complete(golden, golden_dir):
    sizes = {f: os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir)}
    assert sizes["anchor_targets.npz"] < max(v for k, v in sizes.items() if k != "anchor_targets.npz")
    assert len(SCENES) >= 12 and set(SAMPLED) <= set(SCENES)
    assert {"three", "zero_overlap_box", "hard_strip", "dontcare", "rows_sampled", "map_37x56", "clobber", "thresholds_half", "hard_not_precluded", "inside_ones",
            "non_integer", "short_image"} <= set(SCENES)
    # what the reference gave on the probe scenes: the column-maximum quirk makes every zero-overlap anchor foreground
    pre = {n: golden[n + "/labels_presample"] for n in SCENES}
    assert ((pre["three"] == 1).sum(), (pre["three"] == 0).sum()) == (6, 173)
    assert (pre["zero_overlap_box"] == 0).sum() == 0 and (pre["zero_overlap_box"] == 1).sum() > 150
    assert (golden["zero_overlap_box/labels"] == 1).sum() == 150
    # CLOBBER = 1 on that scene: the bg rule, applied last, takes the column-maximum foreground back wherever the overlap is below NEGATIVE
    assert np.array_equal(golden["clobber/gt"], golden["zero_overlap_box/gt"]) and golden["clobber/cfg12"][2] == 1 and golden["zero_overlap_box/cfg12"][2] == 0
    assert not np.array_equal(pre["clobber"], pre["zero_overlap_box"]) and ((pre["clobber"] == 1).sum(), (pre["clobber"] == 0).sum()) == (35, 173)
    assert (pre["hard_strip"] == 1).sum() == 4 and ((pre["dontcare"] == 1).sum(), (pre["dontcare"] == 0).sum()) == (0, 104)


@pytest.mark.parametrize("name", SCENES)
def test_restatement_equals_the_reference(golden, name):
    s = scene(golden, name)
    r = restated(golden, name, batch=0)
    assert np.array_equal(r["labels_presample"], s["labels_presample"])
    assert np.array_equal(r["labels"], s["labels_presample"])                  # RPN_BATCHSIZE 0: nothing is sampled
    if "bbox_targets" in s:
        check_targets_against(r["bbox_targets"], s["bbox_targets"], name)
    else:
        assert hashlib.sha256(np.ascontiguousarray(r["bbox_targets"]).tobytes()).digest() == s["targets_sha256"].tobytes()
    sampled = not np.array_equal(s["labels"], s["labels_presample"])
    assert sampled == (name in SAMPLED)
    q = restated(golden, name, seed=int(s["np_seed"]))                          # the scene's own RPN_BATCHSIZE (300)
    if not sampled:
        assert np.array_equal(q["labels"], s["labels"])
        assert np.array_equal(q["inside_weights"], s["inside_weights"]) and np.array_equal(q["outside_weights"], s["outside_weights"])
    else:
        kept = s["labels"] != -1
        assert np.array_equal(s["labels"][kept], r["labels_presample"][kept])  # the reference disabled, it never relabelled
        for cls in (0, 1):
            assert (q["labels"] == cls).sum() == (s["labels"] == cls).sum(), cls
        # the weights follow the reference's own labels
        assert np.array_equal(s["inside_weights"][s["labels"] == 1], np.tile(s["cfg12"][7:11].astype(np.float32), ((s["labels"] == 1).sum(), 1)))
    assert q["stats"][3] == (q["labels"] == 1).sum() and q["stats"][4] == (q["labels"] == 0).sum()


def test_splitmix_key_and_rule(golden):
    # splitmix64 seeded with 0: its first output is the finaliser of the golden-ratio increment
    assert int(R.keys(0x9E3779B97F4A7C15, 0, [0])[0]) == 0xE220A8397B1DCDAF
    assert int(R.keys(0, 0, [0])[0]) == 0
    assert R.keys(7, 1, [5])[0] != R.keys(7, 0, [5])[0] and R.keys(7, 0, [5])[0] != R.keys(8, 0, [5])[0]
    for name in ("rows_sampled", "zero_overlap_box"):
        for seed in (0, 1, 0xDEADBEEFCAFEF00D):
            r, pre = restated(golden, name, seed=seed), restated(golden, name, batch=0)["labels"]
            for cls, keep in ((1, 150), (0, 300 - min(150, int((pre == 1).sum())))):
                idx = np.nonzero(pre == cls)[0]
                k = R.keys(seed, 0, idx)
                kept = r["labels"][idx] == cls
                assert kept.sum() == min(keep, len(idx))
                assert np.all(r["labels"][idx][~kept] == -1)
                if kept.sum() < len(idx):
                    assert k[kept].max() < k[~kept].min()      # the smallest keys stay
            other = np.nonzero((pre != 0) & (pre != 1))[0]
            assert np.all(r["labels"][other] == -1)
    a, b = restated(golden, "rows_sampled", seed=0)["labels"], restated(golden, "rows_sampled", seed=1)["labels"]
    assert not np.array_equal(a, b)


# ---- targets_dev.h under the sanitizers ----
@pytest.fixture(scope="module")
def exe(root, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("targets_host") / "targets_host")
    subprocess.run(GXX + ["-o", path, os.path.join(root, "tests", "targets_host.cpp")], check=True)
    return path


def run_host(exe, tmp_path, what, payload):
    (tmp_path / "in.bin").write_bytes(payload)
    r = subprocess.run([exe, what, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.stderr == "", r.stderr[-3000:]                                                    # the sanitizers are silent
    assert r.returncode == 0, r.stdout[-2000:]
    return (tmp_path / "out.bin").read_bytes()


def seeded_heads(cells, ld, seed):
    rng = np.random.default_rng(seed)
    h = np.zeros((cells, ld), np.float32)
    h[:, :40] = (rng.standard_normal((cells, 40)) * 0.5).astype(np.float32)
    h[:, 40:60] = (rng.standard_normal((cells, 20)) * 3.0).astype(np.float32)
    if ld > 60:
        h[:, 60:] = np.nan
    return h


def host_scene(exe, tmp_path, s, cfg, seed, image, ld, heads):
    G = s["gt"].shape[0]
    D = 0 if s["dontcare"] is None else s["dontcare"].shape[0]
    payload = struct.pack("<7iQ", s["hf"], s["wf"], G, D, 0 if s["hard"] is None else 1, ld, image, seed & 0xFFFFFFFFFFFFFFFF)
    payload += np.asarray(s["im_info"], np.float32).tobytes() + np.asarray(cfg, np.float64).tobytes() + np.asarray(s["gt"], np.float32).tobytes()
    if s["hard"] is not None:
        payload += np.asarray(s["hard"], np.int32).tobytes()
    if D:
        payload += np.asarray(s["dontcare"], np.float32).tobytes()
    payload += np.asarray(heads, np.float32).tobytes()
    raw = run_host(exe, tmp_path, "scene", payload)
    N, cells = s["hf"] * s["wf"] * 10, s["hf"] * s["wf"]
    out, off = {}, 0
    for key, dt, cnt in (("labels", np.float32, N), ("labels_presample", np.float32, N), ("bbox_targets", np.float32, N * 4), ("inside_weights", np.float32, N * 4),
                         ("outside_weights", np.float32, N * 4), ("max_overlap", np.float64, N), ("argmax", np.int32, N), ("stats", np.int32, 6),
                         ("losses", np.float64, 3), ("counts", np.int32, 2), ("d_heads", np.float32, cells * ld)):
        nb = cnt * np.dtype(dt).itemsize
        out[key] = np.frombuffer(raw[off:off + nb], dt)
        off += nb
    assert off == len(raw)
    return out


def check_targets(got, want, what):
    """a device-text result against the restatement, at the bounds of this file's docstring"""
    assert np.array_equal(np.asarray(got["labels_presample"]).reshape(-1), want["labels_presample"].astype(np.float32)), what
    assert np.array_equal(np.asarray(got["labels"]).reshape(-1), want["labels"].astype(np.float32)), what
    check_targets_against(got["bbox_targets"], want["bbox_targets"], what)
    assert np.array_equal(np.asarray(got["inside_weights"]).reshape(-1, 4), want["inside_weights"]), what
    assert np.array_equal(np.asarray(got["outside_weights"]).reshape(-1, 4), want["outside_weights"]), what
    assert np.array_equal(np.asarray(got["max_overlap"]).reshape(-1).view(np.int64), want["max_overlap"].view(np.int64)), what
    assert np.array_equal(np.asarray(got["argmax"]).reshape(-1), want["argmax"]), what
    assert np.array_equal(np.asarray(got["stats"]).reshape(-1), want["stats"]), what


def check_loss(losses, counts, d_heads, heads, t, what):
    """losses within relative 1e-10 of the float64 restatement (at most 96 000 terms, each within a few ulp of double, sum with an order error
    below K 2^-53 = 1.1e-11); counts exact; d_heads within 1 float32 ulp of autograd's gradient rounded to float"""
    ce, box, model, K, F = R.rpn_loss(heads, t["labels"], t["bbox_targets"], t["inside_weights"], t["outside_weights"])
    assert list(counts) == [K, F], what
    for got, want in zip(losses, (ce, box, model)):
        assert abs(got - want) <= 1e-10 * abs(want), (what, got, want)
    if d_heads is not None:
        _, grad = R.rpn_loss_torch(heads, t["labels"], t["bbox_targets"], t["inside_weights"], t["outside_weights"])
        d = np.asarray(d_heads, np.float32).reshape(grad.shape)
        assert ulp_distance(d[:, :60], grad[:, :60].astype(np.float32)).max() <= 1, what
        assert np.all(d[:, 60:] == 0), what


@pytest.mark.parametrize("name", SCENES)
def test_device_text_under_sanitizers_equals_the_restatement(golden, exe, tmp_path, name):
    s = scene(golden, name)
    cells = s["hf"] * s["wf"]
    for batch, seed, ld in ((0, 0, 60), (None, 12345, 64)):
        cfg = s["cfg12"].copy()
        if batch is not None:
            cfg[4] = batch
        heads = seeded_heads(cells, ld, 3)
        got = host_scene(exe, tmp_path, s, cfg, seed, 0, ld, heads)
        want = restated(golden, name, batch, seed)
        check_targets(got, want, name)
        check_loss(got["losses"], got["counts"], got["d_heads"], heads, want, name)


def test_device_text_edge_scenes(golden, exe, tmp_path):
    base = scene(golden, "three")
    heads = seeded_heads(48, 60, 1)
    # no ground truth; a tiny batch (both classes sampled, fg to 2 of 6); image index 2 changes the keys; a hard box that overlaps nothing
    for what, gt, hard, cfgmod, image in (("G0", np.zeros((0, 5), np.float32), None, {}, 0), ("tiny batch", base["gt"], None, {4: 5.0}, 0),
                                          ("image 2", base["gt"], None, {4: 5.0}, 2),
                                          ("far hard", np.vstack([base["gt"], [[200, 200, 215, 230, 1]]]).astype(np.float32), [0, 0, 0, 1], {4: 0.0}, 0)):
        s = dict(base, gt=gt, hard=None if hard is None else np.array(hard, np.int32))
        cfg = base["cfg12"].copy()
        for k, v in cfgmod.items():
            cfg[k] = v
        got = host_scene(exe, tmp_path, s, cfg, 9, image, 60, heads)
        want = R.anchor_targets(s["hf"], s["wf"], s["im_info"], s["gt"], s["hard"], None, cfg, 9, image)
        check_targets(got, want, what)
        check_loss(got["losses"], got["counts"], got["d_heads"], heads, want, what)
        if what == "far hard":
            first = np.nonzero(want["argmax"] >= 0)[0][0]
            assert want["labels"][first] == -1 and got["labels"][first] == -1          # the first inside anchor, at overlap 0
    # settings no fixture scene moves: FG_FRACTION 0 (every fg anchor disabled: the select's keep <= 0 branch) and 0.25, a dontcare threshold
    # of 0.75 and of 0.9 on an area that covers a column of anchors by 13 / 16, CLOBBER on the zero-overlap box under sampling
    far4 = np.vstack([base["gt"], [[200, 200, 215, 230, 1]]]).astype(np.float32)
    dc = np.array([[0, 0, 60, 95]], np.float32)
    seen = {}
    for what, gt, dcs, cfgmod in (("fraction 0", base["gt"], None, {3: 0.0, 4: 20.0}), ("fraction 0.25", far4, None, {3: 0.25, 4: 40.0}),
                                  ("dc_hi 0.75", base["gt"], dc, {5: 0.75, 4: 0.0}), ("dc_hi 0.9", base["gt"], dc, {5: 0.9, 4: 0.0}),
                                  ("clobber", far4, None, {2: 1.0, 4: 50.0}), ("no clobber", far4, None, {2: 0.0, 4: 50.0})):
        s = dict(base, gt=gt, dontcare=dcs)
        cfg = base["cfg12"].copy()
        for k, v in cfgmod.items():
            cfg[k] = v
        got = host_scene(exe, tmp_path, s, cfg, 9, 0, 60, heads)
        want = R.anchor_targets(s["hf"], s["wf"], s["im_info"], gt, None, dcs, cfg, 9, 0)
        check_targets(got, want, what)
        check_loss(got["losses"], got["counts"], got["d_heads"], heads, want, what)
        seen[what] = want
    assert seen["fraction 0"]["stats"][1] == 6 and seen["fraction 0"]["stats"][3] == 0 and seen["fraction 0"]["stats"][4] == 20
    assert seen["fraction 0.25"]["stats"][3] == 10 and seen["fraction 0.25"]["stats"][1] > 150
    assert seen["dc_hi 0.75"]["stats"][5] > seen["dc_hi 0.9"]["stats"][5] > 0
    assert not np.array_equal(seen["clobber"]["labels_presample"], seen["no clobber"]["labels_presample"])
    a = R.anchor_targets(6, 8, base["im_info"], base["gt"], None, None, [0.3, 0.7, 0, 0.5, 5, 0.5, 1, 0, 1, 0, 1, -1], 9, 0)
    b = R.anchor_targets(6, 8, base["im_info"], base["gt"], None, None, [0.3, 0.7, 0, 0.5, 5, 0.5, 1, 0, 1, 0, 1, -1], 9, 2)
    assert not np.array_equal(a["labels"], b["labels"])


def overlap_cases():
    rng = np.random.default_rng(2)
    b = rng.integers(0, 200, (65, 4)).astype(np.float64)
    b[:, 2:] += b[:, :2]
    q = rng.integers(0, 200, (257, 4)).astype(np.float64) * 0.7324
    q[:, 2:] += q[:, :2]
    edge_b = np.array([[0, 0, 15, 15], [0, 0, 15, 15], [16, 0, 31, 15], [15, 0, 30, 15], [0.5, 0.25, 10.75, 3.125]], np.float64)
    edge_q = np.array([[0, 0, 15, 15], [15, 15, 20, 20], [16, 16, 20, 20], [0, 0, 7, 10], [-5, -5, -1, -1]], np.float64)
    return [(b, q), (edge_b, edge_q), (b[:1], q[:1]), (b[:17], q[:256])]


def test_overlap_text_under_sanitizers_is_bit_equal(exe, tmp_path):
    for b, q in overlap_cases():
        for inter in (0, 1):
            raw = run_host(exe, tmp_path, "overlaps", struct.pack("<3i", len(b), len(q), inter) + b.tobytes() + q.tobytes())
            got = np.frombuffer(raw, np.float64).reshape(len(b), len(q))
            assert np.array_equal(got.view(np.int64), R.overlaps(b, q, bool(inter)).view(np.int64))
    o = R.overlaps(*overlap_cases()[1])
    assert o[0, 0] == 1.0 and o[0, 1] == 1.0 / (256 + 36 - 1) and o[0, 2] == 0.0 and o[0, 3] == 88.0 / 256 and o[0, 4] == 0.0


# ---- plumbing ----
NEW = ("ctpn_target_config_default", "ctpn_bbox_overlaps", "ctpn_anchor_targets", "ctpn_rpn_loss")


def test_symbols_in_header_library_and_binding(root):
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    lib = B.load_library()
    declared = B._declare(C.CDLL(B.lib_path()))
    for name in NEW:
        assert name + "(" in hdr and hasattr(lib, name) and name in declared
    assert lib.ctpn_abi_version() == 10 and "#define CTPN_TARGET_CFG_DOUBLES 12" in hdr
    assert "ctpn_ctx" not in "".join(line for line in hdr.splitlines() if any(n + "(" in line for n in NEW))


def test_default_config_is_the_references(golden):
    assert np.array_equal(ctpn_amd.target_config_default(), golden["cfg12"])
    assert np.array_equal(golden["cfg12"], np.array(R.DEFAULT_CFG))
    assert B.load_library().ctpn_target_config_default(None) == -1


def test_bad_arguments_and_no_device():
    lib = B.load_library()
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int)
    one = np.zeros((4,), np.float64)
    assert lib.ctpn_bbox_overlaps(0, None, 0, None, 5, None, 0) == 0                     # n = 0: nothing to do, nothing written
    assert lib.ctpn_bbox_overlaps(0, one.ctypes.data_as(f64p), 1, one.ctypes.data_as(f64p), 0, None, 1) == 0
    assert lib.ctpn_bbox_overlaps(0, None, 1, None, 1, None, 0) == -1
    assert lib.ctpn_bbox_overlaps(0, one.ctypes.data_as(f64p), 1, one.ctypes.data_as(f64p), 1, one.ctypes.data_as(f64p), 2) == -1
    info = np.array([[96, 128, 1]], np.float32)
    gt = np.array([[16, 20, 31, 50, 1]], np.float32)
    N = 6 * 8 * 10
    lab, t, wi, wo, stats = np.zeros(N, np.float32), np.zeros(N * 4, np.float32), np.zeros(N * 4, np.float32), np.zeros(N * 4, np.float32), np.zeros(6, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def targets(offs=(0, 1), cfg=None, hf=6, wf=8, labels=lab, gtp=gt):
        o = np.array(offs, np.int32)
        c = None if cfg is None else np.array(cfg, np.float64).ctypes.data_as(f64p)
        return lib.ctpn_anchor_targets(0, 1, hf, wf, info.ctypes.data_as(C.POINTER(C.c_float)), None if gtp is None else vp(gtp), o.ctypes.data_as(i32p), None, None,
                                       None, c, 0, 0, None if labels is None else vp(labels), vp(t), vp(wi), vp(wo), stats.ctypes.data_as(i32p), None, None, None)

    d = list(R.DEFAULT_CFG)
    assert targets(labels=None) == -1 and targets(gtp=None) == -1
    assert targets(offs=(1, 2)) == -1 and targets(offs=(0, -1)) == -1
    assert b"gt_offsets" in lib.ctpn_last_error()
    assert targets(hf=4096, wf=4096) == -1
    for i, v in ((0, 1.5), (1, -0.1), (1, float("nan")), (4, -1.0), (4, 2.5), (3, 2.0)):
        bad = list(d)
        bad[i] = v
        assert targets(cfg=bad) == -1, (i, v)
    bad = list(d)
    bad[11] = 0.5
    assert targets(cfg=bad) == -6 and b"RPN_POSITIVE_WEIGHT" in lib.ctpn_last_error()
    losses, counts, heads = np.zeros(3, np.float64), np.zeros(2, np.int32), np.zeros((48, 64), np.float32)

    def loss(ld=64, h=heads, hf=6):
        return lib.ctpn_rpn_loss(0, 1, hf, 8, None if h is None else vp(h), ld, vp(lab), vp(t), vp(wi), vp(wo), 0, losses.ctypes.data_as(f64p), counts.ctypes.data_as(i32p), None)

    assert loss(ld=61) == -1 and loss(h=None) == -1 and loss(hf=0) == -1
    if B.device_count() > 0:
        return
    assert targets() == -5 and b"no CPU fallback" in lib.ctpn_last_error()
    assert loss() == -5 and b"no CPU fallback" in lib.ctpn_last_error()
    with pytest.raises(ctpn_amd.CtpnError) as e:
        ctpn_amd.bbox_overlaps(np.zeros((1, 4)), np.zeros((1, 4)))
    assert e.value.code == -5 and "no CPU fallback" in str(e.value)


def test_label_file_parser(tmp_path):
    from ctpn_amd.ctpn import score_pages as S
    p = tmp_path / "img_1.txt"
    p.write_text("text\t16\t20\t31\t50\ntext\t32\t22\t47\t52\n\n")
    assert np.array_equal(S.read_labels(str(p)), np.array([[16, 20, 31, 50], [32, 22, 47, 52]], np.float32))
    assert np.array_equal(S.scale_boxes(S.read_labels(str(p)), 0.5), np.array([[8, 10, 15.5, 25], [16, 11, 23.5, 26]], np.float32))
    (tmp_path / "empty.txt").write_text("")
    assert S.read_labels(str(tmp_path / "empty.txt")).shape == (0, 4)
    bad = tmp_path / "bad.txt"
    bad.write_text("text\t1\t2\t3\t4\ntext 1 2 3 4\n")
    with pytest.raises(ValueError) as e:
        S.read_labels(str(bad))
    assert "bad.txt:2" in str(e.value)
    (tmp_path / "gt_img_2.txt").write_text("text\t0\t0\t15\t15\n")
    assert S.label_path(str(tmp_path), "/x/img_1.jpg") == str(p) and S.label_path(str(tmp_path), "/x/img_2.png") == str(tmp_path / "gt_img_2.txt")
    assert S.label_path(str(tmp_path), "/x/img_3.png") is None


def test_mirrors_have_the_references_signatures():
    import inspect
    from ctpn_amd.lib.rpn_msr import anchor_target_layer_tf as M
    from ctpn_amd.lib.utils import bbox as X
    assert list(inspect.signature(M.anchor_target_layer).parameters) == ["rpn_cls_score", "gt_boxes", "gt_ishard", "dontcare_areas", "im_info", "_feat_stride", "anchor_scales"]
    assert list(inspect.signature(X.bbox_overlaps).parameters) == ["boxes", "query_boxes"] == list(inspect.signature(X.bbox_intersections).parameters)
