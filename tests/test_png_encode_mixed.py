"""CPU: the PNG writer's TABLE form (ctpn_encode_png_mixed, ctpn_write_annotated_png_files_ragged, ctpn_write_line_crops_png[_ragged]) before
it reaches a GPU. The kernels' source text, csrc/png_enc_dev.h, is compiled with g++ under AddressSanitizer + UBSan into a stand-alone
program (tests/png_enc_mixed_host.cpp) that lays the image set of tests/png_enc_ref.py out as ONE table over one exactly sized source
block -- every second image at a pitch wider than 3 w, the pads holding a sentinel --, walks every work item through pnge_locate and runs
the hist, length, scan and write passes as loops, the table listed and reversed, the write pass in both orders. Every file must equal the
library's host form (ctpn_png_encode) byte for byte with the sanitizers silent. Then the new entry points' argument checks through the C
ABI with a ctx that is never dereferenced, and demo_batch's two new keywords.

The item walk can go wrong where an image's piece count meets the group size of 256: 2x10922 is exactly one full group, 2x10923 one group
and one piece, the 255- and 256-byte streams are one piece. The listed set has no one-piece image BETWEEN two images of several groups
(its large images stand together at the end), so the table repeats two images behind the set: n255-3x28 (one piece) and flat-40x700 (two
groups) follow scan-1025x85 (five groups)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ctpn_amd  # noqa: F401
from ctpn_amd import _binding as B
import png_enc_ref as R
from test_jpeg_ragged import ENTRIES

IMAGES = R.images()
TABLE = [(k, IMAGES[k]) for k in IMAGES] + [("n255-3x28/again", IMAGES["n255-3x28"]), ("flat-40x700/again", IMAGES["flat-40x700"])]
NAMES = [k for k, _ in TABLE]
NEW_SYMBOLS = ("ctpn_encode_png_mixed", "ctpn_write_annotated_png_files_ragged", "ctpn_write_line_crops_png", "ctpn_write_line_crops_png_ragged")


def pieces(h, w):
    return (R.stream_bytes(h, w) + 255) // 256


def groups(h, w):
    return (pieces(h, w) + 255) // 256


@pytest.fixture(scope="module")
def result(root, tmp_path_factory):
    """one run of the program over the table: name -> dict(file and the printed numbers), the totals line, and its output"""
    d = tmp_path_factory.mktemp("png_enc_mixed")
    exe = str(d / "png_enc_mixed_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(root, "tests", "png_enc_mixed_host.cpp")], check=True)
    with open(d / "cases.bin", "wb") as f:
        for _, im in TABLE:
            f.write(struct.pack("<3i", im.shape[0], im.shape[1], 0) + np.ascontiguousarray(im).tobytes())
    r = subprocess.run([exe, str(d / "cases.bin"), str(d)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out, totals = {}, None
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "image":
            rec = dict(zip(t[2::2], (int(v) for v in t[3::2])))
            rec["file"] = (d / ("%d.png" % int(t[1]))).read_bytes()
            assert len(rec["file"]) == rec["bytes"]
            out[NAMES[int(t[1])]] = rec
        elif t[0] == "items":
            totals = dict(zip(t[0::2], (int(v) for v in t[1::2])))
    assert len(out) == len(TABLE) and r.stdout.splitlines()[-1] == "cases %d ok" % len(TABLE)
    return out, totals, r.stdout


def test_the_table_holds_the_shapes_at_which_the_item_walk_can_go_wrong(result):
    rec, totals, _ = result
    a = rec["2x10922"]
    assert (a["stream"], a["pieces"], a["groups"], a["far_ok"]) == (65534, 256, 1, 1)                # exactly one full group
    b = rec["2x10923"]
    assert (b["stream"], b["pieces"], b["groups"], b["far_ok"]) == (65540, 257, 2, 0)                # a second group of one piece; near matches only
    assert b["group0"] == a["group0"] + 1
    assert (rec["n255-3x28"]["stream"], rec["n255-3x28"]["pieces"]) == (255, 1)
    assert (rec["n256-1x85"]["stream"], rec["n256-1x85"]["pieces"]) == (256, 1) and (rec["n256-64x1"]["stream"], rec["n256-64x1"]["pieces"]) == (256, 1)
    g = [rec[k]["groups"] for k in NAMES]
    p = [rec[k]["pieces"] for k in NAMES]
    between = [i for i in range(1, len(g) - 1) if p[i] == 1 and g[i - 1] > 1 and g[i + 1] > 1]
    assert between == [len(g) - 2]                                  # one piece between several groups; the reversed table holds it reversed
    for (k, im), gi, pi in zip(TABLE, g, p):
        assert (pi, gi) == (pieces(*im.shape[:2]), groups(*im.shape[:2])), k
        assert rec[k]["pitch"] >= 3 * im.shape[1]
    wide = [rec[k]["pitch"] > 3 * im.shape[1] for k, im in TABLE]
    assert wide == [bool(i & 1) for i in range(len(TABLE))]         # every second image's pitch is wider than its row
    assert totals["items"] == sum(g) and totals["pieces"] == sum(p)
    # the source block is exactly the images: (h - 1) * pitch + 3 w bytes each
    assert totals["source"] == sum((im.shape[0] - 1) * rec[k]["pitch"] + 3 * im.shape[1] for k, im in TABLE)


@pytest.mark.parametrize("name", NAMES)
def test_every_file_of_the_table_is_the_host_forms(result, name):
    im = dict(TABLE)[name]
    assert result[0][name]["file"] == B.png_encode(im)
    assert np.array_equal(B.png_decode(result[0][name]["file"]), im)


def test_the_symbols_exist_and_are_bound():
    lib = B.load_library()
    assert lib.ctpn_abi_version() == 10
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ctpn_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert "int    %s(" % n in header, n


def mixed_args(n=2, h=8, w=8, pitch=24, source_bytes=None):
    src = np.zeros(n * h * pitch, np.uint8)
    hs, ws = np.full(n, h, np.int32), np.full(n, w, np.int32)
    pt, of = (C.c_size_t * n)(*([pitch] * n)), (C.c_size_t * n)(*[i * h * pitch for i in range(n)])
    bufs = np.zeros((n, 4096), np.uint8)
    out = (C.c_void_p * n)(*[bufs[i].ctypes.data for i in range(n)])
    caps, sizes = (C.c_size_t * n)(*([4096] * n)), (C.c_size_t * n)()
    keep = (src, hs, ws, bufs, pt, of, caps, sizes)
    return keep, [src.ctypes.data_as(C.c_void_p), 0, src.size if source_bytes is None else source_bytes, n, B._ptr(hs, C.c_int), B._ptr(ws, C.c_int), pt, of, out, caps, sizes]


def test_encode_png_mixed_checks_its_arguments_before_it_touches_a_device():
    """a null ctx stands behind every other check that needs no device; then a ctx that is never dereferenced: each call fails on the
    argument named, with its message and the image's index; nothing is allocated"""
    lib = B.load_library()
    fn, err = lib.ctpn_encode_png_mixed, lib.ctpn_last_error
    keep, args = mixed_args()
    assert fn(None, *args) == -1 and b"null pointer" in err() and b"ctpn_encode_png_mixed:" in err()
    fake = C.c_void_p(1)
    for k in (0, 4, 5, 6, 7, 8, 9, 10):                            # source, heights, widths, pitches, offsets, out, capacities, bytes_out
        bad = list(args)
        bad[k] = None
        assert fn(fake, *bad) == -1 and b"null pointer" in err(), k
    for n in (0, -1):
        bad = list(args)
        bad[3] = n
        assert fn(fake, *bad) == -1 and b"empty batch" in err()
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-3, 8)):
        keep, bad = mixed_args()
        keep[1][1], keep[2][1] = h, w
        assert fn(fake, *bad) == -1 and b"image 1: bad size" in err(), (h, w)
    keep, bad = mixed_args()
    keep[4][1] = 23                                                # 3 w - 1
    assert fn(fake, *bad) == -1 and b"image 1: the pitch is below 3 * width" in err()
    keep, bad = mixed_args(source_bytes=2 * 8 * 24 - 1)        # the last image's last row ends at 2 * 8 * 24: one byte short
    assert fn(fake, *bad) == -1 and b"image 1 does not lie inside source_bytes" in err()
    keep, bad = mixed_args()
    keep[5][1] = 8 * 24 + 1                                        # ... and one byte too far in
    assert fn(fake, *bad) == -1 and b"image 1 does not lie inside source_bytes" in err()
    # h (1 + 3 w) above 2^27: 65535 x 700 is 137 689 035 stream bytes. Only the check runs (a device source is not looked at before it)
    assert 65535 * (1 + 3 * 700) > 2 ** 27 >= 63882 * (1 + 3 * 700)
    keep, bad = mixed_args()
    keep[1][1], keep[2][1], keep[4][1] = 65535, 700, 2100
    bad[1] = 1
    assert fn(fake, *bad) == -1 and b"image 1: h (1 + 3 w) above 2^27" in err()


def test_the_other_three_refuse_a_null_ctx():
    lib = B.load_library()
    err = lib.ctpn_last_error
    total = C.c_int(-1)
    cnt, hts, sc = np.zeros(2, np.int32), np.array([32, 16], np.int32), np.ones(2, np.float64)
    canvas = np.zeros((2, 32, 24, 3), np.uint8)
    px = canvas.ctypes.data_as(C.c_void_p)
    keep, paths = B._path_array(["a.png", "b.png"])
    ann = [px, 0, 2, 32, 24, B._ptr(hts, C.c_int), None, 0, B._ptr(cnt, C.c_int), B._ptr(sc, C.c_double), paths]
    fn = lib.ctpn_write_annotated_png_files_ragged
    assert fn(None, *ann) == -1 and b"null pointer" in err() and b"ctpn_write_annotated_png_files_ragged:" in err()
    fake = C.c_void_p(1)
    for k in (0, 5, 8, 9, 10):                                     # canvas, heights, line_counts, scales, paths
        bad = list(ann)
        bad[k] = None
        assert fn(fake, *bad) == -1 and b"null pointer" in err(), k
    hts[1] = 15
    assert fn(fake, *ann) == -1 and b"image 1: height 15 outside 16 .. 32" in err()
    hts[1] = 16
    sc[1] = 1e-4
    assert fn(fake, *ann) == -1 and b"image 1: the resized image is empty or too large for a PNG file" in err()
    # written at 65534 x 16384: inside a file's limits, above the device form's stream limit -- refused before any device work
    big = np.zeros((1, 16, 4, 3), np.uint8)
    h1, s1, c1 = np.array([16], np.int32), np.array([16.0 / 65535.0 * 1.00001], np.float64), np.zeros(1, np.int32)
    keep1, p1 = B._path_array(["a.png"])
    assert fn(fake, big.ctypes.data_as(C.c_void_p), 0, 1, 16, 4, B._ptr(h1, C.c_int), None, 0, B._ptr(c1, C.c_int), B._ptr(s1, C.c_double), p1) == -1
    assert b"image 0: h (1 + 3 w) above 2^27" in err(), err()
    sc[1] = 1.0
    assert lib.ctpn_write_line_crops_png(None, px, 0, 2, 32, 24, None, 0, B._ptr(cnt, C.c_int), 32, 64, 0, None, None, C.byref(total)) == -1
    assert total.value == 0 and b"ctpn_write_line_crops_png: null pointer" in err()
    total.value = -1
    assert lib.ctpn_write_line_crops_png_ragged(None, px, 0, 2, 32, 24, B._ptr(hts, C.c_int), None, 0, B._ptr(cnt, C.c_int), 32, 64, 0, None, None, C.byref(total)) == -1
    assert total.value == 0 and b"ctpn_write_line_crops_png_ragged: null pointer" in err()
    for crop_h, max_w, pad in ((0, 64, 0), (257, 64, 0), (32, 6, 0), (32, 65536, 0), (32, 64, 256)):      # the JPEG form's geometry limits
        assert lib.ctpn_write_line_crops_png_ragged(fake, px, 0, 2, 32, 24, B._ptr(hts, C.c_int), None, 0, B._ptr(cnt, C.c_int), crop_h, max_w, pad, None, None,
                                                    C.byref(total)) == -1, (crop_h, max_w, pad)


def test_write_line_crops_png_has_no_device_entropy_form():
    class NoLib(object):
        def __getattr__(self, name):
            raise AssertionError("the library is not reached: " + name)
    ctx = B.Context.__new__(B.Context)
    ctx._lib = NoLib()
    with pytest.raises(ValueError, match="entropy"):
        B.Context.write_line_crops(ctx, np.zeros((1, 32, 32, 3), np.uint8), [np.zeros((0, 9))], format="png", entropy="device")
    with pytest.raises(ValueError, match="format"):
        B.Context.write_line_crops(ctx, np.zeros((1, 32, 32, 3), np.uint8), [np.zeros((0, 9))], format="bmp")


def test_demo_batch_keyword_defaults():
    import inspect
    from ctpn_amd.ctpn import demo_batch
    for fn in (demo_batch.run, demo_batch._run_gpu):
        p = inspect.signature(fn).parameters
        assert p["crops_format"].default == "jpg" and p["ragged_png"].default is False, fn
    assert inspect.signature(demo_batch.plan_device_jobs).parameters["ragged_png"].default is False
    assert inspect.signature(demo_batch.check_ragged_options).parameters["ragged_png"].default is False
    assert inspect.signature(demo_batch.write_crops).parameters["format"].default == "jpg"
    args = demo_batch.build_parser().parse_args([])
    assert args.crops_format == "jpg" and args.ragged_png is False
    args = demo_batch.build_parser().parse_args(["--crops-format", "png", "--ragged-png"])
    assert args.crops_format == "png" and args.ragged_png is True


def test_run_refuses_each_missing_prerequisite_before_any_work(tmp_path):
    """before the net (None here) or the disk is touched"""
    from ctpn_amd.ctpn import demo_batch
    out, crops = tmp_path / "out", tmp_path / "crops"
    full = dict(decode="gpu", ragged=True, ragged_outputs=True, png_encode="gpu", ragged_png=True)
    for drop, put in (("ragged", False), ("ragged_outputs", False), ("png_encode", "host")):
        kw = dict(full)
        kw[drop] = put
        with pytest.raises(ValueError, match="ragged_png"):
            demo_batch.run(None, [], str(out), **kw)
    with pytest.raises(ValueError):
        demo_batch.run(None, [], str(out), **dict(full, decode="host"))
    with pytest.raises(ValueError, match="ragged_png"):
        demo_batch.run(None, [], str(out), ragged_png=True)
    with pytest.raises(ValueError, match="crops_format"):
        demo_batch.run(None, [], str(out), decode="gpu", crops_dir=str(crops), crops_format="bmp")
    with pytest.raises(ValueError, match="gpu-entropy"):
        demo_batch.run(None, [], str(out), decode="gpu", crops_dir=str(crops), crops_format="png", crops_encode="gpu-entropy")
    # without the new keyword the refusal stands as it did
    with pytest.raises(ValueError, match="ragged device decode does not combine with png_encode='gpu'"):
        demo_batch.run(None, [], str(out), decode="gpu", ragged=True, ragged_outputs=True, png_encode="gpu")
    assert not out.exists() and not crops.exists()
    chk = demo_batch.check_ragged_options
    chk(decode="gpu", encode="gpu", png_encode="gpu", crops_dir=str(crops), ragged_outputs=True, ragged_png=True)      # accepted
    with pytest.raises(ValueError, match="uniform batches"):
        chk(decode="gpu", png_encode="gpu", ragged_outputs=True)
    with pytest.raises(ValueError, match="gpu-entropy"):
        demo_batch.write_crops(None, str(crops), [], [], encode="gpu-entropy", format="png")


def test_planner_without_the_keyword_is_todays_and_with_it_batches_png_files():
    from ctpn_amd.ctpn.demo_batch import plan_device_jobs
    for kw in ({}, {"ragged": True}, {"ragged": True, "waste": 0.0}):
        assert plan_device_jobs(ENTRIES, 32, ragged_png=False, **kw) == plan_device_jobs(ENTRIES, 32, **kw)
    plain = plan_device_jobs(ENTRIES, 32)
    assert sorted((j[1], tuple(j[4])) for j in plain) == [("host", ("g.bmp",)), ("jpg", ("a.jpg",)), ("jpg", ("b.jpg", "h.jpg")), ("jpg", ("c.jpg",)),
                                                         ("jpg", ("d.jpg",)), ("jpg", ("e.jpg",)), ("png", ("f.png",))]
    rag = plan_device_jobs(ENTRIES, 32, ragged=True)
    assert [j[1] for j in rag].count("ragged") == 1 and not any(j[1] == "ragged-png" for j in rag)
    # one PNG file ends alone: the size-grouped job it always had
    assert plan_device_jobs(ENTRIES, 32, ragged=True, ragged_png=True) == rag
    more = ENTRIES + [("i.png", (1600, 1200), (-1, 0), 0.5, (800, 600)), ("k.png", (776, 600), (-1, 0), 1.0, (776, 600)), ("l.png", (600, 900), (-1, 0), 1.0, (600, 900))]
    jobs = plan_device_jobs(more, 32, ragged=True, ragged_png=True)
    assert sorted(n for j in jobs for n in j[4]) == sorted(e[0] for e in more)                    # every image exactly once
    rp = [j for j in jobs if j[1] == "ragged-png"]
    assert len(rp) == 1
    (hc, wc), _, per, rs, members = rp[0]
    assert (hc, wc) == rs == (800, 600) and members == ["f.png", "i.png", "k.png"]
    assert per == [(800, 600, 1.0), (1600, 1200, 0.5), (776, 600, 1.0)]
    assert [j for j in jobs if j[4] == ["l.png"]][0][:4] == ((600, 900), "png", 1.0, (600, 900))
    assert [j for j in jobs if j[1] == "ragged"] == [j for j in rag if j[1] == "ragged"]          # the JPEG plan does not move
