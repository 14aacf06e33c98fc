"""CPU: ragged canvases built on the device from decoded images and PNG files (ctpn_pack_canvas, ctpn_decode_png_files_ragged) -- what of
them needs no device:
  * the per-thread text of canvas_pack_kernel -- csrc/canvas_pack_dev.h over csrc/resize_pixel.h -- compiled with g++ under ASan + UBSan as
    a stand-alone program (tests/canvas_pack_host.cpp) and run as a subprocess over every case of tests/canvas_pack_cases.py, at source
    pitches 3 w, 3 w + 1 and 3 w + 7: the canvas equals oracle/resize_ref.py's of every image in its slot and zeros below, byte for byte,
    from exact-size heap blocks (a one-byte over-read or over-write is a sanitizer report);
  * the cases themselves: every (h, w, f) maps to the canvas width by the oracle AND by the library's ctpn_resize_dims; the shapes the
    GPU test relies on are all there;
  * the two symbols in header, library and binding; ABI version 10; no device: CTPN_ERR_NODEVICE, not a CPU fallback;
  * demo_batch's --ragged-pack: defaults, the option check, the planner's jobs. Pure functions."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canvas_pack_cases as K  # noqa: E402

import ctpn_amd  # noqa: E402
from ctpn_amd import _binding as B  # noqa: E402
from oracle import resize_ref  # noqa: E402

NEW_SYMBOLS = ("ctpn_pack_canvas", "ctpn_decode_png_files_ragged")
GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def pack_program(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("canvas_pack_host") / "canvas_pack_host")
    subprocess.run(GXX + ["-o", exe, os.path.join(root, "tests", "canvas_pack_host.cpp")], check=True)
    return exe


def test_the_cases_hold_every_shape_the_kernel_can_go_wrong_at():
    cases = K.cases()
    assert {c[2] % 4 for c in cases} == {0, 1, 2, 3} and {c[1] for c in cases} == {16, 23} and {len(c[3]) for c in cases} == {1, 2, 5}
    tails = {(len(c[3]) * c[1] * c[2]) % 4 for c in cases}
    assert 0 in tails and tails - {0}                                    # whole quads only, and a byte-wise tail
    assert {k for c in cases for k in c[4]} >= {"copy16", "copy_hc", "narrow1", "narrow2", "narrow3", "down43_16", "down43_hc", "up_mid", "up_hc", "down_mid"}
    for hc in K.HCS:                                                     # the narrow sources exist exactly where the docstring says
        for wc in K.WCS:
            assert [K.find(wc, w, range(16, hc + 1)) is not None for w in (1, 2, 3)] == [hc == 23] * 3
    seen_h = set()
    for name, hc, wc, imgs, kinds in cases:
        _, heights = K.expected(name)
        for (h, w, f), dh in zip(imgs, heights):
            assert K.dims(h, w, f) == (dh, wc) and 16 <= dh <= hc, (name, h, w, f)
            assert tuple(B.resize_dims(h, w, f, f)) == (resize_ref.out_dim(h, f), resize_ref.out_dim(w, f))      # the library's rule is the oracle's
            seen_h.add((hc, int(dh)))
    assert {(16, 16), (23, 16), (23, 23)} <= seen_h and any(16 < d < 23 for hc, d in seen_h if hc == 23)
    assert any(abs(f - wc / 43.0) < 1e-12 for _, _, wc, imgs, _ in cases for _, w, f in imgs if w == 43)      # the non-terminating factor


@pytest.mark.parametrize("extra", K.PITCH_EXTRA)
def test_kernel_text_under_sanitizers_equals_the_oracle_canvas(pack_program, tmp_path, extra):
    for name, hc, wc, imgs, _ in K.cases():
        want, heights = K.expected(name)
        with open(str(tmp_path / "in.bin"), "wb") as f:
            f.write(struct.pack("<iii", len(imgs), hc, wc))
            blocks = []
            for (h, w, fac), src, dh in zip(imgs, K.sources(name), heights):
                buf, at, pitch = K.pitched(src, extra)
                f.write(struct.pack("<iiiqd", h, w, int(dh), pitch, fac))
                blocks.append(buf[at:])                                  # exactly (h - 1) * pitch + 3 w bytes
                assert blocks[-1].size == (h - 1) * pitch + 3 * w
            for b in blocks:
                f.write(b.tobytes())
        r = subprocess.run([pack_program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.stderr == "", (name, r.stderr[-3000:])                  # the sanitizers are silent
        assert r.returncode == 0, (name, r.stdout[-2000:])
        got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
        assert got.size == want.size, name
        got = got.reshape(want.shape)
        for i, dh in enumerate(heights):
            assert np.array_equal(got[i, :dh], want[i, :dh]), (name, i)
            assert not got[i, dh:].any(), (name, i)                      # zeros the text wrote: the buffer held 0xCD
        assert np.array_equal(got, want), name


def test_expected_canvas_is_im_list_to_canvas_of_the_resized_images():
    from ctpn_amd.lib.utils.blob import im_list_to_canvas
    name = "wc19_hc23_n5"
    _, hc, wc, imgs, _ = K.case(name)
    want, heights = K.expected(name)
    resized = [s if f == 1.0 else resize_ref.resize_linear(s, f, f) for s, (_, _, f) in zip(K.sources(name), imgs)]
    canvas, hts = im_list_to_canvas(resized)
    assert list(hts) == list(heights)
    assert np.array_equal(canvas, want[:, : canvas.shape[1]]) and not want[:, canvas.shape[1]:].any()


def test_header_rules_and_build_flags(root):
    src = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    hdr = open(os.path.join(src, "canvas_pack_dev.h")).read()
    code = re.sub(r"//[^\n]*", "", hdr)
    assert "hip" not in code.lower().replace("__hipcc__", "")            # no HIP header, no HIP call: RS_HD carries the qualifiers
    assert set(re.findall(r'#include\s+[<"]([^>"]+)[>"]', code)) == {"stddef.h", "stdint.h", "resize_pixel.h"}
    assert not re.search(r"\bwhile\b|\bdo\b", code)                      # every loop is a for with a constant or precomputed bound
    for loop in re.findall(r"for \(([^)]*)\)", code):
        assert re.search(r"k < (4|3|left)\b|c < 3\b", loop), loop
    mk = open(os.path.join(src, "Makefile")).read()
    nocontract = re.search(r"^NOCONTRACT_UNITS = (.*)$", mk, flags=re.M).group(1).split()
    assert "canvas_pack" in nocontract and "canvas_pack_dev.h" in mk
    srcs = re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()
    assert "canvas_pack" in srcs and "api_canvas_pack" in srcs
    unit = re.sub(r"//[^\n]*", "", open(os.path.join(src, "api_canvas_pack.hip")).read())
    assert "hipDeviceSynchronize" not in unit and "hipMemset" not in unit and unit.count("hipMemcpyAsync(") == 1      # one copy per call, then the kernel


def test_symbols_in_header_library_and_binding(root):
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    lib = B.load_library()
    declared = B._declare(C.CDLL(B.lib_path()))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, hdr) and hasattr(lib, s) and s in declared, s
    assert lib.ctpn_abi_version() == 10 and "#define CTPN_ABI_VERSION 10" in hdr      # additive
    assert len(declared["ctpn_pack_canvas"][1]) == 12 and len(declared["ctpn_decode_png_files_ragged"][1]) == 10
    for name in ("pack_canvas", "decode_png_files_ragged"):
        assert callable(getattr(B, name))
    for name in ("pack_canvas", "decode_png_ragged"):
        assert callable(getattr(ctpn_amd.Context, name))
    assert list(inspect.signature(ctpn_amd.Context.pack_canvas).parameters) == ["self", "images", "factors", "hc", "wc"]
    assert list(inspect.signature(ctpn_amd.Context.decode_png_ragged).parameters) == ["self", "paths", "shapes", "factors", "hc", "wc"]


def test_binding_refuses_mixed_or_malformed_images_before_the_library():
    with pytest.raises(ValueError, match="all images"):
        B.pack_canvas(None, [np.zeros((16, 17, 3), np.uint8), (4096, (16, 17))], [1.0, 1.0], 16, 17)
    with pytest.raises(ValueError, match="uint8"):
        B.pack_canvas(None, [np.zeros((16, 17, 3), np.float32)], [1.0], 16, 17)


def test_no_device_is_an_error_not_a_cpu_fallback(tmp_path):
    if B.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.pack_canvas(None, [np.zeros((16, 17, 3), np.uint8)], [1.0], 16, 17)
    assert e.value.code == -5 and "no CPU fallback" in str(e.value) and "ctpn_pack_canvas" in str(e.value)
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.decode_png_files_ragged(None, [str(tmp_path / "a.png")], [(16, 17)], [1.0], 16, 17)
    assert e.value.code == -5 and "no CPU fallback" in str(e.value) and "ctpn_decode_png_files_ragged" in str(e.value)


# ---- demo_batch: --ragged-pack ----
ENTRIES = [("a.jpg", (600, 900), (3, 2), 1.0, (600, 900)), ("b.jpg", (1200, 1800), (3, 2), 0.5, (600, 900)), ("g.bmp", (480, 640), (0, 0), 1.25, (600, 800)),
           ("f.png", (800, 600), (-1, 0), 1.0, (800, 600)), ("i.png", (1600, 1200), (-1, 0), 0.5, (800, 600)), ("k.png", (776, 600), (-1, 0), 1.0, (776, 600)),
           ("l.png", (600, 900), (-1, 0), 1.0, (600, 900)), ("m.png", (8, 600), (-1, 0), 1.0, (8, 600))]


def test_ragged_pack_defaults_keep_todays_path():
    from ctpn_amd.ctpn import demo_batch
    for fn in (demo_batch.run, demo_batch._run_gpu, demo_batch.plan_device_jobs, demo_batch.check_ragged_options):
        assert inspect.signature(fn).parameters["ragged_pack"].default == "host", fn
    assert demo_batch.build_parser().parse_args([]).ragged_pack == "host"
    assert demo_batch.build_parser().parse_args(["--ragged-pack", "gpu"]).ragged_pack == "gpu"
    with pytest.raises(SystemExit):
        demo_batch.build_parser().parse_args(["--ragged-pack", "cpu"])
    for kw in ({}, {"ragged": True}, {"ragged": True, "ragged_png": True}, {"ragged": True, "waste": 0.0}, {"ragged_png": True}):
        assert demo_batch.plan_device_jobs(ENTRIES, 32, ragged_pack="host", **kw) == demo_batch.plan_device_jobs(ENTRIES, 32, **kw)
    assert demo_batch.plan_device_jobs(ENTRIES, 32, ragged_pack="gpu") == demo_batch.plan_device_jobs(ENTRIES, 32)      # without ragged it plans nothing


def test_check_ragged_options_with_ragged_pack(tmp_path):
    from ctpn_amd.ctpn import demo_batch
    chk = demo_batch.check_ragged_options
    # every call that passed or failed without the argument does the same with its default
    for kw in (dict(decode="gpu"), dict(decode="host"), dict(decode="gpu", encode="gpu", ragged_outputs=True), dict(decode="gpu", crops_dir="x", ragged_outputs=True),
               dict(decode="gpu", encode="gpu", png_encode="gpu", crops_dir="x", ragged_outputs=True, ragged_png=True)):
        chk(**kw)
        chk(ragged_pack="host", **kw)
    for kw in (dict(decode="gpu", encode="gpu"), dict(decode="gpu", png_encode="gpu", ragged_outputs=True), dict(decode="host", ragged_outputs=True),
               dict(decode_procs=2), dict(ragged=False, ragged_outputs=True)):
        with pytest.raises(ValueError):
            chk(**kw)
        with pytest.raises(ValueError):
            chk(ragged_pack="host", **kw)
    # 'gpu': needs ragged and the device path, and no particular output option
    for decode in ("gpu", "gpu-entropy"):
        chk(decode=decode, ragged_pack="gpu")
    chk(decode="gpu", ragged_pack="gpu", encode="gpu", crops_dir="x", ragged_outputs=True)
    chk(decode="gpu", ragged_pack="gpu", encode="gpu", png_encode="gpu", crops_dir="x", ragged_outputs=True, ragged_png=True)
    with pytest.raises(ValueError, match="ragged_pack='gpu'"):
        chk(decode="host", ragged_pack="gpu")
    with pytest.raises(ValueError, match="ragged_pack='gpu'"):
        chk(decode="gpu", ragged=False, ragged_pack="gpu")
    with pytest.raises(ValueError, match="ragged_pack must be"):
        chk(decode="gpu", ragged_pack="device")
    # it unlocks nothing by itself: the uniform writers stay refused without their own switches
    with pytest.raises(ValueError, match="uniform batches"):
        chk(decode="gpu", ragged_pack="gpu", png_encode="gpu")
    with pytest.raises(ValueError, match="uniform batches"):
        chk(decode="gpu", ragged_pack="gpu", crops_dir="x")
    # run() refuses before the net (None) or the disk is touched
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="ragged_pack='gpu'"):
        demo_batch.run(None, [], str(out), ragged_pack="gpu")
    with pytest.raises(ValueError, match="ragged_pack='gpu'"):
        demo_batch.run(None, [], str(out), decode="gpu", ragged_pack="gpu")
    with pytest.raises(ValueError, match="ragged_pack must be"):
        demo_batch.run(None, [], str(out), decode="gpu", ragged=True, ragged_pack="cuda")
    assert not out.exists()


def test_planner_jobs_for_ragged_pack_gpu():
    from ctpn_amd.ctpn.demo_batch import plan_device_jobs
    host = plan_device_jobs(ENTRIES, 32, ragged=True, ragged_png=True)
    for kw in ({}, {"ragged_png": True}):                                # planned as --ragged-png plans them, with or without that switch
        jobs = plan_device_jobs(ENTRIES, 32, ragged=True, ragged_pack="gpu", **kw)
        assert sorted(n for j in jobs for n in j[4]) == sorted(e[0] for e in ENTRIES)                 # every image exactly once
        rp = [j for j in jobs if j[1] == "ragged-png-gpu"]
        assert len(rp) == 1 and not any(j[1] == "ragged-png" for j in jobs)
        (hc, wc), _, per, rs, members = rp[0]
        assert (hc, wc) == rs == (800, 600) and members == ["f.png", "i.png", "k.png"]
        assert per == [(800, 600, 1.0), (1600, 1200, 0.5), (776, 600, 1.0)]      # (file h, file w, factor): what decode_png_ragged takes
        # the same plan as the host canvas's, under another kind
        assert [(j[0], "ragged-png" if j[1] == "ragged-png-gpu" else j[1], j[2], j[3], j[4]) for j in jobs] == host
        # what ends alone, what is too low for a feature row and Pillow's files stay size-grouped
        assert [j for j in jobs if j[4] == ["l.png"]][0][:4] == ((600, 900), "png", 1.0, (600, 900))
        assert [j for j in jobs if j[4] == ["m.png"]][0][1] == "png" and [j for j in jobs if j[4] == ["g.bmp"]][0][1] == "host"
        assert [j for j in jobs if j[1] == "ragged"] == [j for j in plan_device_jobs(ENTRIES, 32, ragged=True) if j[1] == "ragged"]      # the JPEG plan does not move
