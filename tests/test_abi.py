"""CPU: the C-ABI library loads, exports every symbol include/ctpn_hip.h declares, and fails loudly without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B


def header_functions(root):
    txt = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ctpn_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(root):
    lib = B.load_library()
    names = header_functions(root)
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "libctpn_hip.so does not export " + n


def test_binding_declares_every_header_function(root):
    lib = ctypes.CDLL(B.lib_path())
    declared = set(B._declare(lib).keys())
    assert declared == set(header_functions(root))


def test_abi_version_and_manifest_agree_with_python():
    assert B.load_library().ctpn_abi_version() == 10
    got = B.manifest_from_library()
    want = [(n, tuple(s), o) for n, s, o in ctpn_amd.MANIFEST]
    assert got == want
    last = want[-1]
    assert last[2] + int(np.prod(last[1])) == ctpn_amd.WEIGHT_FLOATS == 17893244


def test_no_cpu_fallback_without_device():
    if B.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(ctpn_amd.CtpnError) as e:
        ctpn_amd.Context(0, 1, 64, 64, "fp32")
    assert e.value.code == -5
    with pytest.raises(ctpn_amd.CtpnError) as e:
        B.nms_sorted(np.array([[0, 0, 10, 10, 0.9]], np.float32), 0.5, 0)
    assert e.value.code == -5
    assert "no CPU fallback" in str(e.value)


def test_argument_errors_are_reported_not_crashed():
    lib = B.load_library()
    h = ctypes.c_void_p()
    assert lib.ctpn_create(ctypes.byref(h), 0, 0, 64, 64, 0) == -1      # max_batch 0
    assert lib.ctpn_create(ctypes.byref(h), 0, 1, 64, 64, 7) == -1      # unknown precision (0..3 = fp32, bf16, fp16, split)
    assert b"precision" in lib.ctpn_last_error()
    cnt = ctypes.c_int(5)
    keep = np.zeros(4, np.int32)
    assert lib.ctpn_nms(keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(cnt), None, 0, 5, 0.5, 0) == 0
    assert cnt.value == 0                                                  # empty input -> empty keep, like nms_wrapper.py:12-13
    assert lib.ctpn_text_lines(None, None, 0, 100, 100, 9, -1, None, 0, ctypes.byref(cnt)) == -1  # bad mode


def test_product_library_has_no_wrong_result_switches():
    """the timing-only ablations that produce WRONG results (CTPN_C3_P_ABL, CTPN_C3_WR_VAR) are compiled only with
    -DCTPN_ABLATION (`make ablation` -> libctpn_hip_ablation.so); an inherited environment variable cannot corrupt the product
    library's output because the library never reads it."""
    blob = open(B.lib_path(), "rb").read()
    for name in (b"CTPN_C3_P_ABL", b"CTPN_C3_WR_VAR", b"CTPN_C3_WS", b"CTPN_SORT_RADIX", b"CTPN_NMS_FOOTPRINT", b"CTPN_CONV1_TPW"):
        assert name not in blob, name
    assert b"rocprofiler-sdk-roctx" in blob                      # dlopen'ed by name on demand (CTPN_ROCTX=1) ...
    import subprocess
    needed = subprocess.run(["readelf", "-d", B.lib_path()], capture_output=True, text=True).stdout
    assert "roctx" not in needed and "rccl" not in needed        # ... not a link-time dependency; RCCL likewise


def test_options_are_abi_not_environment(root):
    """behaviour switches are per-ctx options of the ABI (ctpn_set_option), not process-wide environment variables. The
    library enumerates exactly the options the header documents, and the product sources read at most five environment variables, none
    of which selects arithmetic or kernels (tracing, debug sync, host-thread budget / affinity, library search paths)."""
    assert B.option_names() == ["keep_acts", "conv1_kernel", "conv1_fuse", "lstm_split", "nms_columns", "nms_check", "connect_device", "tail_overlap",
                                "conv_p64", "tail_confine", "nms_prefix", "debug_hog", "debug_nms", "split_edge"]
    assert sorted(B.OPTION_ENV) == sorted(B.option_names())
    hdr = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    for name in B.option_names():
        assert re.search(r"\*\s+%s\s" % name, hdr), name + " is not documented in ctpn_hip.h"
    src = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    env = set()
    for f in sorted(os.listdir(src)):
        if f.endswith((".hip", ".h", ".cpp")):
            code = re.sub(r"//[^\n]*", "", open(os.path.join(src, f)).read())
            code = re.sub(r"#ifdef CTPN_ABLATION.*?#endif", "", code, flags=re.S)          # measurement builds only
            env |= set(re.findall(r'(?:getenv|env_int)\("([A-Z_0-9]+)"', code))
    assert env <= {"CTPN_DEBUG_SYNC", "CTPN_ROCTX", "ROCM_PATH", "CTPN_RCCL_LIB", "CTPN_HOST_THREADS", "CTPN_AFFINITY", "LOCAL_WORLD_SIZE", "LOCAL_RANK",
                   "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"}, env      # the last two: quoted in ctpn_create's "device_id out of range" message only
    assert len({e for e in env if e.startswith("CTPN_")}) <= 5
    blob = open(B.lib_path(), "rb").read()
    for name in (b"CTPN_CONV_IMPL", b"CTPN_IGEMM_VARIANT", b"CTPN_C3_PERSIST", b"CTPN_C3_PIPE", b"CTPN_LSTM_SPLIT", b"CTPN_CONV1_MFMA", b"CTPN_KEEP_ACTS",
                 b"CTPN_C3_AHEAD", b"CTPN_C3_STACK", b"CTPN_C3_HALFTAIL", b"CTPN_C3_WR_XCD", b"CTPN_NMS_COLUMNS", b"CTPN_TAIL_OVERLAP", b"CTPN_F16"):
        assert name not in blob, name
    lib = B.load_library()
    assert lib.ctpn_set_option(None, b"keep_acts", 1) == -1 and lib.ctpn_option_name(99) is None


def test_no_null_stream_memset_in_the_launch_paths(root):
    """Round-3 defect: conv3x3_wr's tile-claim counters were zeroed with a plain hipMemset -- null stream -- in front of a launch on the
    ctx's NON-BLOCKING stream, which does not wait for it: the first bf16 forward of a process could start from counters that were not
    zero yet. Device state that a launch depends on is initialised with hipMemsetAsync on the launch stream (or a blocking copy from
    pageable host memory); the only plain hipMemset calls left are in the ctpn_debug_* entry points of the host units (api_*.hip), which
    run everything on the null stream."""
    src = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    conv_hdrs = sorted(f for f in os.listdir(src) if f.startswith("conv3x3") and f.endswith(".h"))      # every conv header, whatever is added later
    assert conv_hdrs and not os.path.exists(os.path.join(src, "conv3x3_impl.h"))
    kernel_units = sorted(f for f in os.listdir(src) if f.endswith(".hip") and not f.startswith("api_"))      # every kernel unit, whatever is added later
    assert {"conv3x3.hip", "igemm.hip", "bilstm.hip", "preprocess.hip", "conv_first.hip", "conv_first_q.hip", "pack.hip", "decode.hip", "sort_keys.hip", "nms.hip", "connect.hip",
            "hog.hip"} <= set(kernel_units) and not os.path.exists(os.path.join(src, "proposal.hip")) and not os.path.exists(os.path.join(src, "layers.hip"))
    for f in kernel_units + ["common.h", "proposal_dev.h"] + conv_hdrs:
        text = open(os.path.join(src, f)).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert "hipMemset(" not in code, f
    units = sorted(f for f in os.listdir(src) if f.startswith("api_") and f.endswith(".hip"))      # every host unit, whatever is added later
    assert units and not os.path.exists(os.path.join(src, "ctpn_api.hip"))
    for f in units:
        api = re.sub(r"//[^\n]*", "", open(os.path.join(src, f)).read())
        for m in re.finditer(r"hipMemset\(", api):
            head = api[:m.start()]
            fns = re.findall(r"\nint (ctpn_\w+)\(", head)
            assert fns and fns[-1].startswith("ctpn_debug_"), (f, fns[-1:])


def test_hip_resources_are_created_and_released_in_owned_h_only(root):
    """The host side owns every device block, page-locked block, event and stream through the four types of csrc/owned.h: a release has no
    other spelling anywhere in csrc/, and in the host units (api_*.hip, ctx.h) neither has an acquisition. The hand-written idioms the
    types replaced are gone by name, and ctpn_destroy is: select the device, drain the streams, delete the ctx.
    The kernel units' launchers keep six acquisitions of process-wide scratch (tile-claim counters, a dump block, the strip stream and its two
    events, conv1_1's constant block): made once per device, never released, not owned by a ctx. They are listed here, file by file, so that
    the list cannot grow unseen; owned.h is not included by the kernel units."""
    src = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    files = sorted(f for f in os.listdir(src) if f.endswith((".hip", ".h", ".cpp")))
    assert "owned.h" in files and "ctx.h" in files
    code = {f: re.sub(r"//[^\n]*", "", open(os.path.join(src, f)).read()) for f in files}
    release = ["hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy("]
    acquire = ["hipMalloc(", "hipHostMalloc(", "hipEventCreate", "hipStreamCreate"]
    for word in release + acquire:
        assert word in code["owned.h"], word
    launcher_scratch = {"conv3x3.hip": {"hipMalloc(": 2, "hipStreamCreate": 1, "hipEventCreate": 2}, "conv_first.hip": {"hipMalloc(": 1}}
    for f in files:
        if f == "owned.h":
            continue
        for word in release:
            assert word not in code[f], (f, word)
        host_unit = f.startswith("api_") or f == "ctx.h"
        assert host_unit or "owned.h" not in code[f], f
        for word in acquire:
            allowed = 0 if host_unit else launcher_scratch.get(f, {}).get(word, 0)
            assert code[f].count(word) == allowed, (f, word, code[f].count(word))
    for f in files:
        for name in ("grow_dev", "grow_host", "jpeg_grow_dev", "jpeg_grow_pair", "Free3", "DC_TRY", "RS_TRY", "DevBufs"):
            assert not re.search(r"\b%s\b" % name, code[f]), (f, name)
    body = re.search(r"\nint ctpn_destroy\(ctpn_ctx\* c\) \{\n(.*?)\n\}\n", code["api_ctx.hip"], flags=re.S).group(1)
    assert "delete c;" in body and "hipSetDevice(c->device)" in body and body.count("hipStreamSynchronize(") == 4
    assert not re.search(r"\b(for|while|do)\b", body), body
