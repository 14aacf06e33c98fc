"""Cases for the tests of a live ctx's weights and of the calls made between a submit and its collect (tests/test_inflight_cases.py,
tests/test_gpu_weights_reload.py, tests/test_gpu_inflight.py). Test infrastructure only; nothing here needs a GPU to import or to build its
inputs -- an op's run(ctx) and fresh() do. The ops, inputs and the comparison are tests/ctx_walks.py's (same: shape, dtype and bytes).

Arenas  W1 = util.stress_arena("biased", 3) (ctx_walks' own), W2 = util.stress_arena("biased", 4): no element of any of the 38 manifest entries
        has the same value at the same place in both (tests/test_inflight_cases.py). mixed(k) = W1 with entry k alone taken from W2.
        arena_of(key): "W1" | "W2" | ("M", k).
fresh   fresh(prec, arena, name, options): FRESH_RUN[name] on a new ctx that has loaded `arena` and done nothing else, once per (precision,
        arena, op, options, capacity) and shared by every GPU test of the two files.
COPIES  what pack_weights (csrc/api_weights.hip) derives from the arena: copy -> the manifest entries it is made from -> the kernels that
        read it -> the RELOAD_CASES that run that reader. Written from the code (api_weights.hip, api_forward.hip, lstm_pre.hip, bilstm.hip):
          * launch_lstm_pre is handed wt_xf in BOTH of its forms (api_forward.hip: launch_lstm_pre(cur, c->wt_xf, ...)): in the 16-bit modes wt_x is
            only what wt_xf is packed from, and no kernel of the forward reads it; fp32 and split precision read wt_x through the im2col GEMM.
          * every ctx_walks op is small for lstm_pre (390 cells at most; the resident form starts beyond 4096 cells on 256 CUs): op uBig, a
            detect of the whole capacity 5 x 304 x 1040 (6175 cells), is here for lstm_pre_kernel.
          * the recurrence's rows (n x hf) stay below 128 within the capacity (95 at most): the split-bf16 recurrence runs in its four-rows form;
            the 16-rows form reads the same wh through the same pointer and layout and has its own exact test (tests/test_gpu_tail_kernels.py).
CLASSES every ctpn_* function of include/ctpn_hip.h that takes a ctpn_ctx, in exactly one class, from reading the function:
          between   may be called with a batch in flight: it changes neither batch, and gives what it gives on a fresh ctx (or its documented code)
          refused   CTPN_ERR_STATE while a slot is busy (the ctx drains its streams first), and harmless
          excluded  not run between a submit and its collect by this suite, with the reason
XS      the between calls as the GPU test makes them: X(name, family, fns, run(ctx, last, placement), expect(last, placement)); last = the
        batch submitted last ("A" | "B"), placement 1 = submit A slot 0 . X . collect 0, 2 = submit A slot 0 . submit B slot 1 . X . collect 0 . collect 1.
        expect -> ("fresh", FRESH_RUN name) | ("code", n).
REFUSED the refused calls: R(name, fn, call(ctx, env), undo(ctx, env)); env: see refused_env()."""
import collections
import functools

import numpy as np

import ctx_walks as W
import util

SEEDS = {"W1": 3, "W2": 4}
BIG = W.CAP
CTPN_ERR_STATE = -3
LSTM_PRE_RESIDENT_ABOVE = 4096      # cells, on 256 CUs (csrc/lstm_pre.hip, lstm_pre_plan): asserted in tests/test_inflight_cases.py


@functools.lru_cache(maxsize=None)
def arena(which):
    a = W.weights() if which == "W1" else util.stress_arena("biased", SEEDS[which])
    a.setflags(write=False)
    return a


def manifest():
    import ctpn_amd
    return [(name, int(np.prod(shape)), int(off)) for name, shape, off in ctpn_amd.MANIFEST]


def mixed(k):
    """W1 with manifest entry k alone taken from W2 (a new array each time: 72 MB, not cached)"""
    _, count, off = manifest()[k]
    a = np.array(arena("W1"))
    a[off:off + count] = arena("W2")[off:off + count]
    return a


def arena_of(key):
    return arena(key) if isinstance(key, str) else mixed(key[1])


# ---------------------------------------------------------------------------------------------------------------
# ops beside ctx_walks'
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extra_inputs():
    import ctpn_amd
    from out_ragged_cases import line
    from util_jpeg import encode, scene
    x = {"Big": ctpn_amd.weights.synthetic_images(*BIG, 71)}
    rng = np.random.default_rng(8)
    hf, wf = 6, 10                                              # D's feature map
    cls = rng.uniform(0.0, 1.0, (1, hf, wf, 20)).astype(np.float32)
    x["cls"], x["bbox"] = cls, (rng.standard_normal((1, hf, wf, 40)) * 0.2).astype(np.float32)
    x["files"] = tuple(encode(scene(48, 64, 3 + i), 90) for i in range(2))
    x["px"] = ctpn_amd.weights.synthetic_images(2, 48, 64, 40)
    x["recs"] = np.array([[line(4.0, 4.0, 52.0, 10.0, 0.95, slant=2.0), line(6.0, 24.0, 32.0, 8.0, 0.9)]] * 2, np.float64)
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


def _uBig(ctx):
    return W._flat(ctx.detect(extra_inputs()["Big"], want_rois=True))


def _heads_of(name):
    """the ctx_walks op and the `heads` behind it"""
    return lambda ctx: W.OP[name].run(ctx) + (ctx.get_tensor("heads"),)


def _forward_then(shape_name, shape):
    def run(ctx):
        ctx.forward(W.inputs()[shape_name])
        return _read_last(ctx, shape)
    return run


def _read_last(ctx, shape):
    """what the read-only calls give for the most recent forward: two maps, the geometry, the proposals and their anchors"""
    heads, rpn = ctx.get_tensor("heads"), ctx.get_tensor("rpn_conv/3x3")
    rois, anchors = ctx.proposals(W._info([shape[1]] * shape[0], shape[2]), want_anchors=True)
    return (heads, rpn) + tuple(int(v) for v in ctx.feat_shape()) + tuple(rois) + tuple(anchors)


def _ragged_forward(ctx):
    x = W.inputs()
    ctx.forward_ragged(x["W"], x["Wh"])
    rois, anchors = ctx.proposals(W._info(list(x["Wh"]), x["W"].shape[2]), want_anchors=True)
    return tuple(rois) + tuple(anchors)


def _from_host(ctx):
    x = extra_inputs()
    rois, anchors = ctx.proposals_from_host(x["cls"], x["bbox"], W._info([W.D[1]], W.D[2]), want_anchors=True)
    return tuple(rois) + tuple(anchors)


def _introspect(ctx):
    from ctpn_amd import _binding as B
    out = tuple(ctx.get_option(nm) for nm in B.option_names()) + tuple(ctx.get_param(nm) for nm in B.param_names())
    return out + (ctx.proposal_capacity, ctx.host_threads(), bool(ctx.stream()))


def _sync(ctx):
    ctx.sync()
    return (0,)


def _profile(ctx):
    ctx.profile_enable(2)
    kinds = len(ctx.profile_read())
    ctx.profile_reset()
    ctx.profile_enable(False)
    return (kinds,)


def _decode(entropy):
    def run(ctx):
        ptr, shape = ctx.decode_jpeg_batch(list(extra_inputs()["files"]), entropy=entropy)
        return (ctx.jpeg_batch_fetch(ptr, shape),) + tuple(int(v) for v in shape)      # fetched before the ctx reuses the buffer
    return run


def _pack_canvas(ctx):
    px = extra_inputs()["px"]
    (ptr, shape), heights = ctx.pack_canvas([px[0], px[1][:32]], [1.0, 1.0], 48, 64)          # one width, two heights
    return (ctx.jpeg_batch_fetch(ptr, shape), np.asarray(heights, np.int32))


def _crop_lines(ctx):
    x = extra_inputs()
    crops, widths = ctx.crop_lines(x["px"], list(x["recs"]), crop_h=16, max_w=64)
    return (crops, np.asarray(widths, np.int32))


def _files(blobs):
    return tuple(np.frombuffer(bytes(b), np.uint8) for b in blobs)


def _encode_jpeg(ctx):
    px = extra_inputs()["px"]
    return _files(ctx.encode_jpeg_batch(px, entropy="host")) + _files(ctx.encode_jpeg_batch(px, entropy="device"))


def _encode_png(ctx):
    return _files(ctx.encode_png_batch(extra_inputs()["px"]))


def _text_lines(ctx, rois):
    lines, keeps = ctx.debug_text_lines(rois, (W.C[1], W.C[2]))
    return tuple(lines) + tuple(np.asarray(k, np.int32) for k in keeps)


# name -> run(ctx): everything fresh() can compute. The ctx_walks ops under their own names.
FRESH_RUN = {o.name: o.run for o in W.OPS}
FRESH_RUN.update({
    "uBig": _uBig, "uC+heads": _heads_of("uC"),
    "read:A": _forward_then("A", W.A), "read:B": _forward_then("B", W.B), "read:C": _forward_then("C", W.C),
    "ragged_forward": _ragged_forward, "from_host": _from_host, "introspect": _introspect, "sync": _sync, "profile": _profile,
    "decode_host": _decode("host"), "decode_device": _decode("device"), "pack_canvas": _pack_canvas, "crop_lines": _crop_lines,
    "encode_jpeg": _encode_jpeg, "encode_png": _encode_png,
})
ROI_OPS = tuple(o.name for o in W.OPS if o.kind != "error") + ("uBig", "uC+heads", "read:A", "read:B", "read:C", "ragged_forward", "from_host")

_fresh = {}


def rows(result, cols, dtype):
    return sum(x.shape[0] for x in result if isinstance(x, np.ndarray) and x.ndim == 2 and x.shape[1] == cols and x.dtype == dtype)


def fresh(prec, akey, name, options=None, maps=(), cap=W.CAP):
    """FRESH_RUN[name] on a new ctx of capacity `cap` that has loaded arena `akey` and done nothing else (with maps: -> (result, {map: array})).
    Cached per (precision, arena, op, options, maps, capacity), except for the mixed arenas, which are asked for once each."""
    import ctpn_amd
    key = (prec, akey, name, tuple(sorted((options or {}).items())), tuple(maps), cap)
    if key in _fresh:
        return _fresh[key]
    with ctpn_amd.Context(0, *cap, prec, options=options or {}) as ctx:
        ctx.load_weights(arena_of(akey))
        res = FRESH_RUN[name](ctx)
        got = {nm: ctx.get_tensor(nm) for nm in maps}
    if name in W.ERROR_CODES:
        assert res == W.ERROR_CODES[name], (prec, name, res)
    elif name in ROI_OPS:
        assert rows(res, 5, np.float32) > 0, "%s %s %s: the fresh result holds no roi, an equality with it would be empty" % (prec, akey, name)
    out = (res, got) if maps else res
    if isinstance(akey, str):
        _fresh[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------
# A. what a load rewrites, who reads it, which case runs the reader
# ---------------------------------------------------------------------------------------------------------------
HALF, ALL = ("fp16", "bf16"), W.PRECS
Case = collections.namedtuple("Case", "precs options ops maps")
RELOAD_CASES = {
    "default": Case(ALL, {}, ("uA", "uC", "bD", "pAB"), False),
    "resident_lstm_pre": Case(HALF, {}, ("uBig",), False),
    "conv1_valu": Case(HALF, {"conv1_kernel": 0}, ("uA",), False),
    "conv1_split": Case(HALF, {"conv1_kernel": 1}, ("uA",), False),
    "conv1_unfused": Case(HALF, {"conv1_fuse": 0}, ("uA",), False),
    "exact_recurrence": Case(("split", "fp16", "bf16"), {"lstm_split": 0}, ("uA",), False),
    "keep_acts": Case(ALL, {"keep_acts": 1}, ("uA",), True),
}
CONV = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3",
        "rpn_conv/3x3"]
_CELL = "lstm_o/bidirectional_rnn/%s/lstm_cell/%s"
_KERNELS, _CELL_BIAS = [_CELL % (d, "kernel") for d in ("fw", "bw")], [_CELL % (d, "bias") for d in ("fw", "bw")]
_FOLDED = ["lstm_o/weights", "lstm_o/biases", "rpn_bbox_pred/weights", "rpn_bbox_pred/biases", "rpn_cls_score/weights", "rpn_cls_score/biases"]
Reader = collections.namedtuple("Reader", "kernel precs cases")
Copy = collections.namedtuple("Copy", "member sources readers")
COPIES = (
    Copy("w_first", ["conv1_1/weights"], [Reader("conv_first_kernel (fp32 VALU)", ("fp32",), ("default", "keep_acts")),
                                          Reader("conv_first_kernel, conv1_kernel = 0", HALF, ("conv1_valu",))]),
    Copy("w_first_frags", ["conv1_1/weights", "conv1_1/biases"], [
        Reader("split-bf16 fragments: launch_conv_first with frags", ("split",), ("default", "keep_acts")),
        Reader("split-bf16 fragments: conv1_kernel = 1", HALF, ("conv1_split",)),
        Reader("split-bf16 fragments: the float-blob feed (op bD)", HALF, ("default",)),
        Reader("q-image fragments (bf16 set / fp16 set), conv1_1 fused into conv1_2's window stage", HALF, ("default",)),
        Reader("q-image fragments, launch_conv_first_from_q (conv1_fuse = 0, keep_acts = 1)", HALF, ("conv1_unfused", "keep_acts"))]),
    Copy("b_conv", [c + "/biases" for c in CONV], [Reader("every conv kernel's epilogue", ALL, ("default", "keep_acts"))]),
    Copy("wt_conv", [c + "/weights" for c in CONV[1:]], [Reader("conv3x3 kernels (pack_transpose_kernel's layout)", ("fp32",) + HALF, ("default", "keep_acts")),
                                                        Reader("conv3x3 split kernels (pack_split_kernel's layout)", ("split",), ("default", "keep_acts"))]),
    Copy("wt_x", _KERNELS, [Reader("lstm_pre as the im2col GEMM", ("fp32", "split"), ("default", "keep_acts"))]),      # 16-bit: the source of wt_xf only
    Copy("b_x", _CELL_BIAS, [Reader("the im2col GEMM's epilogue", ("fp32", "split"), ("default",)),
                             Reader("lstm_pre_small_kernel / lstm_pre_kernel", HALF, ("default", "resident_lstm_pre"))]),
    Copy("wt_xf", _KERNELS, [Reader("lstm_pre_small_kernel", HALF, ("default",)), Reader("lstm_pre_kernel", HALF, ("resident_lstm_pre",))]),
    Copy("wh", _KERNELS, [Reader("bilstm, exact", ("fp32",), ("default",)), Reader("bilstm, exact (lstm_split = 0)", ("split",), ("exact_recurrence",)),
                          Reader("bilstm, exact with v_exp / v_rcp gates (lstm_split = 0)", HALF, ("exact_recurrence",)),
                          Reader("bilstm, split-bf16 (lstm_split = 1)", ("split",) + HALF, ("default",))]),
    Copy("wt_fc", ["lstm_o/weights"], [Reader("lstm_o FC GEMM", ("fp32", "split"), ("default",)), Reader("lstm_o FC GEMM, keep_acts = 1", HALF, ("keep_acts",))]),
    Copy("b_fc", ["lstm_o/biases"], [Reader("lstm_o FC GEMM", ("fp32", "split"), ("default",)), Reader("lstm_o FC GEMM, keep_acts = 1", HALF, ("keep_acts",))]),
    Copy("wt_h", ["rpn_bbox_pred/weights", "rpn_cls_score/weights"], [Reader("heads GEMM", ("fp32", "split"), ("default",)),
                                                                      Reader("heads GEMM, keep_acts = 1", HALF, ("keep_acts",))]),
    Copy("b_h", ["rpn_bbox_pred/biases", "rpn_cls_score/biases"], [Reader("heads GEMM", ("fp32", "split"), ("default",)),
                                                                   Reader("heads GEMM, keep_acts = 1", HALF, ("keep_acts",))]),
    Copy("wt_fold", _FOLDED[0::2], [Reader("folded heads GEMM (keep_acts = 0)", HALF, ("default",))]),
    Copy("b_fold", _FOLDED, [Reader("folded heads GEMM (keep_acts = 0)", HALF, ("default",))]),
)
# cells (n x hf x wf) of the ops that decide lstm_pre's form in the 16-bit modes
LSTM_PRE_CELLS = {"uA": 3 * 2 * 65, "uC": 2 * 4 * 6, "bD": 6 * 10, "pAB": 3 * 19 * 16, "uBig": 5 * 19 * 65}
A2_GROUPS = ((0, 10), (10, 20), (20, 28), (28, 38))          # manifest entries [lo, hi) per test: 38 fresh ctxs per precision, split four ways


# ---------------------------------------------------------------------------------------------------------------
# B. the ABI between a submit and its collect
# ---------------------------------------------------------------------------------------------------------------
X = collections.namedtuple("X", "name family fns run expect")


def _on(name):
    return lambda ctx, last, placement: FRESH_RUN[name](ctx)


def _is(name):
    return lambda last, placement: ("fresh", name)


def _free_slot_only(name):
    """ctpn_detect* takes the free slot (api_detect.hip: slot = slot[0].busy ? 1 : 0); with both busy that is slot 1: ctpn_detect_submit's refusal"""
    return lambda last, placement: ("fresh", name) if placement == 1 else ("code", CTPN_ERR_STATE)


def _detect_or_code(name):
    return lambda ctx, last, placement: FRESH_RUN[name](ctx) if placement == 1 else W._code(lambda: FRESH_RUN[name](ctx))


_SHAPE = {"A": W.A, "B": W.B}
XS = (
    X("forward", "forward", ("ctpn_forward", "ctpn_get_tensor", "ctpn_feat_shape", "ctpn_proposals", "ctpn_proposal_anchors"), _on("read:C"), _is("read:C")),
    X("forward_blob", "forward", ("ctpn_forward_blob",), _on("bD"), _is("bD")),
    X("forward_ragged", "forward", ("ctpn_forward_ragged",), _on("ragged_forward"), _is("ragged_forward")),
    # the read-only calls on the batch in flight itself: the most recent forward is the submit's
    X("read_in_flight", "proposals", ("ctpn_get_tensor", "ctpn_feat_shape", "ctpn_proposals", "ctpn_proposal_anchors"),
      lambda ctx, last, placement: _read_last(ctx, _SHAPE[last]), lambda last, placement: ("fresh", "read:" + last)),
    X("proposals_from_host", "proposals", ("ctpn_proposals_from_host", "ctpn_proposal_anchors"), _on("from_host"), _is("from_host")),
    X("sync", "forward", ("ctpn_sync",), _on("sync"), _is("sync")),
    X("detect", "detect", ("ctpn_detect",), _detect_or_code("uC"), _free_slot_only("uC")),
    X("detect_ragged", "detect", ("ctpn_detect_ragged",), _detect_or_code("rW"), _free_slot_only("rW")),
    X("introspect", "detect", ("ctpn_get_option", "ctpn_get_param", "ctpn_proposal_capacity", "ctpn_host_threads", "ctpn_stream"), _on("introspect"), _is("introspect")),
    X("profile", "detect", ("ctpn_profile_enable", "ctpn_profile_read", "ctpn_profile_reset"), _on("profile"), _is("profile")),
    X("decode_host", "io", ("ctpn_decode_jpeg_batch", "ctpn_jpeg_batch_fetch"), _on("decode_host"), _is("decode_host")),
    X("decode_device", "io", ("ctpn_decode_jpeg_batch_device", "ctpn_jpeg_batch_fetch"), _on("decode_device"), _is("decode_device")),
    X("pack_canvas", "io", ("ctpn_pack_canvas", "ctpn_jpeg_batch_fetch"), _on("pack_canvas"), _is("pack_canvas")),
    X("crop_lines", "io", ("ctpn_crop_lines",), _on("crop_lines"), _is("crop_lines")),
    X("encode_jpeg", "io", ("ctpn_encode_jpeg_batch", "ctpn_encode_jpeg_batch_device"), _on("encode_jpeg"), _is("encode_jpeg")),
    X("encode_png", "io", ("ctpn_encode_png_batch",), _on("encode_png"), _is("encode_png")),
)
IO_PREC = "bf16"          # the image I/O units do not depend on the precision


def xs_for(prec):
    return tuple(x for x in XS if x.family != "io" or prec == IO_PREC)


R = collections.namedtuple("R", "name fn call undo")


def refused_env():
    """what the refused calls need beside the ctx (GPU): W2 as a device tensor, synchronised; the caller adds "rois" for the text-line tail"""
    import torch
    dev = torch.from_numpy(np.array(arena("W2"))).cuda()
    torch.cuda.synchronize()
    return {"W2_dev": dev}


def _load(which):
    return lambda ctx, env: ctx.load_weights(arena(which))


def _reload_w1(ctx, env):
    ctx.load_weights(arena("W1"))


def _nothing(ctx, env):
    pass


def _broadcast_rank(ctx, env):
    from ctpn_amd import _binding as B
    ctx.broadcast_weights_rank(B.comm_unique_id(), 0, 1, root=0)          # an id of its own for every communicator


def _broadcast_all(ctx, env):
    from ctpn_amd import _binding as B
    B.broadcast_weights([ctx])


def _tail_on_fresh_rois(ctx, env):
    return _text_lines(ctx, env["rois"])


REFUSED = (
    R("set_option", "ctpn_set_option", lambda ctx, env: ctx.set_option("nms_prefix", 0), lambda ctx, env: ctx.set_option("nms_prefix", 1)),
    R("set_param", "ctpn_set_param", lambda ctx, env: ctx.set_param("RPN_MIN_SIZE", 9.0), lambda ctx, env: ctx.set_param("RPN_MIN_SIZE", 8.0)),
    R("reserve_proposals", "ctpn_reserve_proposals", lambda ctx, env: ctx.reserve_proposals(2048), lambda ctx, env: ctx.reserve_proposals(1000)),
    R("debug_text_lines", "ctpn_debug_text_lines", _tail_on_fresh_rois, _nothing),
    R("load_weights_W2", "ctpn_load_weights_host", _load("W2"), _reload_w1),
    R("load_weights_W1", "ctpn_load_weights_host", _load("W1"), _nothing),          # the rule goes by state, not by content
    R("load_weights_device", "ctpn_load_weights_device", lambda ctx, env: ctx.load_weights_device(env["W2_dev"].data_ptr()), _reload_w1),
    R("broadcast_weights_rank", "ctpn_broadcast_weights_rank", _broadcast_rank, _nothing),
    R("broadcast_weights", "ctpn_broadcast_weights", _broadcast_all, _nothing),     # n = 1: every handle is checked before anything else
)

_SUBMIT = "the placements themselves: a submit beside a batch in flight, the collects"
CLASSES = {
    "between": {fn: x.name for x in XS for fn in x.fns},
    "refused": {r.fn: r.name for r in REFUSED},
    "excluded": {
        "ctpn_create": "makes a ctx: nothing can be in flight on it",
        "ctpn_create_postproc": "makes a ctx: nothing can be in flight on it",
        "ctpn_destroy": "ends the ctx: drains the four streams and drops the batch, nothing is left to collect",
        "ctpn_debug_proposal_fetch": "test hook of the proposal kernels: reads the shared tail buffers, whose content after a submit is that batch's",
        "ctpn_debug_proposals_from_heads": "test hook of the proposal kernels (tests/test_gpu_decode_heads.py); ctpn_proposals_from_host's path, which is run",
        "ctpn_decode_jpeg_files": "ctpn_decode_jpeg_batch behind a file read: the same pipeline, which is run",
        "ctpn_decode_jpeg_files_device": "ctpn_decode_jpeg_batch_device behind a file read",
        "ctpn_decode_jpeg_batch_ragged": "the ragged decode: the uniform decode's stream and buffer sets, which are run",
        "ctpn_decode_jpeg_files_ragged": "the ragged decode behind a file read",
        "ctpn_decode_png_files_ragged": "host PNG decode + ctpn_pack_canvas's kernel, which is run",
        "ctpn_jpeg_entropy_decode_device": "test hook of the device entropy decoder; run through ctpn_decode_jpeg_batch_device",
        "ctpn_jpeg_entropy_device_stats": "counters of the last device entropy decode: pure host read",
        "ctpn_jpeg_entropy_encode_device": "test hook of the device entropy coder; run through ctpn_encode_jpeg_batch_device",
        "ctpn_jpeg_entropy_encode_device_stats": "counters of the last device entropy coding: pure host read",
        "ctpn_png_encode_device_stats": "counters of the last PNG encode: pure host read",
        "ctpn_encode_jpeg_mixed": "the output stage of ctpn_encode_jpeg_batch (run) over images of mixed sizes",
        "ctpn_encode_jpeg_mixed_device": "the output stage of ctpn_encode_jpeg_batch_device (run) over images of mixed sizes",
        "ctpn_encode_png_mixed": "the output stage of ctpn_encode_png_batch (run) over images of mixed sizes",
        "ctpn_crop_lines_ragged": "ctpn_crop_lines (run) with a height per image",
    },
}
CLASSES["between"].update({"ctpn_detect_submit": _SUBMIT, "ctpn_detect_submit_ragged": _SUBMIT, "ctpn_detect_collect": _SUBMIT,
                           "ctpn_debug_forward_sets": "pure host read: the second placement calls it in between, to see batch B on set 1"})
# the writers: an encoder or the crops (run) in front of a file write
CLASSES["excluded"].update({fn: "writes files: %s, which is run, in front of a file write" % via for fn, via in {
    "ctpn_write_annotated_files": "ctpn_encode_jpeg_batch", "ctpn_write_annotated_files_device": "ctpn_encode_jpeg_batch_device",
    "ctpn_write_annotated_files_ragged": "ctpn_encode_jpeg_batch", "ctpn_write_annotated_files_ragged_device": "ctpn_encode_jpeg_batch_device",
    "ctpn_write_annotated_png_files": "ctpn_encode_png_batch", "ctpn_write_annotated_png_files_ragged": "ctpn_encode_png_batch",
    "ctpn_write_line_crops": "ctpn_crop_lines + ctpn_encode_jpeg_batch", "ctpn_write_line_crops_device": "ctpn_crop_lines + ctpn_encode_jpeg_batch_device",
    "ctpn_write_line_crops_ragged": "ctpn_crop_lines + ctpn_encode_jpeg_batch", "ctpn_write_line_crops_ragged_device": "ctpn_crop_lines + ctpn_encode_jpeg_batch_device",
    "ctpn_write_line_crops_png": "ctpn_crop_lines + ctpn_encode_png_batch", "ctpn_write_line_crops_png_ragged": "ctpn_crop_lines + ctpn_encode_png_batch"}.items()})

PLACEMENTS = (1, 2)


def submit(ctx, placement):
    """the placement's submits -> the name of the batch submitted last"""
    ctx.detect_submit(images=W.inputs()["A"], slot=0)
    if placement == 1:
        return "A"
    ctx.detect_submit(images=W.inputs()["B"], slot=1)
    return "B"


def collect(ctx, placement):
    a = ctx.detect_collect(0, want_rois=True)
    return W._flat(a) if placement == 1 else W._flat(a, ctx.detect_collect(1, want_rois=True))


COLLECTED = {1: "uA", 2: "pAB"}          # the fresh op a placement's collects equal
