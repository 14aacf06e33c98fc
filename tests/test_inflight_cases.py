"""CPU: the cases of tests/test_gpu_weights_reload.py and tests/test_gpu_inflight.py cannot pass vacuously (tests/inflight_cases.py) -- the two
arenas differ in every element, the copy -> reader -> case table names what pack_weights writes and reaches both lstm_pre forms by the plan
hook, every ctx-taking function of the ABI is in exactly one class, and the placements are what the GPU tests say they are."""
import ctypes
import os
import re

import numpy as np
import pytest

import ctpn_amd
from ctpn_amd import _binding as B
import ctx_walks as W
import inflight_cases as K


def test_arenas_share_no_element_in_any_manifest_entry():
    w1, w2 = K.arena("W1"), K.arena("W2")
    assert w1 is W.weights() and K.SEEDS == {"W1": 3, "W2": 4} and not w1.flags.writeable and not w2.flags.writeable
    m = K.manifest()
    assert len(m) == 38 and sum(c for _, c, _ in m) == ctpn_amd.WEIGHT_FLOATS == w1.size == w2.size
    for name, count, off in m:
        assert not (w1[off:off + count] == w2[off:off + count]).any(), name
    assert np.isfinite(w2).all() and not (w2 == 0).any()


@pytest.mark.parametrize("k", [0, 1, 26, 28, 37])
def test_mixed_arena_is_w1_but_for_one_entry(k):
    w1, w2, mk = K.arena("W1"), K.arena("W2"), K.mixed(k)
    name, count, off = K.manifest()[k]
    assert np.array_equal(mk[off:off + count], w2[off:off + count]) and np.array_equal(mk[:off], w1[:off]) and np.array_equal(mk[off + count:], w1[off + count:])
    assert mk is not K.mixed(k) and np.array_equal(K.arena_of(("M", k)), mk) and K.arena_of("W2") is w2
    assert sorted(i for lo, hi in K.A2_GROUPS for i in range(lo, hi)) == list(range(38))


def _pack_weights_members(root):
    src = open(os.path.join(root, "text-detection-ctpn_amd", "csrc", "api_weights.hip")).read()
    body = src[src.index("int pack_lstm_projection("):src.index("c->weights_loaded = true;")]
    body = re.sub(r"//[^\n]*", "", body)
    members = set(re.findall(r"\bc->(\w+)", body)) - {"stream", "arena", "prec", "wx_row_bytes"}
    return members, src


def test_copy_table_is_what_pack_weights_writes(root):
    members, src = _pack_weights_members(root)
    table = {c.member for c in K.COPIES}
    assert members == table, (sorted(members - table), sorted(table - members))
    names = [n for n, _, _ in K.manifest()]
    fed = {s for c in K.COPIES for s in c.sources}
    assert fed == set(names), sorted(set(names) ^ fed)                     # every entry feeds a copy, no copy names an entry that does not exist
    folded = {c.member: c.sources for c in K.COPIES}
    assert len(folded["b_fold"]) == 6 and set(folded["wt_x"]) == set(folded["wh"]) == set(folded["wt_xf"])      # what A2 separates
    fwd = open(os.path.join(root, "text-detection-ctpn_amd", "csrc", "api_forward.hip")).read()
    for c in K.COPIES:                                                         # a copy nobody reads would need no case
        assert re.search(r"c->%s\b" % c.member, fwd), c.member
    assert "launch_lstm_pre(cur, c->wt_xf" in fwd and "g.wt = c->wt_x;" in fwd       # the docstring's reading of who reads wt_x / wt_xf
    assert "if (!c->weights_loaded)" not in src                                # no copy is packed on the first load only


def test_every_reader_has_a_case_in_each_of_its_precisions():
    for c in K.COPIES:
        assert c.readers, c.member
        for r in c.readers:
            assert r.precs and set(r.precs) <= set(W.PRECS) and r.cases, (c.member, r.kernel)
            for prec in r.precs:
                assert any(prec in K.RELOAD_CASES[name].precs for name in r.cases), (c.member, r.kernel, prec)
    used = {name for c in K.COPIES for r in c.readers for name in r.cases}
    assert used == set(K.RELOAD_CASES)
    for name, case in K.RELOAD_CASES.items():
        assert case.ops and all(op in K.FRESH_RUN for op in case.ops) and set(case.precs) <= set(W.PRECS), name
        assert all(k in B.OPTION_ENV for k in case.options), name
    # the issue's list: the ops of the default case, conv1_kernel 0 / 1 / 2 with conv1_fuse 0 and 1, lstm_split 0 and 1, keep_acts 0 and 1
    assert K.RELOAD_CASES["default"].ops == ("uA", "uC", "bD", "pAB") and K.RELOAD_CASES["default"].precs == W.PRECS
    opts = [c.options for c in K.RELOAD_CASES.values()]
    for want in ({"conv1_kernel": 0}, {"conv1_kernel": 1}, {"conv1_fuse": 0}, {"lstm_split": 0}, {"keep_acts": 1}, {}):
        assert want in opts, want


def test_lstm_pre_forms_come_from_the_plan_hook():
    """ctpn_debug_lstm_pre_plan, planned for the MI355X's 256 CUs (pure host arithmetic): the ctx_walks ops are all small, uBig is resident"""
    form = {op: B.lstm_pre_plan(cells, cu_count=256).form for op, cells in K.LSTM_PRE_CELLS.items()}
    assert form == {"uA": "small", "uC": "small", "bD": "small", "pAB": "small", "uBig": "lds"}, form      # "lds": lstm_pre_kernel, the weight slice resident in LDS
    assert B.lstm_pre_plan(K.LSTM_PRE_RESIDENT_ABOVE, cu_count=256).form == "small" and B.lstm_pre_plan(K.LSTM_PRE_RESIDENT_ABOVE + 1, cu_count=256).form == "lds"
    n, h, w = K.BIG
    assert K.LSTM_PRE_CELLS["uBig"] == n * (h // 16) * (w // 16) and K.extra_inputs()["Big"].shape == (n, h, w, 3)
    assert n * (h // 16) <= 128                                                # the recurrence's rows: its four-rows form everywhere (module docstring)
    assert "uBig" in K.RELOAD_CASES["resident_lstm_pre"].ops and "uA" in K.RELOAD_CASES["default"].ops


def ctx_functions(root):
    """the ctpn_* functions of the header with a ctpn_ctx* or ctpn_ctx** parameter"""
    txt = open(os.path.join(root, "include", "ctpn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(ctpn_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S) if "ctpn_ctx" in m.group(2)}


def test_every_ctx_function_is_in_exactly_one_class(root):
    declared = set(B._declare(ctypes.CDLL(B.lib_path())).keys())
    takes_ctx = ctx_functions(root)
    assert takes_ctx <= declared and len(takes_ctx) >= 70 and {"ctpn_destroy", "ctpn_broadcast_weights", "ctpn_create"} <= takes_ctx
    assert "ctpn_nms" not in takes_ctx and "ctpn_weight_count" not in takes_ctx
    classes = {name: set(fns) for name, fns in K.CLASSES.items()}
    assert set(classes) == {"between", "refused", "excluded"}
    for a, b in (("between", "refused"), ("between", "excluded"), ("refused", "excluded")):
        assert not classes[a] & classes[b], (a, b, sorted(classes[a] & classes[b]))
    classified = classes["between"] | classes["refused"] | classes["excluded"]
    assert takes_ctx - classified == set(), "not classified (tests/inflight_cases.py, CLASSES): %s" % sorted(takes_ctx - classified)
    assert classified - takes_ctx == set(), "classified, but not a ctx-taking function of the header: %s" % sorted(classified - takes_ctx)
    for fn, reason in K.CLASSES["excluded"].items():
        assert isinstance(reason, str) and len(reason) > 20 and "\n" not in reason, fn
    # the issue's minimum
    assert {"ctpn_set_option", "ctpn_set_param", "ctpn_reserve_proposals", "ctpn_debug_text_lines", "ctpn_load_weights_host", "ctpn_load_weights_device",
            "ctpn_broadcast_weights_rank"} <= classes["refused"]
    assert {"ctpn_forward", "ctpn_forward_blob", "ctpn_forward_ragged", "ctpn_proposals", "ctpn_proposals_from_host", "ctpn_proposal_anchors", "ctpn_get_tensor",
            "ctpn_feat_shape", "ctpn_sync", "ctpn_detect", "ctpn_detect_ragged", "ctpn_decode_jpeg_batch", "ctpn_decode_jpeg_batch_device", "ctpn_pack_canvas",
            "ctpn_crop_lines", "ctpn_encode_jpeg_batch", "ctpn_encode_png_batch", "ctpn_profile_enable", "ctpn_profile_read", "ctpn_get_option", "ctpn_get_param",
            "ctpn_proposal_capacity"} <= classes["between"]


def test_refused_functions_refuse_in_the_source(root):
    """what puts a function into the class: it drains and answers CTPN_ERR_STATE naming itself while a slot is busy"""
    src = os.path.join(root, "text-detection-ctpn_amd", "csrc")
    code = "\n".join(re.sub(r"//[^\n]*", "", open(os.path.join(src, f)).read()) for f in sorted(os.listdir(src)) if f.startswith("api_") and f.endswith(".hip"))
    for fn in K.CLASSES["refused"]:
        assert re.search(r'"%s: a submitted batch has not been collected"|weights_quiesce\(\w+(\[i\])?, "%s"\)' % (fn, fn), code), fn
    body = code[code.index("static int weights_quiesce("):]
    body = body[:body.index("\n}\n")]
    order = [body.index(s) for s in ("hipSetDevice(c->device)", "sync_forwards(c)", "hipStreamSynchronize(c->stream_p)", "sl.busy", "tail_pending = false")]
    assert order == sorted(order)                                              # ctpn_set_option's contract, in its order
    rank = code[code.index("int ctpn_broadcast_weights_rank("):]
    assert rank.index("weights_quiesce(") < rank.index("comm_init_rank(")      # a local pre-check, in front of the communicator
    for fn in ("ctpn_load_weights_host", "ctpn_load_weights_device"):
        b = code[code.index("int %s(" % fn):]
        assert b.index("weights_quiesce(") < b.index("hipMemcpyAsync(c->arena")


def test_between_calls_and_placements():
    names = [x.name for x in K.XS]
    assert len(set(names)) == len(names) and {x.family for x in K.XS} == {"forward", "proposals", "detect", "io"}
    for x in K.XS:
        assert x.fns and all(fn in K.CLASSES["between"] for fn in x.fns), x.name
        for placement in K.PLACEMENTS:
            for last in ("A", "B"):
                kind, what = x.expect(last, placement)
                assert (kind == "fresh" and what in K.FRESH_RUN) or (kind == "code" and what < 0), (x.name, kind, what)
    # one slot free: the call runs; both busy: ctpn_detect_submit's refusal
    for name in ("detect", "detect_ragged"):
        x = next(x for x in K.XS if x.name == name)
        assert x.expect("A", 1)[0] == "fresh" and x.expect("B", 2) == ("code", K.CTPN_ERR_STATE)
    assert K.xs_for("bf16") == K.XS and all(x.family != "io" for x in K.xs_for("fp32")) and len(K.xs_for("fp32")) == len(K.XS) - 6
    assert K.PLACEMENTS == (1, 2) and K.COLLECTED == {1: "uA", 2: "pAB"}
    assert len({r.name for r in K.REFUSED}) == len(K.REFUSED) == 9 and {r.fn for r in K.REFUSED} == set(K.CLASSES["refused"])

    class Recorder:
        def __init__(self):
            self.calls = []

        def detect_submit(self, images=None, slot=0):
            self.calls.append(("submit", images.shape[:3], slot))

        def detect_collect(self, slot, want_rois=False):
            self.calls.append(("collect", slot))
            return [np.zeros((0, 9))], [np.zeros((0, 5), np.float32)]

    for placement, want, last in ((1, [("submit", W.A, 0), ("collect", 0)], "A"),
                                  (2, [("submit", W.A, 0), ("submit", W.B, 1), ("collect", 0), ("collect", 1)], "B")):
        r = Recorder()
        assert K.submit(r, placement) == last
        assert len(K.collect(r, placement)) == 2 * placement and r.calls == want


def test_fresh_registry_holds_the_ops_and_same_sees_a_stale_weight():
    assert {o.name for o in W.OPS} <= set(K.FRESH_RUN) and set(K.ROI_OPS) <= set(K.FRESH_RUN)
    a = (np.arange(6, dtype=np.float32).reshape(2, 3), 3)
    b = (np.nextafter(a[0], np.float32(9)), 3)
    assert W.same(a, a) is None and W.same(a, b) == 0 and K.rows((np.zeros((4, 5), np.float32), np.zeros((2, 9))), 5, np.float32) == 4
