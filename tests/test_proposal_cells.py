"""CPU: the table of proposal-layer cells (tests/proposal_cell_cases.py) is complete and true, the library's plan function equals the launch
conditions as enqueue_proposals / launch_nms_columns stood before the plan existed, and the checks of tests/test_gpu_proposal_kernels.py reject
eleven numpy models of the stage with one defect each. No device."""
import numpy as np
import pytest

from ctpn_amd import _binding as B
import proposal_cells as C
from proposal_cell_cases import CASES


def test_the_table_equals_the_census():
    want = set(C.census())
    have = {C.cell_plan_half(cell, c) for cell, c in CASES}
    assert have == want, (sorted(want - have), sorted(have - want))
    assert len({c.name for _, c in CASES}) == len(CASES)
    # every census row is held by its smallest case
    for key, (n, hf, wf, pre, cols, prefix) in C.census().items():
        assert any(C.cell_plan_half(cell, c) == key and (c.n, c.hf, c.wf) == (n, hf, wf) for cell, c in CASES), key


def test_every_data_class_is_reached():
    have = set()
    for cell, _ in CASES:
        w = cell.split("/")
        have |= {(w[2], "prefix", w[3]), (w[2], "kept", w[4]), (None, "valid", w[6])}
    assert [r for r in C.REQUIRED_DATA if r not in have] == []
    # the kept lists of the two 0.9-threshold maps pass both LDS capacities, as the oracle's roi counts from one column say
    by_name = {c.name: c for _, c in CASES}
    for name in ("kept_60x3_groups", "kept_100x2_groups"):
        assert max(s["kept_max"] for s in C.model(by_name[name])["stats"]) > 256
    assert 128 < max(s["kept_max"] for s in C.model(by_name["kept_mid_groups"])["stats"]) <= 256
    # 1020 / 1030 candidates per column: the multi-workgroup form's list holds the one, the other keeps the one-workgroup form
    assert C.case_plan(by_name["nms_1020"]).nms == "groups" and C.case_plan(by_name["nms_1030"]).nms == "one_wg"
    assert C.case_plan(by_name["info_narrow"]).nms == "one_wg" and C.case_plan(by_name["sort_3x5_differ"]).nms == "groups"      # the veto
    assert C.case_plan(by_name["pre_7000"]).nms == "groups"          # colid pitch 7008


@pytest.mark.parametrize("cell,case", CASES, ids=[c.name for _, c in CASES])
def test_every_case_is_its_cell_and_the_model_passes_the_checks(cell, case):
    assert C.case_cell(case) == cell
    C.check_stages(case, C.model(case))


def test_switch_points_of_the_segmented_sort():
    P = lambda n, hf, wf, **kw: B.proposal_plan(n, hf, wf, **kw)
    assert P(1, 409, 1).sort == "one_wg" and P(1, 102, 4).sort == "one_wg"                      # 4090, 4080
    p = P(1, 41, 10)
    assert (p.sort, p.seg_len, p.last_seg, p.fill_keys, p.merge_wgs) == ("segmented", 576, 68, False, 5)
    p = P(1, 59, 7)
    assert (p.seg_len, p.last_seg) == (576, 98)
    p = P(1, 2, 256)
    assert (p.seg_len, p.last_seg) == (640, 640)
    p = P(1, 52, 63)
    assert (p.sort, p.seg_len, p.last_seg) == ("segmented", 4096, 4088)                           # 32 760: MG_MAXSEG
    assert P(1, 29, 113).sort == "one_wg" and P(1, 29, 113).fill_keys                             # 32 770
    assert P(4, 41, 10).sort == "segmented" and P(5, 41, 10).sort == "one_wg"
    assert P(1, 41, 10, nms_columns=0).sort == "one_wg" and P(1, 41, 10, nms_columns=2).sort == "one_wg"
    # inside the segmented form's domain the last segment is never short of a wave: 68 keys at the least over maps (4100 = 7 x 576 + 68), 65 over
    # key counts (4097: ctpn_debug_sort_keys runs it) -- a segment is ceil(per_img / 8) rounded UP to 64, so seven of them leave more than 64 keys
    raw = B.proposal_plan_sweep(1, 1, 1, 1, 3300)[0]
    seg = raw[:, 2] == 1
    assert seg.any() and raw[seg, 4].min() == 68
    per = np.arange(4097, 32769)
    sl = ((per + 7) // 8 + 63) & ~63
    assert (per - 7 * sl).min() == 65 and per[np.argmin(per - 7 * sl)] == 4097


def _restated(n, cols, prefix, scratch, pre, post, thresh, narrow):
    """the conditions of enqueue_proposals_impl / launch_decode / launch_sort_keys / launch_nms_columns, in numpy over the whole grid"""
    hf = np.arange(1, C.GRID_HF + 1)[:, None] + np.zeros((1, C.GRID_WF), np.int64)
    wf = np.arange(1, C.GRID_WF + 1)[None, :] + np.zeros((C.GRID_HF, 1), np.int64)
    per = hf * wf * 10
    npad = (2 ** np.ceil(np.log2(per))).astype(np.int64)
    seg_len = ((per + 7) // 8 + 63) & ~63
    seg = np.full(per.shape, cols not in (0, 2) and n <= 4) & (per > 4096) & (seg_len <= 4096)
    cols_ok = np.full(per.shape, cols != 0 and pre <= 12288 and thresh >= 0.1) & (wf <= 256)
    mw = cols_ok & (hf * 10 <= 1024) & bool(scratch and ((cols == 3 and n <= 32) or (cols == 1 and n <= 4)))
    if narrow is not None:
        mw &= np.float32(narrow) >= ((wf - 1) * 16 + 1).astype(np.float32)
    pfx = 4096 if prefix else 0
    two = pfx > 0 and pfx < pre and post < pfx
    one = pfx > 0 and post < pfx
    out = np.zeros(per.shape + (9,), np.int64)
    out[..., 0] = npad
    out[..., 1] = (npad > per) & ~seg
    out[..., 2] = seg
    out[..., 3] = np.where(seg, seg_len, per)
    out[..., 4] = np.where(seg, per - 7 * seg_len, per)
    out[..., 5] = np.where(seg, (per + 1023) // 1024, 0)
    out[..., 6] = np.where(mw, 2, np.where(cols_ok, 1, 0))
    out[..., 7] = np.where(mw, (wf + 3) // 4, 0)
    out[..., 8] = np.where(mw, 2 if two else 0, np.where(cols_ok, 1 if one else 0, 0))
    return out


@pytest.mark.parametrize("cols", [0, 1, 2, 3])
@pytest.mark.parametrize("prefix", [0, 1])
def test_the_plan_equals_the_launch_conditions(cols, prefix):
    for n in range(1, 34):
        for pre, post, thresh, scratch, narrow in ((12000, 1000, 0.7, True, None), (300, 100, 0.7, True, None), (4096, 1000, 0.7, True, None),
                                                   (4097, 4096, 0.7, True, None), (12289, 1000, 0.7, True, None), (12000, 1000, 0.05, True, None),
                                                   (12000, 1000, 0.7, False, None), (12000, 1000, 0.7, True, 801.0)):
            if n > 5 and (pre, thresh, scratch, narrow) != (12000, 0.7, True, None):
                continue                                   # (the batch size meets the other inputs in one place each: n <= 4, n <= 32)
            w = None if narrow is None else np.array([9000.0] * (n - 1) + [narrow], np.float32)
            got = B.proposal_plan_sweep(n, 1, C.GRID_HF, 1, C.GRID_WF, pre=pre, post=post, thresh=thresh, nms_columns=cols, nms_prefix=prefix,
                                        mw_scratch=scratch, im_widths=w)
            want = _restated(n, cols, prefix, scratch, pre, post, thresh, narrow)
            assert np.array_equal(got, want), (n, pre, post, thresh, scratch, narrow, np.argwhere(got != want)[:3])


def test_plan_hook_refuses_nonsense():
    with pytest.raises(B.CtpnError):
        B.proposal_plan_sweep(0, 1, 1, 1, 1)
    with pytest.raises(B.CtpnError):
        B.proposal_plan_sweep(1, 0, 1, 1, 1)
    with pytest.raises(B.CtpnError):
        B.proposal_plan_sweep(1, 1, 1, 1, 1, pre=0)


def test_key_order_ranks_negative_zero_below_positive_zero():
    """The key orders the score's bits: descending score, and -0.0 BEHIND +0.0 where the oracle's float comparison sees a tie (ctpn_hip.h)."""
    s = np.array([0.25, -0.0, 0.0, -1.5, np.inf, 1e-40, -1e-40, 0.0, -0.0, 1.0], np.float32)
    boxes = np.tile(np.array([0, 0, 15, 15], np.float32), (s.size, 1))
    order = (np.sort(C.keys_ref(boxes, s, [100, 100, 1.0], 8.0)) & np.uint64(0xffffffff)).astype(int).tolist()
    assert order == [4, 9, 0, 5, 2, 7, 1, 8, 6, 3]
    bits = C.order_bits(s)
    assert bits[1] < bits[2] and np.array_equal(C.score_from_order_bits(bits).view(np.uint32), s.view(np.uint32))
    from oracle.postproc import desc_order
    assert desc_order(s).tolist() == [4, 9, 0, 5, 1, 2, 7, 8, 6, 3]      # the oracle: the four zeros tie, by index


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_the_checks_reject_the_mutant(mutant):
    hits = [c.name for _, c in CASES if C.caught(c, mutant)]
    assert hits, "no committed case tells the '%s' model from the stage" % mutant
