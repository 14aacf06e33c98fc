"""CPU: the cases of tests/decode_heads_cells.py have teeth -- a numpy model of decode_kernel's production branch passes the checks of
tests/test_gpu_decode_heads.py on every case, and with any one of ten defects fails them on at least one -- and the shapes reach the block and
image seams they are listed for. No device."""
import numpy as np
import pytest

import decode_heads_cells as D
import proposal_cells as C


@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_the_intact_model_passes_the_checks(case):
    report = []
    D.check(case, D.model(case), report)
    assert report[0][2] == 0 and report[0][4] <= 1.0          # the model's exponentials are the correctly rounded ones


@pytest.mark.parametrize("defect", D.DEFECTS)
def test_the_checks_reject_the_defect(defect):
    hits = [c.name for c in D.CASES if D.caught(c, defect)]
    assert hits, "no case tells the '%s' model from the branch" % defect


def test_each_defect_is_caught_where_it_is_expected():
    """the cases the table lists for a situation are the ones that catch its defect"""
    assert D.caught(D.BY_NAME["four_selects"], "select_image2_gets_row1") and D.caught(D.BY_NAME["seams_3x5x7"], "select_image2_gets_row1")
    assert D.caught(D.BY_NAME["four_selects"], "select_image3_gets_row2")
    assert not D.caught(D.BY_NAME["five_device_rows"], "select_image3_gets_row2")      # five images: the device copy, no selects
    assert D.caught(D.BY_NAME["ragged_6_3_1"], "valid_rows_le") and D.caught(D.BY_NAME["ragged_6_3_1"], "valid_rows_of_previous_image")
    assert not D.caught(D.BY_NAME["ragged_idle"], "valid_rows_le")                        # the idle filter: present, and nothing to drop
    for c in D.CASES:
        if c.n * c.hf * c.wf > 1:
            assert D.caught(c, "head_ld_60"), c.name
        for defect in ("pair_of_next_anchor", "fg_bg_swapped_in_store", "dy_dh_from_x_z"):
            assert D.caught(c, defect), (c.name, defect)


def test_the_shapes_reach_their_seams():
    shape = {c.name: (c.n, c.hf * c.wf * 10) for c in D.CASES}
    n, per = shape["one_cell"]
    assert n * per == 10 and 3 * n < n * per                                  # the threads that publish im_info are anchors' threads too
    n, per = shape["four_selects"]
    assert n == 4 and n * per == 240 <= 256                                   # all four select arms inside one 256-thread block
    n, per = shape["five_device_rows"]
    assert n == 5 and (n * per + 255) // 256 == 2 and 256 // per == n - 1     # above four images; one block seam, inside the last image
    n, per = shape["seams_3x5x7"]
    assert n * per == 1050 and (n * per + 255) // 256 == 5 and all((i * per) % 256 for i in range(1, n))      # image seams in mid-block
    c = D.BY_NAME["ragged_6_3_1"]
    assert c.valid_rows[0] == c.hf and 0 < c.valid_rows[2] < c.valid_rows[1] < c.hf
    c = D.BY_NAME["ragged_idle"]
    assert set(c.valid_rows) == {c.hf}
    for c in D.CASES:
        assert c.n * c.hf * c.wf * 10 <= 1050
        info = D.case_inputs(c)[1]
        assert np.all(info[:, 1] >= (c.wf - 1) * 16 + 1)                      # no image narrower than its map's last column: the planned NMS form stays
        if c.n > 1:
            assert len({tuple(r) for r in info.tolist()}) == c.n and D.swapped_row_shows(c), c.name


def test_every_recipe_is_reached_and_the_poison_is_in_place():
    kinds, dkinds = set(), set()
    for c in D.CASES:
        heads, _, _, kind, dkind = D.case_inputs(c)
        kinds |= set(np.unique(kind).tolist())
        dkinds |= set(np.unique(dkind).tolist())
        assert np.all(np.isnan(heads[..., 60:]))
        if c.n * c.hf * c.wf * 10 >= 240:
            assert set(np.unique(kind).tolist()) == set(range(len(D.KINDS))), c.name
            assert set(np.unique(dkind).tolist()) == set(range(len(D.DELTA_KINDS))), c.name
    assert kinds == set(range(len(D.KINDS))) and dkinds == set(range(len(D.DELTA_KINDS)))
    # the exponentials of the recipes are what the module's table says: normal, subnormal, zero
    tiny = np.float32(np.finfo(np.float32).tiny)
    e = np.exp(np.array([-20, -88, -104, -200], np.float64)).astype(np.float32)
    assert e[0] >= tiny and 0 < e[1] < tiny and e[2] == 0 and e[3] == 0
    assert np.exp(-104.0) < 2.0 ** -150                                       # below half the smallest subnormal: zero is the correct rounding


def test_the_softmax_expectations():
    s = np.array([[1.5, 1.5], [0.0, -200.0], [1e30, np.nextafter(np.float32(1e30), np.float32(np.inf))], [-np.inf, 0.25], [np.inf, 0.25], [np.nan, 0.25],
                  [0.25, np.nan], [-1e30, np.nextafter(np.float32(-1e30), np.float32(-np.inf))]], np.float32)
    nan, exact, p = D.softmax_expected(s)
    assert nan.tolist() == [False, False, False, False, True, True, True, False] and exact.tolist() == [True, True, True, True, False, False, False, True]
    assert p[:4].tolist() == [[0.5, 0.5], [1.0, 0.0], [0.0, 1.0], [0.0, 1.0]] and p[7].tolist() == [1.0, 0.0]
    assert np.array_equal(np.isnan(D.softmax64(s)[:, 0]), nan)                # the float64 pair softmax says NaN where the kernel's operations do
    # without the max subtraction the saturated and the huge pairs are NaN: the recipes need it
    assert np.isnan(D.softmax_restated(s[[2, 7]], max_subtraction=False)).all()
    assert np.isnan(D.softmax_restated(np.array([[0.0, 200.0]], np.float32), max_subtraction=False)).any()


def test_the_non_finite_deltas_are_what_the_module_says():
    """fmaxf(fminf(v, lim), 0) against numpy's maximum(minimum(v, lim), 0): they differ for dh = NaN only, and the key stays valid only below
    min_size x scale = 1 (the finding of the module docstring)"""
    seen = set()
    valid_where_numpy_drops = 0
    for c in D.CASES:
        info = D.case_inputs(c)[1]
        for i, a, kind, kb, nb, agree, kkeep, nkeep in D.nonfinite_expected(c):
            seen.add(kind)
            hl = info[i, 0] - np.float32(1.0)
            assert agree == (kind != "dh_nan"), (c.name, i, a, kind)
            if kind == "dh+100":
                assert kb[1] == 0 and kb[3] == hl and kkeep
            elif kind == "dh-100":
                assert kb[1] == kb[3] and kkeep == (c.min_size * info[i, 2] <= 1)
            elif kind == "dy+inf":
                assert kb[1] == hl and kb[3] == hl
            elif kind == "dy-inf":
                assert kb[1] == 0 and kb[3] == 0
            else:
                assert kb[1] == hl and kb[3] == hl and np.isnan(nb[1]) and np.isnan(nb[3]) and not nkeep
                assert kkeep == (c.min_size * info[i, 2] <= 1), (c.name, i, a)
                valid_where_numpy_drops += int(kkeep)
    assert seen == set(D.DELTA_KINDS[1:])
    assert valid_where_numpy_drops > 0 and all(r[6] == r[7] or c.name == "min_size_half" for c in D.CASES for r in D.nonfinite_expected(c))


def test_key_of_a_nan_score_is_invalid_in_the_model():
    c = D.BY_NAME["seams_3x5x7"]
    m = D.model(c)
    score = m["cls_prob"].reshape(c.n, -1, 2)[..., 1]
    for i in range(c.n):
        idx = (m["sorted_keys"][i][m["sorted_keys"][i] != D.KEY_INVALID] & np.uint64(0xffffffff)).astype(np.int64)
        assert np.isnan(score[i]).any() and not np.isnan(score[i][idx]).any()
    assert C.next_pow2(350) == 512
