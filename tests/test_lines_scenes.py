"""CPU: the committed scenes of tests/lines_scenes.py reach what they are committed for (conditions, by the oracle alone), and have teeth:
each mutant of the oracle's connector below -- one plausible way a device or host connector can be subtly wrong -- changes at least one
record on at least one scene. tests/test_gpu_text_line_tail.py compares the device with the unmutated oracle on the same scenes, so a
kernel that makes one of these mistakes cannot pass there."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lines_scenes as S  # noqa: E402
from oracle import postproc as P  # noqa: E402


@functools.lru_cache(maxsize=None)
def all_scenes():
    return tuple(S.scenes())


@functools.lru_cache(maxsize=None)
def baseline():
    """{(scene name, mode): records} of the unmutated oracle"""
    return {(sc.name, m): S.oracle_lines(sc, m) for sc in all_scenes() for m in "HO"}


@functools.lru_cache(maxsize=None)
def stats():
    out = {}
    for sc in all_scenes():
        keep = S.oracle_keep(sc)
        d = S.prefix_dets(sc)
        chains = P._chains(d[keep, :4], d[keep, 4], sc.w) if keep else []
        out[sc.name] = dict(rois=sc.rois.shape[0], prefix=d.shape[0], kept=len(keep), longest=max([len(c) for c in chains] + [0]),
                            H=baseline()[(sc.name, "H")].shape[0], O=baseline()[(sc.name, "O")].shape[0])
    return out


@pytest.fixture(autouse=True, scope="module")
def unpatched_oracle_first():
    """the baseline is the UNPATCHED oracle's: computed before any test of this module (a module fixture is set up before a test's monkeypatch),
    so a mutant test selected alone compares against the same records as in a whole run"""
    baseline()
    stats()


def test_scenes_are_well_formed_and_reproducible():
    names = [c.name for c in S.CASES]
    assert len(set(names)) == len(names) and set(S.BATCH_NAMES) <= set(names)
    geo = {(c.h, c.w) for c in S.CASES if c.name in S.BATCH_NAMES}
    assert len(geo) == 1 and len(S.BATCH_NAMES) == 6                               # one geometry: they share a launch
    for c, sc in zip(S.CASES, all_scenes()):
        r = sc.rois
        assert r.dtype == np.float32 and r.shape[1] == 5 and r.shape[0] <= 1000
        assert np.array_equal(r, S.make_scene(c).rois)                             # seeded
        if r.shape[0] == 0:
            continue
        assert np.all(r[:-1, 0] >= r[1:, 0])                                       # descending score
        assert np.all(r[:, 1] % 16 == 0) and np.all(r[:, 3] == r[:, 1] + 15) and r[:, 3].max() <= sc.w - 1      # the anchor grid, inside the image
        assert r[:, 2].min() >= 0 and r[:, 4].max() <= sc.h - 1 and np.all(r[:, 4] > r[:, 2])
        if c.kind in ("mixed", "long"):
            lv = np.isin(r[:, 0], S.LEVELS)
            assert 0.8 < lv.mean() < 0.99 and np.all(r[~lv, 0] <= np.float32(0.7))    # nine in ten on the levels, the rest at or below 0.7
            assert np.unique(r[lv, 0]).size <= 15 < lv.sum() // 8                      # ties are the rule
    assert any(np.any(sc.rois[:, 0] == np.float32(0.7)) for sc in all_scenes())        # the threshold value itself


def test_committed_scenes_meet_their_conditions(monkeypatch):
    st = stats()
    by_name = {c.name: c for c in S.CASES}
    assert any(256 < s["kept"] <= 512 for s in st.values()) and any(s["kept"] > 512 for s in st.values())      # a second and a third pass of connect_kernel's loops
    assert any(256 < st[n]["kept"] for n in S.BATCH_NAMES)                                                      # ... also inside a batch
    assert any(128 < s["longest"] <= 256 for s in st.values())                                                  # numpy's pairwise sum splits once
    assert any(s["longest"] > 256 and by_name[n].w > 4096 for n, s in st.items())                               # ... twice, past the column NMS's 256 columns
    assert any(s["H"] >= 10 and s["O"] >= 10 for s in st.values())
    assert any(s["H"] != s["O"] for s in st.values())
    assert any(s["rois"] == 0 for s in st.values())                                                             # an empty scene
    assert any(s["rois"] > 0 and s["prefix"] == 0 for s in st.values())                                         # nothing above 0.7
    assert any(s["rois"] == 1000 == s["prefix"] for s in st.values())                                           # lines_prep's look-ahead row is the buffer's last
    assert any(0 < s["prefix"] < s["rois"] for s in st.values())                                                # the prefix ends inside the list
    scales = [c.scale for c in S.CASES]
    assert any(np.log2(s) % 1 != 0 and s < 4 for s in scales) and any(s > 4 for s in scales)                    # not a power of two; the generic fallback
    assert any(float(np.float32(s)) != s for s in scales)                                                       # not an fp32 value: where the division is rounded matters
    # one column whose kept list outgrows the LDS capacity of both column NMS forms (48 and 256 boxes), and candidates that only a kept box
    # beyond it drops (tests/test_gpu_text_line_tail.py::test_kept_list_past_its_lds_capacity)
    deep = next(sc for sc in all_scenes() if sc.name == "deep")
    depths = S.sole_suppressor_depths(S.prefix_dets(deep), S.oracle_keep(deep), P.Cfg.TEXT_PROPOSALS_NMS_THRESH)
    assert st["deep"]["kept"] > 256 and np.unique(deep.rois[:, 1]).size == 1 and deep.scale == 1.0
    assert sum(d >= 48 for d in depths) >= 8 and sum(d >= 256 for d in depths) >= 8
    # a line that filter_boxes drops for each of its three reasons alone (detectors.py:37-49), in both modes
    monkeypatch.setattr(P.Cfg, "MIN_RATIO", -1.0)
    monkeypatch.setattr(P.Cfg, "LINE_MIN_SCORE", -1.0)
    monkeypatch.setattr(P.Cfg, "TEXT_PROPOSALS_WIDTH", -1.0)
    for mode in "HO":
        seen = set()
        for sc in all_scenes():
            r = S.oracle_lines(sc, mode)
            if r.shape[0] == 0:
                continue
            hh = (np.abs(r[:, 5] - r[:, 1]) + np.abs(r[:, 7] - r[:, 3])) / 2.0 + 1
            ww = (np.abs(r[:, 2] - r[:, 0]) + np.abs(r[:, 6] - r[:, 4])) / 2.0 + 1
            fails = np.stack([~(ww / hh > 0.5), ~(r[:, 8] > 0.9), ~(ww > 32)], axis=1)
            seen |= {int(np.argmax(f)) for f in fails if f.sum() == 1}
            assert r.shape[0] - int(fails.any(axis=1).sum()) == stats()[sc.name][mode]
        assert seen == {0, 1, 2}, (mode, seen)


def test_outside_scene_is_outside():
    """the scene of the IndexError test: boxes / scale reach past the image, and the oracle, like the reference, raises on it"""
    sc = S.make_scene(S.OUTSIDE)
    assert sc.scale < 1 and (S.prefix_dets(sc)[:, 0] >= sc.w).any()
    with pytest.raises(IndexError):
        S.oracle_lines(sc, "H")


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------
def changed_records():
    """(scene, mode) pairs on which the oracle, as patched by the caller, no longer gives the baseline's records"""
    out = []
    for sc in all_scenes():
        for m in "HO":
            got, want = S.oracle_lines(sc, m), baseline()[(sc.name, m)]
            if got.shape != want.shape or not np.array_equal(got, want):
                out.append((sc.name, m))
    return out


def chains_variant(p, s, im_w, last_max=False, farthest=False):
    """oracle/postproc.py::_chains restated with two switches: the successor is the LAST maximum of its column instead of the first; the
    precursors of a node come from the FARTHEST matching column within the gap instead of the nearest. Both off: the oracle (asserted)."""
    n = p.shape[0]
    h = p[:, 3] - p[:, 1] + 1
    table = [[] for _ in range(im_w)]
    for i in range(n):
        table[int(p[i, 0])].append(i)

    def succ(i):
        x = int(p[i, 0])
        for left in range(x + 1, min(x + P.Cfg.MAX_HORIZONTAL_GAP + 1, im_w)):
            r = [j for j in table[left] if P._meet_v_iou(p, h, j, i)]
            if r:
                return r
        return []

    def prec(i):
        x = int(p[i, 0])
        cols = range(x - 1, max(int(p[i, 0] - P.Cfg.MAX_HORIZONTAL_GAP), 0) - 1, -1)
        for left in (reversed(cols) if farthest else cols):
            r = [j for j in table[left] if P._meet_v_iou(p, h, j, i)]
            if r:
                return r
        return []

    nxt, has_in = [-1] * n, [False] * n
    for i in range(n):
        c = succ(i)
        if not c:
            continue
        sc = s[c]
        best = c[len(c) - 1 - int(np.argmax(sc[::-1]))] if last_max else c[int(np.argmax(sc))]
        if s[i] >= np.max(s[prec(best)]):
            nxt[i] = best
            has_in[best] = True
    out = []
    for i in range(n):
        if not has_in[i] and nxt[i] >= 0:
            ch = [i]
            while nxt[ch[-1]] >= 0:
                ch.append(nxt[ch[-1]])
            out.append(ch)
    return out


def test_chains_restatement_is_the_oracle(monkeypatch):
    monkeypatch.setattr(P, "_chains", chains_variant)
    assert changed_records() == []


def test_mutant_successor_takes_the_last_maximum(monkeypatch):
    monkeypatch.setattr(P, "_chains", functools.partial(chains_variant, last_max=True))
    assert changed_records()


def test_mutant_precursor_takes_the_farthest_column(monkeypatch):
    monkeypatch.setattr(P, "_chains", functools.partial(chains_variant, farthest=True))
    assert changed_records()


class NumpyWith:
    """numpy, with some of its functions replaced: what oracle/postproc.py sees as `np` under a mutant"""

    def __init__(self, **over):
        self._over = over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(np, name)


class SequentialSum(np.ndarray):
    """.sum() of a 1-D fp32 array as a plain left-to-right fp32 loop instead of numpy's pairwise reduction"""

    def sum(self, *a, **k):
        if a or k or self.ndim != 1 or self.dtype != np.float32:
            return np.asarray(self).sum(*a, **k)
        acc = np.float32(0)
        for v in np.asarray(self):
            acc = np.float32(acc + v)
        return acc


class GreaterIsGreaterEqual(np.ndarray):
    def __gt__(self, other):
        return np.asarray(self) >= other


def test_mutant_score_mean_is_a_sequential_sum(monkeypatch):
    monkeypatch.setattr(P, "np", NumpyWith(asarray=lambda *a, **k: np.asarray(*a, **k).view(SequentialSum)))
    assert changed_records()


def test_mutant_score_filter_is_greater_or_equal(monkeypatch):
    monkeypatch.setattr(P, "np", NumpyWith(asarray=lambda *a, **k: np.asarray(*a, **k).view(GreaterIsGreaterEqual)))
    assert changed_records()


def test_mutant_boxes_divided_in_float64_then_rounded(monkeypatch):
    monkeypatch.setattr(S, "divide", lambda boxes, scale: (boxes.astype(np.float64) / float(scale)).astype(np.float32))
    assert changed_records()
