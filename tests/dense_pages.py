"""Dense pages: proposal-layer inputs whose text covers the page, so that more than 1000 proposals per image carry lines. A CTPN proposal is
a 16-pixel slice of a line: a full-width line of a map wf cells wide costs wf proposals, and RPN_POST_NMS_TOP_N = 1000 (the reference's
default, a fresh ctx's capacity) covers 1000 / wf of them -- the slices that fall off the end are the lowest-scored of every line, and the
lines break into fragments. Shared by tests/test_dense_pages.py (CPU), tests/test_gpu_dense_pages.py and tools/dense_page_throughput.py.

dense_page(hf, wf, pitch, anchor, seed):
  foreground probabilities uniform in [0, 0.3] everywhere, uniform in [0.92, 0.999] on anchor `anchor` of every pitch-th feature row (below
  about 0.9 mean score filter_boxes drops the lines); deltas normal(0, 0.02); im_info = [16 hf, 16 wf, 1].
"""
import collections
import functools
import os

import numpy as np

from oracle import postproc as P

Page = collections.namedtuple("Page", "name hf wf pitch anchor seed")
# the pages the issue's table lists: slices above 0.7 = (hf / pitch) wf
PAGES = {
    "40x64": Page("40x64", 40, 64, 1, 0, 0),          # a text row in every feature row, anchor height 11: 2560 slices
    "40x64/2": Page("40x64/2", 40, 64, 2, 1, 0),      # every second feature row, anchor height 16: 1280
    "24x48": Page("24x48", 24, 48, 1, 0, 0),          # 1152
    "64x64": Page("64x64", 64, 64, 1, 0, 0),          # 4096: exactly the largest capacity
    "65x64": Page("65x64", 65, 64, 1, 0, 0),          # 4160: more than any capacity
    "40x64/4": Page("40x64/4", 40, 64, 4, 2, 1),      # a sparser page of the 40 x 64 map (anchor height 23), for batches of different kinds
}
CAPACITY_MAX = 4096


def dense_page(hf, wf, pitch, anchor, seed):
    """-> cls_prob (1, hf, wf, 20), bbox_pred (1, hf, wf, 40), im_info (3,) float32: one image's proposal-layer inputs"""
    rng = np.random.default_rng(seed)
    fg = rng.uniform(0.0, 0.3, (hf, wf, 10))
    fg[::pitch, :, anchor] = rng.uniform(0.92, 0.999, (len(range(0, hf, pitch)), wf))
    cls = np.zeros((1, hf, wf, 10, 2), np.float32)
    cls[0, ..., 1] = fg
    cls[0, ..., 0] = 1.0 - fg
    box = rng.normal(0.0, 0.02, (1, hf, wf, 40)).astype(np.float32)
    return cls.reshape(1, hf, wf, 20), box, np.array([16.0 * hf, 16.0 * wf, 1.0], np.float32)


@functools.lru_cache(maxsize=None)
def page(name):
    p = PAGES[name]
    return dense_page(p.hf, p.wf, p.pitch, p.anchor, p.seed)


@functools.lru_cache(maxsize=None)
def oracle_rois(name, post=CAPACITY_MAX):
    """oracle.postproc.proposal_layer at RPN_POST_NMS_TOP_N = post (computed once per page and value; do not write into it)"""
    cls, box, info = page(name)
    r = P.proposal_layer(cls, box, info, post_nms_topn=post)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def oracle_anchors(name, post=CAPACITY_MAX):
    """the anchor index (y wf + x) 10 + a of every oracle roi: proposal_layer's steps on the indices (min-size filter, order, NMS)"""
    cls, box, info = page(name)
    boxes, scores, _ = P.decode(cls, box, info)
    ok = np.where((boxes[:, 2] - boxes[:, 0] + 1 >= 8) & (boxes[:, 3] - boxes[:, 1] + 1 >= 8))[0]
    order = ok[P.desc_order(scores[ok])][:12000]
    keep = P.nms(np.hstack([boxes[order], scores[order][:, None]]), 0.7)[:post]
    return order[keep].astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle_lines(name, post, mode="H"):
    """oracle.postproc.text_detect on the first `post` rois of the page (rois are in rank order: a prefix is what a smaller top-N returns)"""
    p = PAGES[name]
    r = oracle_rois(name)[:post]
    return P.text_detect(r[:, 1:5], r[:, 0], (16 * p.hf, 16 * p.wf), mode)


def slices_above(name, thresh=0.7):
    return int(np.count_nonzero(oracle_rois(name)[:, 0] > np.float32(thresh)))


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/dense_pages.npz (tools/make_dense_golden.py): the REFERENCE's own proposal_layer and TextDetector at RPN_POST_NMS_TOP_N =
    4096 on the 24x48 and 40x64 pages -> {"rois_<page>", "recs_H_<page>", "recs_O_<page>"}"""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_pages.npz")) as z:
        return {k: z[k] for k in z.files}


GOLDEN_PAGES = ("24x48", "40x64")
