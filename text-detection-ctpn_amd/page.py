"""Pages larger than a ctx's network input, detected as tiles at native resolution (include/ctpn_hip.h, "pages in tiles").

detect_page is orchestration only: the plan and the merge are host arithmetic of the library (ctpn_page_plan, ctpn_page_merge), the cut and the
page-level tail are its kernels (ctpn_page_cut, ctpn_page_text_lines), and the forward on the tiles is the ctx's ordinary batched path,
ctpn_detect_submit / ctpn_detect_collect over its two slots, at scale 1. The two tile buffers are torch uint8 tensors on the ctx's device."""
import collections

import numpy as np

from . import _binding as B

# The NMS of the page tail: 0 = ctpn_nms (one workgroup over the whole list), 1 = ctpn_page_nms (the page form of the column kernels). Both give
# the same lines. On an A4 page (20 091 proposals, 8 310 kept) the seam takes 19.1 ms as form 0 and 0.19 ms as form 1, the whole tail 22.1 and
# 3.2 ms, the page end to end 33.4 and 14.7 ms (profiles/page_throughput.json, MI355X): form 1 is the default wherever its domain holds. A page's merged proposals always lie on the
# column grid; what can leave the domain is a ctx whose TEXT_PROPOSALS_NMS_THRESH was set below 0.1, and there the default is form 0.
DEFAULT_NMS_FORM = 1

PageResult = collections.namedtuple("PageResult", "lines boxes scores src tiles grid")


def tile_shape(ctx):
    """the tile of a ctx: its max_h x max_w rounded down to the anchor grid"""
    return int(ctx.max_h) // 16 * 16, int(ctx.max_w) // 16 * 16


def ctx_connector_config(ctx):
    """the ctx's connector thresholds as the 8 values ctpn_text_lines_cfg takes"""
    return np.array([ctx.get_param(n) for n in B.CONNECTOR_PARAM_NAMES], np.float64)


def default_nms_form(ctx):
    """DEFAULT_NMS_FORM where the ctx's connector threshold is inside ctpn_page_nms's domain, 0 below it"""
    return DEFAULT_NMS_FORM if ctx.get_param("TEXT_PROPOSALS_NMS_THRESH") >= 0.1 else 0


def detect_page(ctx, page, overlap=128, mode="H", nms_form=None, line_capacity=4096):
    """Text lines of a page of any size up to 16384 x 16384, in page coordinates.

    page: (h, w, 3) uint8 BGR -- a numpy array (rows may be a view of a wider buffer) or a torch uint8 tensor on the ctx's device.
    nms_form: None (the default: default_nms_form), 0 or 1.
    overlap: pixels two neighbouring tiles share, a multiple of 32 up to half the tile's shorter side; choose it >= the tallest text
    expected (a box taller than the overlap whose centre lies near a seam is clipped by its tile).
    Returns PageResult(lines (m, 9) float64, boxes (r, 4), scores (r,), src (r,), tiles (k, 8), grid (rows, columns)): the records
    ctpn_detect returns, the merged proposals with src = tile * ctx.proposal_capacity + row, and the plan."""
    import torch
    form = default_nms_form(ctx) if nms_form is None else int(nms_form)
    if form not in (0, 1):
        raise ValueError("nms_form is 0 (ctpn_nms) or 1 (ctpn_page_nms)")
    th, tw = tile_shape(ctx)
    dev = torch.device("cuda", int(ctx.device_id))
    if isinstance(page, torch.Tensor):
        if page.dtype != torch.uint8 or page.dim() != 3 or page.shape[2] != 3 or not page.is_cuda or page.stride()[1:] != (3, 1):
            raise ValueError("detect_page wants an (h, w, 3) uint8 page (numpy, or a torch tensor on the ctx's device)")
        dpage = page
    else:
        a = np.asarray(page)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("detect_page wants an (h, w, 3) uint8 page (numpy, or a torch tensor on the ctx's device)")
        dpage = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ph, pw = int(dpage.shape[0]), int(dpage.shape[1])
    tiles, grid = B.page_plan(ph, pw, th, tw, overlap)
    k, mb, cap = tiles.shape[0], int(ctx.max_batch), ctx.proposal_capacity
    bufs = [torch.empty((min(mb, k), th, tw, 3), dtype=torch.uint8, device=dev) for _ in range(2 if k > mb else 1)]
    torch.cuda.synchronize(dev)      # the page's upload, before a stream of the library's reads it
    rois = np.zeros((k, cap, 5), np.float32)
    counts = np.zeros((k,), np.int32)
    chunks = [(first, min(mb, k - first)) for first in range(0, k, mb)]

    def collect(j):
        first, n = chunks[j]
        _, got = ctx.detect_collect(slot=j % 2, mode=mode, line_capacity=max(512, cap // 2), want_rois=True)
        for i, r in enumerate(got):
            rois[first + i, : r.shape[0]] = r
            counts[first + i] = r.shape[0]

    for j, (first, n) in enumerate(chunks):
        buf = bufs[j % len(bufs)]
        B.page_cut(None, tiles, first, n, th, tw, device_id=ctx.device_id, out_ptr=buf.data_ptr(), page_ptr=dpage.data_ptr(), page_shape=(ph, pw),
                   pitch=int(dpage.stride()[0]))
        ctx.detect_submit(device_ptr=buf.data_ptr(), shape=(n, th, tw), slot=j % 2)
        if j > 0:
            collect(j - 1)
    collect(len(chunks) - 1)
    boxes, scores, src = B.page_merge(tiles, rois, counts, ph, pw, ctx.get_param("RPN_MIN_SIZE"))
    lines = B.page_text_lines(boxes, scores, (ph, pw), mode=mode, device_id=ctx.device_id, capacity=line_capacity, config=ctx_connector_config(ctx), nms_form=form)
    return PageResult(lines, boxes, scores, src, tiles, grid)
