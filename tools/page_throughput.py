#!/usr/bin/env python
"""Throughput of the page path (ctpn_amd.detect_page) on one MI355X -> profiles/page_throughput.json.

The page: A4 at 300 dpi, 3508 x 2480, white with seeded rows of dark glyph-like marks; bf16, max_batch 32, tile 608 x 912, overlap 128 (an 8 x 3
plan: 24 tiles, one chunk). Reported:
  * tiles per page, and milliseconds per page end to end (host page in, lines out: upload, cut, forward, collect, merge, tail) with either
    nms_form -- medians of --runs alternating runs; page_ms is the default form's;
  * the tile rate (tiles / page time) as a share of the same ctx's RESIDENT batch-32 rate in the same process (a device batch of 32 tiles
    through detect_submit / detect_collect over both slots, nothing uploaded);
  * the page tail alone (ctpn_page_text_lines on the merged proposals) with nms_form 0 and nms_form 1, medians of --runs ALTERNATING runs, with
    r (merged proposals), the NMS's input (score > TEXT_PROPOSALS_MIN_SCORE) and kept counts, and the two NMS seams alone on that input.
Needs a GPU: without one the library's calls fail, there is no fallback.

    python tools/page_throughput.py [--runs 5] [--out profiles/page_throughput.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctpn_amd  # noqa: E402
from ctpn_amd import _binding as B  # noqa: E402
from ctpn_amd import page as PG  # noqa: E402

PAGE_H, PAGE_W, TILE_H, TILE_W, OVERLAP, BATCH = 3508, 2480, 608, 912, 128, 32


def synthetic_page(seed=0):
    """white paper, rows of dark marks of 8 .. 40 px height: the statistics of print, not its meaning (the weights are seeded, not trained)"""
    rng = np.random.default_rng(seed)
    page = np.full((PAGE_H, PAGE_W, 3), 245, np.uint8)
    y = 150
    while y < PAGE_H - 200:
        h = int(rng.integers(8, 41))
        x = 200
        while x < PAGE_W - 200:
            w = int(rng.integers(max(3, h // 3), h + 1))
            if rng.uniform() < 0.85:
                page[y + int(rng.integers(0, 3)): y + h, x: x + w] = rng.integers(10, 90, 3, dtype=np.uint8)
            x += w + int(rng.integers(2, max(4, h // 2)))
        y += h + int(rng.integers(h // 2 + 4, 2 * h + 8))
    return page


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return out, (time.perf_counter() - t0) * 1e3


def main(argv=None):
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_throughput.json"))
    args = ap.parse_args(argv)
    if B.device_count() < 1:
        raise SystemExit("page_throughput: no GPU visible; nothing is measured without one")
    page = synthetic_page()
    res = {"page_h": PAGE_H, "page_w": PAGE_W, "tile_h": TILE_H, "tile_w": TILE_W, "overlap": OVERLAP, "batch": BATCH, "precision": "bf16", "runs": args.runs}
    with ctpn_amd.Context(0, BATCH, TILE_H, TILE_W, "bf16") as ctx:
        ctx.load_weights(ctpn_amd.make_synthetic_arena(0))
        sync = torch.cuda.synchronize
        for form in (0, 1):                                           # warm-up: code objects, buffers, both tails
            first = ctpn_amd.detect_page(ctx, page, overlap=OVERLAP, nms_form=form)
        res["tiles_per_page"] = int(len(first.tiles))
        res["grid"] = list(first.grid)
        res["proposals_r"] = int(len(first.boxes))
        res["lines"] = int(len(first.lines))
        page_ms = {0: [], 1: []}
        for _ in range(args.runs):
            for form in (0, 1):
                page_ms[form].append(timed(lambda: ctpn_amd.detect_page(ctx, page, overlap=OVERLAP, nms_form=form), sync)[1])
        for form in (0, 1):
            res["page_ms_form%d_runs" % form] = [round(v, 2) for v in page_ms[form]]
            res["page_ms_form%d" % form] = round(statistics.median(page_ms[form]), 2)
        res["page_ms"] = res["page_ms_form%d" % PG.default_nms_form(ctx)]      # ... as detect_page runs by default
        res["tiles_per_s"] = round(res["tiles_per_page"] / (res["page_ms"] * 1e-3), 1)

        # the same ctx's resident rate: a device batch of 32 tiles, both slots, nothing uploaded
        tiles32 = torch.from_numpy(np.ascontiguousarray(B.page_cut(page, first.tiles, 0, len(first.tiles), TILE_H, TILE_W)[np.arange(BATCH) % len(first.tiles)])).cuda()
        sync()

        def resident(batches):
            for k in range(batches):
                ctx.detect_submit(device_ptr=tiles32.data_ptr(), shape=(BATCH, TILE_H, TILE_W), slot=k % 2)
                if k:
                    ctx.detect_collect(slot=(k - 1) % 2)
            ctx.detect_collect(slot=(batches - 1) % 2)
        resident(2)
        rates = []
        for _ in range(args.runs):
            _, t = timed(lambda: resident(6), sync)
            rates.append(6 * BATCH / (t * 1e-3))
        res["resident_tiles_per_s_runs"] = [round(v, 1) for v in rates]
        res["resident_tiles_per_s"] = round(statistics.median(rates), 1)
        res["tile_rate_vs_resident"] = round(res["tiles_per_s"] / res["resident_tiles_per_s"], 3)

        # the tail alone, forms alternating
        cfg8 = PG.ctx_connector_config(ctx)
        tail = {0: [], 1: []}
        lines = {}
        for _ in range(args.runs):
            for form in (0, 1):
                lines[form], t = timed(lambda: B.page_text_lines(first.boxes, first.scores, (PAGE_H, PAGE_W), device_id=0, config=cfg8, nms_form=form), sync)
                tail[form].append(t)
        res["tail_equal"] = bool(lines[0].tobytes() == lines[1].tobytes() == first.lines.tobytes())
        for form in (0, 1):
            res["tail_ms_form%d_runs" % form] = [round(v, 2) for v in tail[form]]
            res["tail_ms_form%d" % form] = round(statistics.median(tail[form]), 2)
        # ... and the NMS seams alone, on the tail's own input
        min_score = np.float32(ctx.get_param("TEXT_PROPOSALS_MIN_SCORE"))
        thr = float(ctx.get_param("TEXT_PROPOSALS_NMS_THRESH"))
        sel = np.where(first.scores > min_score)[0]
        order = sel[np.argsort(-first.scores[sel].astype(np.float64), kind="stable")]
        dets = np.concatenate([first.boxes[order], first.scores[order, None]], 1).astype(np.float32)
        res["nms_input"] = int(len(dets))
        nms = {0: [], 1: []}
        keep = {}
        for _ in range(args.runs + 1):
            for form, fn in ((0, B.nms_sorted), (1, B.page_nms_sorted)):
                keep[form], t = timed(lambda: fn(dets, thr, 0), sync)
                nms[form].append(t)
        res["nms_kept"] = int(len(keep[0]))
        res["nms_equal"] = bool(keep[0].tolist() == keep[1].tolist())
        for form in (0, 1):
            res["nms_ms_form%d_runs" % form] = [round(v, 3) for v in nms[form][1:]]
            res["nms_ms_form%d" % form] = round(statistics.median(nms[form][1:]), 3)
        res["default_nms_form"] = PG.default_nms_form(ctx)
    res["note"] = ("page_ms: host page in, lines out, one page at a time (upload, cut, one chunk of 24 tiles, collect with per-tile lines, merge, tail); "
                   "tail_ms_*: ctpn_page_text_lines from host arrays, the host's score filter, sort and connector included; nms_ms_*: the seam calls with "
                   "their copies")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
