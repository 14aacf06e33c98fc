"""The text-line tail on dense pages at RPN_POST_NMS_TOP_N = 4096 (ctpn_reserve_proposals): the large device connector against the host
connector, through ctpn_debug_text_lines -- the function the detect path's tail calls -- on the 40 x 64 and 64 x 64 pages of
tests/dense_pages.py (2560 and 4096 line slices per image) at batch 1 and batch 32. Writes profiles/dense_pages.json.

What a figure is: wall-clock milliseconds of one ctpn_debug_text_lines call, which uploads the rois, runs lines_prep_kernel, the connector's
NMS and (connect_device = 1) connect_large_kernel, copies the results back, synchronises, and (connect_device = 0) runs connect_lines on the
ctx's host workers. The two forms alternate inside every round (same process, same ctx, same inputs); reported: the median over the rounds
of a round's mean call time, and the smallest and largest round. Both forms' records are compared byte for byte before anything is timed.

    python tools/dense_page_throughput.py [--rounds 9] [--calls 20] [--out profiles/dense_pages.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ctpn_amd  # noqa: E402
from ctpn_amd import _binding as B  # noqa: E402
import dense_pages as D  # noqa: E402

POST = 4096
SIZE = (1024, 1024)
FORMS = (("device_buckets", 1), ("host", 0))


def one_call(ctx, packed, rcnt, scales, recs, lcnt, keep, kcnt):
    n = packed.shape[0]
    B._check(ctx._lib.ctpn_debug_text_lines(ctx._h, B._ptr(packed, C.c_float), B._ptr(rcnt, C.c_int), n, SIZE[0], SIZE[1], B._ptr(scales, C.c_float), B.MODE_H,
                                            B._ptr(recs, C.c_double), recs.shape[1], B._ptr(lcnt, C.c_int), B._ptr(keep, C.c_int), B._ptr(kcnt, C.c_int)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_pages.json"))
    args = ap.parse_args(argv)
    if B.device_count() < 1:
        raise SystemExit("no GPU: nothing is measured without one")
    result = {"what": "ms per ctpn_debug_text_lines call, RPN_POST_NMS_TOP_N = 4096, mode H; median [min, max] over rounds of a round's mean",
              "rounds": args.rounds, "calls_per_round": args.calls, "host_threads": None, "cells": []}
    with ctpn_amd.Context(0, 32, SIZE[0], SIZE[1], postproc_only=True) as ctx:
        ctx.reserve_proposals(POST)
        ctx.set_param("RPN_POST_NMS_TOP_N", POST)
        result["host_threads"] = ctx.host_threads()
        for page in ("40x64", "64x64"):
            rois = D.oracle_rois(page)
            for n in (1, 32):
                packed = np.ascontiguousarray(np.broadcast_to(rois, (n,) + rois.shape), np.float32)
                rcnt = np.full((n,), rois.shape[0], np.int32)
                scales = np.ones((n,), np.float32)
                bufs = {}
                for name, cd in FORMS:
                    bufs[name] = (np.zeros((n, 2048, 9), np.float64), np.zeros((n,), np.int32), np.zeros((n, POST), np.int32), np.zeros((n,), np.int32))
                    ctx.set_option("connect_device", cd)
                    for _ in range(3):      # warm-up: code objects, the pool
                        one_call(ctx, packed, rcnt, scales, *bufs[name])
                a, b = bufs["device_buckets"], bufs["host"]
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "the two connectors differ"
                plan = B.text_line_plan(n, SIZE[1] // 16, POST, connect_device=1)
                per = {name: [] for name, _ in FORMS}
                for _ in range(args.rounds):
                    for name, cd in FORMS:
                        ctx.set_option("connect_device", cd)
                        one_call(ctx, packed, rcnt, scales, *bufs[name])
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            one_call(ctx, packed, rcnt, scales, *bufs[name])
                        per[name].append((time.perf_counter() - t0) * 1e3 / args.calls)
                cell = {"page": page, "batch": n, "line_slices_per_image": D.slices_above(page), "kept_per_image": int(a[3][0]), "lines_per_image": int(a[1][0]),
                        "plan_device": list(plan)}
                for name, _ in FORMS:
                    cell[name] = {"median_ms": round(statistics.median(per[name]), 4), "min_ms": round(min(per[name]), 4), "max_ms": round(max(per[name]), 4)}
                print(json.dumps(cell))
                result["cells"].append(cell)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
