#!/usr/bin/env python
"""What the ragged output stage (ctpn_write_annotated_files_ragged, ctpn_crop_lines_ragged, ctpn_write_line_crops_ragged) buys on the folder
of tools/jpeg_ragged_throughput.py -- 64 JPEG files of 16 file sizes that resize_im maps to width 600 and four heights --, files in,
result files out through ctpn/demo_batch.py's run(), once with the annotated images written and once with the text-line crops written:

    (a) size-grouped device decode with the library's writers: --decode gpu --encode gpu | --crops DIR --crops-encode gpu
        (the only way to keep pixels off the host before this stage);
    (b) --ragged with the host writers: the canvas fetched and Pillow writing one file at a time (for the crops, which a ragged run
        refused before, the crops cut by ctpn_crop_lines_ragged and written by Pillow: --ragged-outputs --crops-encode host);
    (c) --ragged --ragged-outputs with the library's writers, --encode / --crops-encode gpu and gpu-entropy.

A quarter of that folder (the 9:16 pages, 1067 rows) exceeds TEST.MAX_SIZE and takes demo_batch's single-image path in EVERY form: Pillow
decode, a lone forward, the host writer. --batched-only leaves those pages out, so that the forms differ in all the work that is timed.
One process, bf16, every form warmed up, the forms alternating inside each of --repeats rounds; the median and every run.
The new kernels' times come from a profiler run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ragged_outputs_throughput.py --kernels-only
    python tools/ragged_outputs_throughput.py --out profiles/ragged_outputs_throughput.json --kernel-stats DIR
"""
import argparse
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KERNELS = ("resize_linear_mixed_kernel", "draw_boxes_ragged_kernel", "draw_boxes_kernel", "crop_lines_kernel", "jpeg_fdct_mixed_kernel", "jpeg_fdct_kernel",
           "resize_linear_kernel")

FORMS_IMAGES = {
    "a_size_grouped_gpu": dict(encode="gpu"),
    "b_ragged_host_writer": dict(ragged=True),
    "c_ragged_outputs_gpu": dict(ragged=True, ragged_outputs=True, encode="gpu"),
    "c_ragged_outputs_gpu_entropy": dict(ragged=True, ragged_outputs=True, encode="gpu-entropy"),
}
FORMS_CROPS = {
    "a_size_grouped_gpu": dict(crops_encode="gpu"),
    "b_ragged_host_writer": dict(ragged=True, ragged_outputs=True, crops_encode="host"),
    "c_ragged_outputs_gpu": dict(ragged=True, ragged_outputs=True, crops_encode="gpu"),
    "c_ragged_outputs_gpu_entropy": dict(ragged=True, ragged_outputs=True, crops_encode="gpu-entropy"),
}


def kernel_stats(directory):
    """calls and average microseconds per call of the output stage's kernels from rocprofv3's kernel_stats CSV under `directory`"""
    import csv
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in KERNELS:
                    if ("ctpn::" + k + "(") in name or ("ctpn::" + k + "<unsigned char>") in name or name.startswith(k + "("):
                        avg_ns = float(row.get("AverageNs") or row.get("Average") or 0.0)
                        out[k] = {"calls": int(row.get("Calls", 0)), "average_us": round(avg_ns / 1000.0, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batched-only", action="store_true",
                    help="leave out the pages of 1067 rows: demo_batch sends them through the single-image path (their second rescale, "
                         "TEST.MAX_SIZE, is not the identity), the same work in every form")
    ap.add_argument("--kernels-only", action="store_true", help="only form (c) 'gpu', images then crops, --kernel-calls times (the profiler's workload)")
    ap.add_argument("--kernel-calls", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="fold rocprofv3's kernel_stats CSV of a --kernels-only run into the output")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctpn_amd
    from ctpn_amd import _binding as B
    from ctpn_amd.ctpn import demo_batch as DB
    from ctpn_amd.lib.fast_rcnn.config import cfg
    from ctpn_amd.lib.networks.factory import get_network
    from jpeg_ragged_throughput import make_files
    if B.device_count() <= 0:
        raise SystemExit("no HIP device: nothing here can be measured without one")
    cfg.TEST.PRECISION = "bf16"
    net = get_network("VGGnet_test")
    net.load_arena(ctpn_amd.make_synthetic_arena(0))
    out = {"n_images": args.images, "width": 600, "max_batch": args.batch, "precision": "bf16", "repeats": args.repeats}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            src = os.path.join(tmp, "in")
            os.makedirs(src)
            entries = make_files(src, args.images, args.seed)
            if args.batched_only:
                entries = [e for e in entries if e[4][0] <= cfg.TEST.MAX_SIZE]
            names = [e[0] for e in entries]
            out["n_images"], out["batched_only"] = len(names), bool(args.batched_only)
            out["n_single_image_path"] = sum(1 for e in entries if e[4][0] > cfg.TEST.MAX_SIZE)
            out["file_sizes"] = len({e[1] for e in entries})
            counted = {}

            def one(kind, key, kw):
                d = os.path.join(tmp, "out_%s_%s" % (kind, key))
                extra = dict(write_images=True) if kind == "images" else dict(write_images=False, crops_dir=os.path.join(d, "crops"), crop_h=32)
                t0 = time.perf_counter()
                res = DB.run(net, names, d, batch=args.batch, log=lambda s: None, decode="gpu", **extra, **kw)
                dt = time.perf_counter() - t0
                counted[kind] = sum(len(r) for r in res.values())
                return len(names) / dt
            if args.kernels_only:
                for _ in range(args.kernel_calls):
                    one("images", "c_ragged_outputs_gpu", FORMS_IMAGES["c_ragged_outputs_gpu"])
                    one("crops", "c_ragged_outputs_gpu", FORMS_CROPS["c_ragged_outputs_gpu"])
                print("kernels-only: %d runs of form (c) with images and with crops, %d lines per run" % (args.kernel_calls, counted["crops"]))
                return
            for kind, forms in (("images", FORMS_IMAGES), ("crops", FORMS_CROPS)):
                for key, kw in forms.items():      # warm-up: every geometry and buffer of every form once
                    one(kind, key, kw)
                rates = {k: [] for k in forms}
                for _ in range(args.repeats):
                    for key, kw in forms.items():
                        rates[key].append(one(kind, key, kw))
                out[kind] = {k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1), "runs": [round(x, 1) for x in v]}
                             for k, v in rates.items()}
                med = {k: out[kind][k]["median"] for k in rates}
                out[kind]["c_gpu_over_a"] = round(med["c_ragged_outputs_gpu"] / med["a_size_grouped_gpu"], 3)
                out[kind]["c_gpu_over_b"] = round(med["c_ragged_outputs_gpu"] / med["b_ragged_host_writer"], 3)
            out["lines_per_run"] = counted.get("crops", 0)
    finally:
        net.close()
    if args.kernel_stats:
        out["kernels_form_c"] = {"runs": args.kernel_calls, "per_call": kernel_stats(args.kernel_stats)}
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
