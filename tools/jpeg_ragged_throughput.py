#!/usr/bin/env python
"""What the ragged device JPEG decode (ctpn_decode_jpeg_files_ragged) buys on a folder of portrait pages whose FILES have many sizes:
JPEG files of 16 file sizes and three chroma layouts that resize_im maps to width 600 and heights 776 (letter), 800 (3:4), 849 (A4) and
1067 (9:16) -- plan_ragged_batches' own example --, detected three ways through the pipelined submit / collect pair, files to text lines:

    (a) size-grouped device decode + uniform detect: ctpn/demo_batch.py --decode gpu without --ragged (one batch per file size and layout);
    (b) ragged device decode + ragged detect: --decode gpu --ragged (batches by RESIZED shape, whatever the file sizes);
    (c) --ragged with the host decoder: Pillow + resize_im on a thread pool one batch ahead, canvases built on the host.

One process, the forms interleaved, --repeats times after a warm-up of every form; every rate with its spread. --entropy device: (a) and (b)
with the Huffman decode on the device too.
The kernels themselves are compared on ONE uniform batch (900 x 1350 files -> 600 x 900): the uniform call's jpeg_color_kernel +
resize_linear_kernel against the ragged call's fused jpeg_color_resize_ragged_kernel, from a profiler run of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/jpeg_ragged_throughput.py --kernels-only
    python tools/jpeg_ragged_throughput.py --out profiles/jpeg_ragged_throughput.json --kernel-stats DIR
"""
import argparse
import glob
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHTS = (776, 800, 849, 1067)
FILE_SCALES = (1.0, 1.25, 1.5, 2.0)
KERNELS = ("jpeg_idct_kernel", "jpeg_color_kernel", "resize_linear_kernel", "jpeg_idct_ragged_kernel", "jpeg_color_resize_ragged_kernel")


def jpeg_bytes(bgr, subsampling, quality=90):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def make_files(directory, images, seed):
    """-> [(path, file (h, w), layout, factor, resized (h, w))], the entries demo_batch.plan_device_jobs takes"""
    import ctpn_amd
    from ctpn_amd import _binding as B
    from ctpn_amd.ctpn import demo as D
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    rng = np.random.default_rng(seed)
    kinds, made = [], {}
    for k in range(images):
        kinds.append((HEIGHTS[int(rng.integers(4))], FILE_SCALES[int(rng.integers(4))]))
    entries = []
    for k, (hr, s) in enumerate(kinds):
        if (hr, s) not in made:      # one picture per file size (the content does not matter to any rate here; generating 64 large ones does)
            h, w = int(round(hr * s)), int(round(600 * s))
            f = D.resize_factor((h, w), TextLineCfg.SCALE, TextLineCfg.MAX_SCALE)
            rs = (h, w) if f == 1.0 else B.resize_dims(h, w, f, f)
            assert rs == (hr, 600), ((h, w), f, rs)
            sub = (2, 0, 1)[len(made) % 3]
            made[hr, s] = (jpeg_bytes(ctpn_amd.weights.synthetic_images(1, h, w, 100 + len(made))[0], sub), (h, w), f, rs)
        data, size, f, rs = made[hr, s]
        path = os.path.join(directory, "page%03d.jpg" % k)
        with open(path, "wb") as fh:
            fh.write(data)
        pr = B.jpeg_probe(data)
        assert pr[:2] == size
        entries.append((path, size, (pr[2], pr[3]), f, rs))
    return entries


def kernel_stats(directory):
    """average microseconds per call of the decoder's kernels from rocprofv3's kernel_stats CSV under `directory`"""
    import csv
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in KERNELS:
                    if ("ctpn::" + k + "(") in name or ("ctpn::" + k + "<") in name or name.startswith(k):
                        avg_ns = float(row.get("AverageNs") or row.get("Average") or 0.0)
                        out[k + ("<float>" if "<float>" in name else "")] = {"calls": int(row.get("Calls", 0)), "average_us": round(avg_ns / 1000.0, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--entropy", default="host", choices=["host", "device"])
    ap.add_argument("--decode-threads", type=int, default=8, help="form (c): host threads decoding the next batch")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernels-only", action="store_true", help="only the uniform 900 x 1350 -> 600 x 900 batch through both calls (the profiler's workload)")
    ap.add_argument("--kernel-batch", type=int, default=8)
    ap.add_argument("--kernel-calls", type=int, default=10)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="fold rocprofv3's kernel_stats CSV of a --kernels-only run into the output")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctpn_amd
    from ctpn_amd import _binding as B
    from ctpn_amd.ctpn import demo_batch as DB
    from ctpn_amd.lib.utils.blob import im_list_to_canvas
    if B.device_count() <= 0:
        raise SystemExit("no HIP device: nothing here can be measured without one")
    arena = ctpn_amd.make_synthetic_arena(0)

    if args.kernels_only:
        files = [jpeg_bytes(ctpn_amd.weights.synthetic_images(1, 900, 1350, 7 + i)[0], 2) for i in range(args.kernel_batch)]
        f = 600.0 / 900.0
        with ctpn_amd.Context(0, args.kernel_batch, 600, 900, args.precision) as ctx:
            want = None
            for _ in range(args.kernel_calls):
                ptr, shape = ctx.decode_jpeg_batch(files, 900, 1350, f, f)
                uni = ctx.jpeg_batch_fetch(ptr, shape)
                (ptr, shape), heights = ctx.decode_jpeg_ragged(files, [(900, 1350)] * len(files), [f] * len(files), 600, 900)
                rag = ctx.jpeg_batch_fetch(ptr, shape)
                assert shape == (len(files), 600, 900) and np.array_equal(uni, rag), "the two calls' images differ"
                want = uni
        print("kernels-only: %d calls of each form on %d files 900 x 1350 -> %s, byte-equal" % (args.kernel_calls, len(files), want.shape[1:3]))
        return

    out = {"images": args.images, "width": 600, "max_batch": args.batch, "precision": args.precision, "entropy": args.entropy, "repeats": args.repeats,
           "waste": DB.RAGGED_WASTE}
    with tempfile.TemporaryDirectory() as tmp:
        entries = make_files(tmp, args.images, args.seed)
        jobs_a = DB.plan_device_jobs(entries, args.batch)
        jobs_b = DB.plan_device_jobs(entries, args.batch, ragged=True)
        by_name = {e[0]: e for e in entries}
        batches_c, alone_c = DB.plan_ragged_batches([e[4] for e in entries], args.batch)
        jobs_c = [[entries[i][0] for i in m] for _, m in batches_c] + [[entries[i][0]] for i in alone_c]
        out["file_sizes"] = len({e[1] for e in entries})
        out["resized_heights"] = {str(h): sum(1 for e in entries if e[4][0] == h) for h in HEIGHTS}
        out["batches"] = {"a_size_grouped": [len(j[4]) for j in jobs_a], "b_ragged_device": [len(j[4]) for j in jobs_b], "c_ragged_host": [len(j) for j in jobs_c]}
        with ctpn_amd.Context(0, args.batch, max(HEIGHTS), 600, args.precision) as ctx:
            ctx.load_weights(arena)

            def device_run(jobs):
                t0 = time.perf_counter()
                for k, ((h, w), kind, f, rs, members) in enumerate(jobs):
                    if kind == "ragged":
                        (ptr, shape), heights = ctx.decode_jpeg_ragged(members, [t[:2] for t in f], [t[2] for t in f], h, w, entropy=args.entropy)
                        ctx.detect_submit(device_ptr=ptr, shape=shape, heights=heights, slot=k & 1)
                    else:
                        ptr, shape = ctx.decode_jpeg_files(members, h, w, f, f, entropy=args.entropy)
                        ctx.detect_submit(device_ptr=ptr, shape=shape, slot=k & 1)
                    if k:
                        ctx.detect_collect((k - 1) & 1, line_capacity=1024)
                ctx.detect_collect((len(jobs) - 1) & 1, line_capacity=1024)
                return args.images / (time.perf_counter() - t0)

            def host_run(jobs):
                from concurrent.futures import ThreadPoolExecutor
                t0 = time.perf_counter()
                with ThreadPoolExecutor(max_workers=max(1, args.decode_threads)) as pool:
                    ahead = [pool.submit(DB._load, nm) for nm in jobs[0]]
                    for k, members in enumerate(jobs):
                        imgs = [fu.result()[0] for fu in ahead]
                        ahead = [pool.submit(DB._load, nm) for nm in jobs[k + 1]] if k + 1 < len(jobs) else []
                        assert all(im.shape[:2] == tuple(by_name[nm][4]) for im, nm in zip(imgs, members))
                        canvas, heights = im_list_to_canvas(imgs)
                        ctx.detect_submit(images=canvas, heights=heights, slot=k & 1)
                        if k:
                            ctx.detect_collect((k - 1) & 1, line_capacity=1024)
                    ctx.detect_collect((len(jobs) - 1) & 1, line_capacity=1024)
                return args.images / (time.perf_counter() - t0)
            forms = {"a_size_grouped": (device_run, jobs_a), "b_ragged_device": (device_run, jobs_b), "c_ragged_host": (host_run, jobs_c)}
            for fn, jobs in forms.values():      # warm-up: every geometry of every form once
                fn(jobs)
            rates = {k: [] for k in forms}
            for _ in range(args.repeats):
                for k, (fn, jobs) in forms.items():
                    rates[k].append(fn(jobs))
        out["images_per_s"] = {k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1), "runs": [round(x, 1) for x in v]}
                               for k, v in rates.items()}
        med = {k: out["images_per_s"][k]["median"] for k in rates}
        out["b_over_a"] = round(med["b_ragged_device"] / med["a_size_grouped"], 3)
        out["b_over_c"] = round(med["b_ragged_device"] / med["c_ragged_host"], 3)
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        out["kernels_900x1350_to_600x900"] = {"batch": args.kernel_batch, "average_us_per_call": ks}
        if "jpeg_color_kernel" in ks and "resize_linear_kernel" in ks and "jpeg_color_resize_ragged_kernel" in ks:
            two = ks["jpeg_color_kernel"]["average_us"] + ks["resize_linear_kernel"]["average_us"]
            out["kernels_900x1350_to_600x900"]["colour_plus_resize_us"] = round(two, 2)
            out["kernels_900x1350_to_600x900"]["fused_over_two"] = round(ks["jpeg_color_resize_ragged_kernel"]["average_us"] / two, 3)
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
