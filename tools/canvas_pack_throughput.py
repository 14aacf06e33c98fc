#!/usr/bin/env python
"""What building ragged PNG canvases on the device (ctpn_decode_png_files_ragged; ctpn/demo_batch.py --ragged-pack gpu) buys on a folder of
portrait pages whose FILES have many sizes: PNG files of 16 file sizes that resize_im maps to width 600 and heights 776 (letter), 800
(3:4), 849 (A4) and 1067 (9:16) -- tools/jpeg_ragged_throughput.py's folder as PNG files --, detected three ways through the pipelined
submit / collect pair, files to text lines, each form as ctpn/demo_batch.py runs it:

    (a) the size-grouped device path: --decode gpu [--ragged] without the switch -- one batch per FILE size, decoded by the library's C++
        threads one job ahead (ctpn_decode_png_files), resized on the device (ctpn_resize), submitted from the host;
    (b) --ragged-png's host canvas: batches by RESIZED shape, every file through the host loader and resize_im, the zero-padded canvas
        built with numpy and copied to the device by the submit;
    (c) --ragged-pack gpu: the same batches, the files decoded by the library's pool into page-locked memory, one copy, one kernel
        (canvas_pack_kernel), submitted where the canvas lies.

(a) and (b) are the code paths the library had before (c) existed; (c) is compared against them, never against itself. One process, the
forms interleaved, --repeats times after a warm-up of every form; medians with their spread. The box-to-box spread of such rates is
about +-3 % (README): a ratio inside it is no difference.

    python tools/canvas_pack_throughput.py --out profiles/canvas_pack_throughput.json
"""
import argparse
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


def make_files(directory, images, seed):
    """-> [(path, file (h, w), layout, factor, resized (h, w))], the entries demo_batch.plan_device_jobs takes"""
    from PIL import Image
    import ctpn_amd
    from ctpn_amd import _binding as B
    from ctpn_amd.ctpn import demo as D
    from ctpn_amd.ctpn import demo_batch as DB
    from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg
    rng = np.random.default_rng(seed)
    kinds = [(HEIGHTS[int(rng.integers(4))], FILE_SCALES[int(rng.integers(4))]) for _ in range(images)]
    made, entries = {}, []
    for k, (hr, s) in enumerate(kinds):
        if (hr, s) not in made:      # one picture per file size (the content does not matter to any rate here; generating 64 large ones does)
            h, w = int(round(hr * s)), int(round(600 * s))
            f = D.resize_factor((h, w), TextLineCfg.SCALE, TextLineCfg.MAX_SCALE)
            rs = (h, w) if f == 1.0 else B.resize_dims(h, w, f, f)
            assert rs == (hr, 600), ((h, w), f, rs)
            first = os.path.join(directory, "kind%02d.png" % len(made))
            Image.fromarray(np.ascontiguousarray(ctpn_amd.weights.synthetic_images(1, h, w, 100 + len(made))[0][:, :, ::-1])).save(first, compress_level=6)
            made[hr, s] = (open(first, "rb").read(), (h, w), f, rs)
            os.remove(first)
        data, size, f, rs = made[hr, s]
        path = os.path.join(directory, "page%03d.png" % k)
        with open(path, "wb") as fh:
            fh.write(data)
        entries.append((path, size, DB.PNG_LAYOUT, f, rs))
    return entries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--read-threads", type=int, default=8, help="form (a): the library's PNG decode threads, as demo_batch passes them")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctpn_amd
    from ctpn_amd import _binding as B
    from ctpn_amd.ctpn import demo_batch as DB
    from ctpn_amd.lib.utils.blob import im_list_to_canvas
    if B.device_count() <= 0:
        raise SystemExit("no HIP device: nothing here can be measured without one")
    arena = ctpn_amd.make_synthetic_arena(0)
    out = {"images": args.images, "width": 600, "max_batch": args.batch, "precision": args.precision, "repeats": args.repeats, "waste": DB.RAGGED_WASTE}
    with tempfile.TemporaryDirectory() as tmp:
        entries = make_files(tmp, args.images, args.seed)
        jobs_a = DB.plan_device_jobs(entries, args.batch, ragged=True)
        jobs_b = DB.plan_device_jobs(entries, args.batch, ragged=True, ragged_png=True)
        jobs_c = DB.plan_device_jobs(entries, args.batch, ragged=True, ragged_pack="gpu")
        assert all(j[1] == "png" for j in jobs_a) and [j[1:] for j in jobs_b if j[1] == "ragged-png"] == [("ragged-png",) + j[2:] for j in jobs_c if j[1] == "ragged-png-gpu"]
        out["file_sizes"] = len({e[1] for e in entries})
        out["resized_heights"] = {str(h): sum(1 for e in entries if e[4][0] == h) for h in HEIGHTS}
        out["batches"] = {"a_size_grouped": [len(j[4]) for j in jobs_a], "b_ragged_host_canvas": [len(j[4]) for j in jobs_b], "c_ragged_pack_gpu": [len(j[4]) for j in jobs_c]}
        with ctpn_amd.Context(0, args.batch, max(HEIGHTS), 600, args.precision) as ctx:
            ctx.load_weights(arena)

            def uniform_png(job):
                (h, w), _, f, rs, members = job
                imgs = B.decode_png_files(members, h, w, args.read_threads)
                return imgs if f == 1.0 else B.resize_linear(imgs, f, f)

            def run(jobs):
                from concurrent.futures import ThreadPoolExecutor
                t0 = time.perf_counter()
                with ThreadPoolExecutor(max_workers=1) as pool:      # demo_batch's 'png' jobs are decoded one job ahead
                    ahead = {0: pool.submit(uniform_png, jobs[0])} if jobs[0][1] == "png" else {}
                    for k, job in enumerate(jobs):
                        (h, w), kind, f, rs, members = job
                        if k + 1 < len(jobs) and jobs[k + 1][1] == "png":
                            ahead[k + 1] = pool.submit(uniform_png, jobs[k + 1])
                        if kind == "png":
                            ctx.detect_submit(images=ahead.pop(k).result(), slot=k & 1)
                        elif kind == "ragged-png":
                            canvas, heights = im_list_to_canvas([DB._load(nm)[0] for nm in members])
                            ctx.detect_submit(images=canvas, heights=heights, slot=k & 1)
                        else:
                            (ptr, shape), heights = ctx.decode_png_ragged(members, [t[:2] for t in f], [t[2] for t in f], h, w)
                            ctx.detect_submit(device_ptr=ptr, shape=shape, heights=heights, slot=k & 1)
                        if k:
                            ctx.detect_collect((k - 1) & 1, line_capacity=1024)
                    ctx.detect_collect((len(jobs) - 1) & 1, line_capacity=1024)
                return args.images / (time.perf_counter() - t0)
            forms = {"a_size_grouped": jobs_a, "b_ragged_host_canvas": jobs_b, "c_ragged_pack_gpu": jobs_c}
            for jobs in forms.values():      # warm-up: every geometry of every form once
                run(jobs)
            rates = {k: [] for k in forms}
            for _ in range(args.repeats):
                for k, jobs in forms.items():
                    rates[k].append(run(jobs))
        out["images_per_s"] = {k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1), "runs": [round(x, 1) for x in v]}
                               for k, v in rates.items()}
        med = {k: out["images_per_s"][k]["median"] for k in rates}
        out["c_over_a"] = round(med["c_ragged_pack_gpu"] / med["a_size_grouped"], 3)
        out["c_over_b"] = round(med["c_ragged_pack_gpu"] / med["b_ragged_host_canvas"], 3)
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
