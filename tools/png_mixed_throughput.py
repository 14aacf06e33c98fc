#!/usr/bin/env python
"""Rates of the PNG writer's table form (ctpn_encode_png_mixed, ctpn_write_line_crops_png: csrc/png_enc.hip over the one-dimensional
work-item grid). Three parts, each a set of forms INTERLEAVED run by run in this one process, --repeats runs after a warm-up of every
form, every rate with its median and its range:

    uniform   ctpn_encode_png_batch of 32 synthetic 600 x 900 "document" pictures (tools/png_encode_throughput.py's writer-alone batch),
              from host pixels and from a device-resident batch. --uniform-only stops here, and --root TREE imports the library of
              another checkout: the A/B of the uniform call across two trees is this part run alternately on both.
    mixed     the pages of the 16-size folder tools/jpeg_ragged_throughput.py builds (776 .. 2134 rows by 600 .. 1200 columns), decoded
              to host pixels: ONE ctpn_encode_png_mixed call against one ctpn_encode_png_batch call per file size -- from the pages as
              separate host arrays (both forms pack them first), and from one device-resident block (kernels and the way back only).
    crops     the text-line crops of a 600 x 900 batch as PNG files: ctpn_write_line_crops_png (cut, coded and written by the library)
              against ctpn_crop_lines + Pillow's writer one file at a time (what crops_encode='host' does).

    python tools/png_mixed_throughput.py --out profiles/png_mixed_throughput.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rates(times, count):
    r = sorted(count / t for t in times)
    return {"median": round(float(np.median(r)), 1), "min": round(r[0], 1), "max": round(r[-1], 1), "runs": [round(count / t, 1) for t in times]}


def interleaved(forms, repeats, count):
    """every form once as a warm-up, then `repeats` rounds of all forms in turn -> {form: rates}"""
    for fn in forms.values():
        fn()
    times = {f: [] for f in forms}
    for _ in range(repeats):
        for f, fn in forms.items():
            t0 = time.perf_counter()
            fn()
            times[f].append(time.perf_counter() - t0)
    return {f: rates(t, count) for f, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT, help="the checkout whose library is measured (default: this one)")
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--images", type=int, default=32, help="pages of the mixed part")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8, help="uniform part: calls per timed run")
    ap.add_argument("--lines", type=int, default=16, help="crops part: lines per image")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    from PIL import Image
    import ctpn_amd
    from decode_throughput import make_image
    out = {"root": os.path.relpath(root, ROOT), "batch": args.batch, "repeats": args.repeats}
    tmp = tempfile.mkdtemp(prefix="ctpn_png_mixed_")
    try:
        with ctpn_amd.Context(0, args.batch, 600, 900, "bf16") as ctx:
            ctx.load_weights(ctpn_amd.make_synthetic_arena(0))
            imgs = np.stack([np.ascontiguousarray(make_image(i)) for i in range(args.batch)])
            dev = torch.from_numpy(imgs).to("cuda:0")
            torch.cuda.synchronize()

            def calls(fn):
                return lambda: [fn() for _ in range(args.calls)]
            out["uniform_images_per_s"] = interleaved({"host_pixels": calls(lambda: ctx.encode_png_batch(imgs)),
                                                       "device_pixels": calls(lambda: ctx.encode_png_batch(device_ptr=dev.data_ptr(), shape=imgs.shape[:3]))},
                                                      args.repeats, args.batch * args.calls)
            out["uniform_stats"] = ctx.png_encode_device_stats()
            if not args.uniform_only:
                from ctpn_amd import _binding as B
                from jpeg_ragged_throughput import make_files
                pages_dir = os.path.join(tmp, "pages")
                os.makedirs(pages_dir)
                entries = make_files(pages_dir, args.images, 0)
                pages = [np.ascontiguousarray(np.asarray(Image.open(e[0]).convert("RGB"))[:, :, ::-1]) for e in entries]
                groups = {}
                for im in pages:
                    groups.setdefault(im.shape, []).append(im)
                mixed = ctx.encode_png_mixed(pages)
                out["mixed_file_sizes"] = len(groups)
                out["mixed_equals_host_form"] = all(f == B.png_encode(im) for f, im in list(zip(mixed, pages))[:4])
                out["mixed_mean_file_kb"] = round(float(np.mean([len(f) for f in mixed])) / 1024, 1)
                # (the bindings try a buffer of the raw size + 4096 first, encode_png_mixed a 64th more: a file above it repeats its call)
                out["mixed_files_above_raw_plus_4096"] = sum(len(f) > im.size + 4096 for f, im in zip(mixed, pages))
                # from the pages as a caller holds them, separate arrays: both forms pack them first (one block / one stack per size)
                out["mixed_images_per_s"] = interleaved({"one_mixed_call": lambda: ctx.encode_png_mixed(pages),
                                                         "one_uniform_call_per_size": lambda: [ctx.encode_png_batch(np.stack(g)) for g in groups.values()]},
                                                        args.repeats, len(pages))
                # ... and from ONE device-resident block, the pages of a size side by side: no packing, no copy in -- the kernels and the way back
                ordered = [im for g in groups.values() for im in g]
                block = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ordered])).to("cuda:0")
                torch.cuda.synchronize()
                offs = np.cumsum([0] + [im.size for im in ordered])[:-1]
                tabs = dict(heights=[im.shape[0] for im in ordered], widths=[im.shape[1] for im in ordered], pitches=[3 * im.shape[1] for im in ordered], offsets=offs)
                firsts, at = [], 0
                for g in groups.values():
                    firsts.append((int(offs[at]), (len(g),) + g[0].shape[:2]))
                    at += len(g)
                out["mixed_device_resident_images_per_s"] = interleaved(
                    {"one_mixed_call": lambda: ctx.encode_png_mixed(device_ptr=block.data_ptr(), **tabs),
                     "one_uniform_call_per_size": lambda: [ctx.encode_png_batch(device_ptr=block.data_ptr() + o, shape=s) for o, s in firsts]}, args.repeats, len(pages))
                # crops: `lines` boxes per image, 20 rows high, 150 .. 600 columns wide
                rng = np.random.default_rng(1)
                recs = []
                for _ in range(args.batch):
                    r = []
                    for k in range(args.lines):
                        x, y, w = float(rng.integers(5, 250)), 10.0 + 36.0 * k, float(rng.integers(150, 600))
                        r.append([x, y, x + w, y, x, y + 20.0, x + w, y + 20.0, 0.9])
                    recs.append(np.array(r, np.float64))
                total = args.batch * args.lines
                lib_dir, pil_dir = os.path.join(tmp, "crops_lib"), os.path.join(tmp, "crops_pillow")
                os.makedirs(lib_dir)
                os.makedirs(pil_dir)
                lib_paths = [os.path.join(lib_dir, "%05d.png" % k) for k in range(total)]

                def by_library():
                    ctx.write_line_crops(recs=recs, crop_h=32, max_w=512, device_ptr=dev.data_ptr(), shape=imgs.shape[:3], paths=lib_paths, format="png")

                def by_pillow():
                    crops, widths = ctx.crop_lines(None, recs, crop_h=32, max_w=512, device_ptr=dev.data_ptr(), shape=imgs.shape[:3])
                    for k in range(total):
                        Image.fromarray(np.ascontiguousarray(crops[k, :, :widths[k], ::-1])).save(os.path.join(pil_dir, "%05d.png" % k), compress_level=1)
                out["crops_per_s"] = interleaved({"library_png": by_library, "crop_lines_then_pillow": by_pillow}, args.repeats, total)
                out["crops"] = total
                a = np.asarray(Image.open(lib_paths[0]).convert("RGB"))
                b = np.asarray(Image.open(os.path.join(pil_dir, "00000.png")).convert("RGB"))
                out["crops_pixels_identical"] = bool(np.array_equal(a, b))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
