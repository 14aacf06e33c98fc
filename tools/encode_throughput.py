#!/usr/bin/env python
"""Rate of the batch demo path WITH its annotated images (ctpn/demo.py:28-52: draw_boxes, cv2.resize by 1 / scale, cv2.imwrite), the mode
the reference runs in and no other tool here measures (tools/decode_throughput.py passes write_images=False).

    python tools/encode_throughput.py --images 512 --out profiles/encode_throughput.json

Writes N synthetic 600 x 900 "document" JPEG files (tools/decode_throughput.py's pictures) into a scratch directory and runs
ctpn/demo_batch.py::run over them with decode='gpu' three ways in ONE process: write_images=False, write_images=True with encode='host'
(every batch fetched to the host, drawn there, written by Pillow on the Python thread) and with encode='gpu' (ctpn_write_annotated_files:
outlines, resize, colour conversion, DCT and quantiser as HIP kernels, Huffman coding and file writing on the ctx's C++ pool). Checks that the two
writers' files are byte-identical and prints one JSON line. --kernels-only: a few encoder calls and nothing else (the run to put under
`rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--distinct", type=int, default=64, help="encode only this many distinct input images and copy them under --images names")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "split", "fp32"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from PIL import Image
    from decode_throughput import make_image
    from ctpn_amd import _binding as B
    from ctpn_amd.ctpn import demo as D, demo_batch as DB
    from ctpn_amd.lib.networks.factory import get_network
    from ctpn_amd.lib.fast_rcnn.config import cfg, cfg_from_file

    tmp = tempfile.mkdtemp(prefix="ctpn_encode_")
    out = {"images": args.images, "batch": args.batch, "height": 600, "width": 900, "precision": args.precision, "host_cpus": os.cpu_count(),
           "host_thread_budget": B.host_thread_budget(os.cpu_count() or 1, 1, 0)}
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        distinct = min(args.distinct, args.images)
        for i in range(args.images):
            p = os.path.join(src, "img_%04d.jpg" % i)
            if i < distinct:
                Image.fromarray(make_image(i)[:, :, ::-1].copy()).save(p, quality=90)
            else:
                shutil.copyfile(os.path.join(src, "img_%04d.jpg" % (i % distinct)), p)
        cfg_from_file(os.path.join(ROOT, "text-detection-ctpn_amd", "ctpn", "text.yml"))
        cfg.TEST.PRECISION = args.precision
        net = get_network("VGGnet_test")
        D.load_weights(net, 0)
        names = DB.list_images(src)
        quiet = lambda *a: None  # noqa: E731
        if args.kernels_only:
            net.ensure_capacity(args.batch, 600, 900)
            ptr, shape = net.ctx.decode_jpeg_files(names[: args.batch], 600, 900)
            recs = net.ctx.detect(device_ptr=ptr, shape=shape)
            paths = [os.path.join(tmp, "k_%d.jpg" % i) for i in range(args.batch)]
            for _ in range(5):
                net.ctx.write_annotated_files(ptr, shape, recs, 1.0, paths)
            out["kernels_only_calls"] = 5
        else:
            modes = (("no_images", dict(write_images=False)), ("encode_host", dict(write_images=True, encode="host")),
                     ("encode_gpu", dict(write_images=True, encode="gpu")))
            for key, kw in modes:
                od = os.path.join(tmp, "out_" + key)
                DB.run(net, names[: args.batch * 2], od, batch=args.batch, log=quiet, decode="gpu", **kw)      # warm-up: buffers grown, files cached
                rates = []
                for _ in range(args.repeats):
                    t0 = time.time()
                    DB.run(net, names, od, batch=args.batch, log=quiet, decode="gpu", **kw)
                    rates.append(round(len(names) / (time.time() - t0), 1))
                out[key + "_images_per_s"] = max(rates)
                out[key + "_runs"] = rates
            same = all(open(os.path.join(tmp, "out_encode_host", os.path.basename(nm)), "rb").read() ==
                       open(os.path.join(tmp, "out_encode_gpu", os.path.basename(nm)), "rb").read() for nm in names)
            out["files_identical"] = bool(same)
            out["mean_output_kb"] = round(float(np.mean([os.path.getsize(os.path.join(tmp, "out_encode_gpu", os.path.basename(nm))) for nm in names])) / 1024, 1)
            out["encode_gpu_vs_host"] = round(out["encode_gpu_images_per_s"] / out["encode_host_images_per_s"], 2)
            # the writer alone: one live batch, its lines, written again and again
            ptr, shape = net.ctx.decode_jpeg_files(names[: args.batch], 600, 900)
            recs = net.ctx.detect(device_ptr=ptr, shape=shape)
            paths = [os.path.join(tmp, "w_%d.jpg" % i) for i in range(args.batch)]
            net.ctx.write_annotated_files(ptr, shape, recs, 1.0, paths)
            t0 = time.time()
            for _ in range(10):
                net.ctx.write_annotated_files(ptr, shape, recs, 1.0, paths)
            out["write_annotated_files_only_images_per_s"] = round(10 * args.batch / (time.time() - t0), 1)
        net.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    txt = json.dumps(out)
    print(txt)
    if args.out:
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
