#!/usr/bin/env python
"""Rate of the PNG writer (ctpn_encode_png_batch / ctpn_write_annotated_png_files: csrc/png_enc.hip) against the host form of the same file
(ctpn_png_encode) and against Pillow's compress_level=1 writer, which is what lib/utils/image.py's imwrite uses for a PNG-named output.

    python tools/png_encode_throughput.py --images 256 --out profiles/png_encode_throughput.json

Writer alone: one batch of 32 synthetic 600 x 900 "document" pictures (tools/decode_throughput.py's) in host memory, coded to bytes in
memory again and again, the three forms INTERLEAVED call by call in this one process: the device form (host pixels in, files out: the
host-to-device copy is part of the call), ctpn_png_encode on as many threads as the ctx's pool has, and Pillow on the Python thread. Per
form: images/s (median and every round), host CPU seconds per 1000 images (process time: all threads), and for the device form the
device-to-host bytes per image. Then the mean file size of the library's files against Pillow's of the same pictures, and
ctpn/demo_batch.py::run over a directory of PNG files with png_encode='gpu' against 'host'. Prints one JSON line."""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256, help="PNG files of the demo_batch part")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "split", "fp32"])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=8, help="timed calls per form of the writer-alone part")
    ap.add_argument("--kernels-only", action="store_true", help="a few encoder calls on a device-resident batch and nothing else (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from PIL import Image
    from decode_throughput import make_image
    from ctpn_amd import _binding as B
    from ctpn_amd.ctpn import demo as D, demo_batch as DB
    from ctpn_amd.lib.networks.factory import get_network
    from ctpn_amd.lib.fast_rcnn.config import cfg, cfg_from_file

    threads = B.host_thread_budget(os.cpu_count() or 1, 1, 0)
    out = {"batch": args.batch, "height": 600, "width": 900, "precision": args.precision, "host_cpus": os.cpu_count(), "host_thread_budget": threads}
    tmp = tempfile.mkdtemp(prefix="ctpn_png_encode_")
    try:
        cfg_from_file(os.path.join(ROOT, "text-detection-ctpn_amd", "ctpn", "text.yml"))
        cfg.TEST.PRECISION = args.precision
        net = get_network("VGGnet_test")
        D.load_weights(net, 0)
        net.ensure_capacity(args.batch, 600, 900)
        imgs = np.stack([np.ascontiguousarray(make_image(i)) for i in range(args.batch)])
        if args.kernels_only:
            names = []
            for i in range(args.batch):
                names.append(os.path.join(tmp, "k_%02d.jpg" % i))
                Image.fromarray(imgs[i][:, :, ::-1].copy()).save(names[-1], quality=95)
            ptr, shape = net.ctx.decode_jpeg_files(names, 600, 900)
            for _ in range(5):
                net.ctx.encode_png_batch(device_ptr=ptr, shape=shape)
            out["kernels_only_calls"] = 5
            net.close()
            print(json.dumps(out))
            return
        pool = ThreadPoolExecutor(max_workers=threads)

        def pillow(batch):
            files = []
            for im in batch:
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(im[:, :, ::-1])).save(buf, "PNG", compress_level=1)
                files.append(buf.getvalue())
            return files
        forms = {"device": lambda: net.ctx.encode_png_batch(imgs), "host_form": lambda: list(pool.map(B.png_encode, imgs)), "pillow": lambda: pillow(imgs)}
        files = {f: fn() for f, fn in forms.items()}      # warm-up: buffers grown
        out["device_equals_host_form"] = files["device"] == files["host_form"]
        out["lossless"] = all(np.array_equal(np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[:, :, ::-1], im) for f, im in zip(files["device"], imgs))
        out["mean_file_kb"] = round(float(np.mean([len(f) for f in files["device"]])) / 1024, 1)
        out["mean_pillow_file_kb"] = round(float(np.mean([len(f) for f in files["pillow"]])) / 1024, 1)
        out["file_size_vs_pillow"] = round(out["mean_file_kb"] / out["mean_pillow_file_kb"], 3)
        wall, cpu = {f: [] for f in forms}, {f: 0.0 for f in forms}
        for _ in range(args.rounds):
            for f, fn in forms.items():
                c0, t0 = time.process_time(), time.perf_counter()
                fn()
                wall[f].append(time.perf_counter() - t0)
                cpu[f] += time.process_time() - c0
                if f == "device":
                    st = net.ctx.png_encode_device_stats()
                    out["device_d2h_bytes_per_image"] = round(st["d2h_bytes"] / args.batch, 1)
                    out["device_files_on_device"], out["device_files_on_host"] = st["device"], st["host"]
        for f in forms:
            out["writer_only_%s_images_per_s" % f] = round(args.batch / float(np.median(wall[f])), 1)
            out["writer_only_%s_rounds_images_per_s" % f] = [round(args.batch / t, 1) for t in wall[f]]
            out["writer_only_%s_host_cpu_s_per_1000_images" % f] = round(1000.0 * cpu[f] / (args.rounds * args.batch), 3)
        pool.shutdown()
        # files in, lines and pictures out: a directory of PNG files
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        distinct = min(args.batch * 2, args.images)
        for i in range(args.images):
            p = os.path.join(src, "img_%04d.png" % i)
            if i < distinct:
                Image.fromarray(make_image(i)[:, :, ::-1].copy()).save(p, compress_level=1)
            else:
                shutil.copyfile(os.path.join(src, "img_%04d.png" % (i % distinct)), p)
        names = DB.list_images(src)
        quiet = lambda *a: None  # noqa: E731
        for key in ("host", "gpu"):
            od = os.path.join(tmp, "out_" + key)
            DB.run(net, names[: args.batch * 2], od, batch=args.batch, log=quiet, decode="gpu", png_encode=key)      # warm-up
            rates = []
            for _ in range(args.repeats):
                t0 = time.time()
                DB.run(net, names, od, batch=args.batch, log=quiet, decode="gpu", png_encode=key)
                rates.append(round(len(names) / (time.time() - t0), 1))
            out["demo_batch_png_encode_%s_images_per_s" % key] = max(rates)
            out["demo_batch_png_encode_%s_runs" % key] = rates
        out["demo_batch_images"] = len(names)
        out["demo_batch_gpu_vs_host"] = round(out["demo_batch_png_encode_gpu_images_per_s"] / out["demo_batch_png_encode_host_images_per_s"], 2)
        same = True
        for nm in names[: args.batch]:
            a, b = (np.asarray(Image.open(os.path.join(tmp, "out_" + k, os.path.basename(nm))).convert("RGB")) for k in ("host", "gpu"))
            same = same and np.array_equal(a, b)
        out["demo_batch_pixels_identical"] = bool(same)
        net.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    txt = json.dumps(out)
    print(txt)
    if args.out:
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
