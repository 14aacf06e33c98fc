#!/usr/bin/env python
"""Rate of the batch demo path WITH its annotated images (ctpn/demo.py:28-52: draw_boxes, cv2.resize by 1 / scale, cv2.imwrite), the mode
the reference runs in and no other tool here measures (tools/decode_throughput.py passes write_images=False).

    python tools/encode_throughput.py --images 512 --out profiles/encode_throughput.json

Writes N synthetic 600 x 900 "document" JPEG files (tools/decode_throughput.py's pictures) into a scratch directory and runs
ctpn/demo_batch.py::run over them with decode='gpu' three ways in ONE process: write_images=False, write_images=True with encode='host'
(every batch fetched to the host, drawn there, written by Pillow on the Python thread) and with encode='gpu' (ctpn_write_annotated_files:
outlines, resize, colour conversion, DCT and quantiser as HIP kernels, Huffman coding and file writing on the ctx's C++ pool). Checks that the two
writers' files are byte-identical and prints one JSON line. --kernels-only: a few encoder calls and nothing else (the run to put under
`rocprofv3 --kernel-trace --stats`).
--entropy host|device|both chooses the writer's entropy form(s): host (default) is ctpn_write_annotated_files, device is
ctpn_write_annotated_files_device (Huffman coding on the device too, demo_batch's encode='gpu-entropy'). With both, the writer-alone part
runs the two forms INTERLEAVED, call by call, in this one process, and reports per form: images/s (median and every round), host CPU
seconds per 1000 images (process time: the C++ pool's threads included) and device-to-host bytes per image."""
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
    ap.add_argument("--entropy", default="host", choices=["host", "device", "both"], help="entropy form(s) of the library's writer")
    ap.add_argument("--rounds", type=int, default=10, help="timed calls per form of the writer-alone part")
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
        forms = ("host", "device") if args.entropy == "both" else (args.entropy,)
        if args.kernels_only:
            net.ensure_capacity(args.batch, 600, 900)
            ptr, shape = net.ctx.decode_jpeg_files(names[: args.batch], 600, 900)
            recs = net.ctx.detect(device_ptr=ptr, shape=shape)
            paths = [os.path.join(tmp, "k_%d.jpg" % i) for i in range(args.batch)]
            for _ in range(5):
                for form in forms:
                    net.ctx.write_annotated_files(ptr, shape, recs, 1.0, paths, entropy=form)
            out["kernels_only_calls"] = 5
            out["kernels_only_forms"] = list(forms)
        else:
            modes = [("no_images", dict(write_images=False)), ("encode_host", dict(write_images=True, encode="host"))]
            if "host" in forms:
                modes.append(("encode_gpu", dict(write_images=True, encode="gpu")))
            if "device" in forms:
                modes.append(("encode_gpu_entropy", dict(write_images=True, encode="gpu-entropy")))
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
            lib_modes = [k for k, _ in modes[2:]]
            same = all(open(os.path.join(tmp, "out_encode_host", os.path.basename(nm)), "rb").read() ==
                       open(os.path.join(tmp, "out_" + k, os.path.basename(nm)), "rb").read() for nm in names for k in lib_modes)
            out["files_identical"] = bool(same)
            out["mean_output_kb"] = round(float(np.mean([os.path.getsize(os.path.join(tmp, "out_" + lib_modes[0], os.path.basename(nm))) for nm in names])) / 1024, 1)
            for k in lib_modes:
                out[k + "_vs_host"] = round(out[k + "_images_per_s"] / out["encode_host_images_per_s"], 2)
            # the writer alone: one live batch, its lines, written again and again -- the forms interleaved call by call
            ptr, shape = net.ctx.decode_jpeg_files(names[: args.batch], 600, 900)
            recs = net.ctx.detect(device_ptr=ptr, shape=shape)
            paths = {f: [os.path.join(tmp, "w_%s_%d.jpg" % (f, i)) for i in range(args.batch)] for f in forms}
            wall, cpu, d2h = {f: [] for f in forms}, {f: 0.0 for f in forms}, {}
            for f in forms:      # warm-up: buffers grown
                for _ in range(2):
                    net.ctx.write_annotated_files(ptr, shape, recs, 1.0, paths[f], entropy=f)
            for _ in range(args.rounds):
                for f in forms:
                    c0, t0 = time.process_time(), time.perf_counter()
                    net.ctx.write_annotated_files(ptr, shape, recs, 1.0, paths[f], entropy=f)
                    wall[f].append(time.perf_counter() - t0)
                    cpu[f] += time.process_time() - c0
                    if f == "device":
                        d2h[f] = net.ctx.jpeg_encode_device_stats()["d2h_bytes"] / args.batch
                    else:
                        d2h[f] = float(6 * ((shape[1] + 15) // 16) * ((shape[2] + 15) // 16) * 64 * 2)      # every coefficient, int16
            for f in forms:
                key = "writer_only_" + f
                out[key + "_images_per_s"] = round(args.batch / float(np.median(wall[f])), 1)
                out[key + "_rounds_images_per_s"] = [round(args.batch / t, 1) for t in wall[f]]
                out[key + "_host_cpu_s_per_1000_images"] = round(1000.0 * cpu[f] / (args.rounds * args.batch), 3)
                out[key + "_d2h_bytes_per_image"] = round(d2h[f], 1)
            if len(forms) == 2:
                out["writer_only_files_identical"] = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(paths["host"], paths["device"]))
                out["writer_only_device_vs_host"] = round(out["writer_only_device_images_per_s"] / out["writer_only_host_images_per_s"], 2)
            if "host" in forms:
                out["write_annotated_files_only_images_per_s"] = out["writer_only_host_images_per_s"]
        net.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    txt = json.dumps(out)
    print(txt)
    if args.out:
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
