#!/usr/bin/env python
"""Files in, results AND text-line crops out: ctpn/demo_batch.py --decode gpu --crops DIR over one folder of JPEG files with the three
forms of --crops-encode -- host (the crops are fetched and written one at a time by Pillow), gpu (ctpn_write_line_crops: cut, JPEG-coded
and written by the library, Huffman coding on its C++ pool) and gpu-entropy (ctpn_write_line_crops_device: the Huffman coding on the
device too) -- in ONE process on one box, next to the HBM-resident rate of the same ctx. The baseline is the host form: the only form
before ctpn_write_line_crops existed. No torch in this process (CTPN_NO_TORCH=1).

    CTPN_NO_TORCH=1 python tools/crops_throughput.py --images 512 --distinct 64 --out profiles/crops_throughput.json
"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FORMS = ("host", "gpu", "gpu-entropy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--crop-height", type=int, default=32)
    ap.add_argument("--threads", type=int, default=0, help="decode threads (0: the rank's host thread budget)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "split", "fp32"])
    args = ap.parse_args()
    from PIL import Image
    import ctpn_amd  # noqa: F401
    from ctpn_amd import _binding as B
    from ctpn_amd.ctpn import demo as D, demo_batch as DB
    from ctpn_amd.lib.networks.factory import get_network
    from ctpn_amd.lib.fast_rcnn.config import cfg_from_file
    from decode_throughput import make_image
    tmp = tempfile.mkdtemp(prefix="ctpn_crops_")
    threads = args.threads or B.host_thread_budget(os.cpu_count() or 1, 1, 0)
    out = {"images": args.images, "distinct_images": args.distinct, "height": 600, "width": 900, "batch": args.batch, "crop_height": args.crop_height,
           "host_cpus": os.cpu_count(), "decode_threads": threads, "precision": args.precision}
    try:
        d = os.path.join(tmp, "jpg")
        os.makedirs(d)
        for i in range(args.images):
            p = os.path.join(d, "img_%04d.jpg" % i)
            if i < args.distinct:
                Image.fromarray(make_image(i)[:, :, ::-1].copy()).save(p, "JPEG", quality=90)
            else:
                shutil.copyfile(os.path.join(d, "img_%04d.jpg" % (i % args.distinct)), p)
        names = DB.list_images(d)
        cfg_from_file(os.path.join(ROOT, "text-detection-ctpn_amd", "ctpn", "text.yml"))
        from ctpn_amd.lib.fast_rcnn.config import cfg
        cfg.TEST.PRECISION = args.precision
        net = get_network("VGGnet_test")
        D.load_weights(net, 0)
        od = os.path.join(tmp, "out")

        def run(form, subset, crops_dir):
            kw = {} if form is None else {"crops_dir": crops_dir, "crop_h": args.crop_height, "crops_encode": form}
            return DB.run(net, subset, od, batch=args.batch, write_images=False, log=lambda *a: None, decode="gpu", decode_threads=threads, **kw)
        run(None, names[: args.batch * 2], None)                      # warm: buffers, kernels
        rates = []
        for _ in range(args.runs):
            t0 = time.time()
            res = run(None, names, None)
            rates.append(round(len(names) / (time.time() - t0), 1))
        out["no_crops_images_per_s"], out["no_crops_runs"] = max(rates), rates
        crops = sum(len(res[nm]) for nm in names)
        out["crops"], out["crops_per_image"] = crops, round(crops / len(names), 2)
        listing, rates = {}, {form: [] for form in FORMS}
        dirs = {form: os.path.join(tmp, "crops-" + form) for form in FORMS}
        for form in FORMS:                                             # warm every form's buffers
            run(form, names[: args.batch * 2], dirs[form])
        for _ in range(args.runs):                                     # the forms alternate inside every round: they share the box's moods
            for form in FORMS:
                shutil.rmtree(dirs[form], ignore_errors=True)
                t0 = time.time()
                run(form, names, dirs[form])
                rates[form].append(round(len(names) / (time.time() - t0), 1))
        for form in FORMS:
            key, cd = form.replace("-", "_"), dirs[form]
            out[key + "_images_per_s"], out[key + "_runs"] = max(rates[form]), rates[form]
            out[key + "_median_images_per_s"] = sorted(rates[form])[len(rates[form]) // 2]
            out[key + "_crops_per_s"] = round(max(rates[form]) * crops / len(names), 1)
            listing[form] = {f: os.path.getsize(os.path.join(cd, f)) for f in sorted(os.listdir(cd))}
            if form != "host":                                         # same names, same sizes; the bytes file by file on the first 64
                same = listing[form] == listing["host"]
                for f in sorted(listing["host"])[:64]:
                    same = same and open(os.path.join(cd, f), "rb").read() == open(os.path.join(dirs["host"], f), "rb").read()
                out[key + "_files_equal_host"] = bool(same)
        out["crop_files"] = len(listing["host"])
        out["mean_crop_file_bytes"] = round(sum(listing["host"].values()) / max(len(listing["host"]), 1), 1)
        # the resident rate: a batch the decoder leaves in device memory, bench.py's loop
        ctx = net.ctx
        datas = []
        for i in range(args.batch):
            buf = io.BytesIO()
            Image.fromarray(make_image(i)[:, :, ::-1].copy()).save(buf, "JPEG", quality=90)
            datas.append(buf.getvalue())
        ptr, shape = ctx.decode_jpeg_batch(datas, 600, 900)

        def loop(steps):
            for k in range(steps):
                ctx.detect_submit(device_ptr=ptr, shape=shape, slot=k & 1)
                if k:
                    ctx.detect_collect((k - 1) & 1)
            ctx.detect_collect((steps - 1) & 1)
        loop(3)
        t0 = time.time()
        loop(30)
        out["resident_images_per_s"] = round(args.batch * 30 / (time.time() - t0), 1)
        for form in FORMS:
            key = form.replace("-", "_")
            out[key + "_vs_resident"] = round(out[key + "_images_per_s"] / out["resident_images_per_s"], 3)
        out["gpu_vs_host"] = round(out["gpu_images_per_s"] / out["host_images_per_s"], 3)
        out["gpu_entropy_vs_host"] = round(out["gpu_entropy_images_per_s"] / out["host_images_per_s"], 3)
        out["gpu_vs_host_medians"] = round(out["gpu_median_images_per_s"] / out["host_median_images_per_s"], 3)
        out["gpu_entropy_vs_host_medians"] = round(out["gpu_entropy_median_images_per_s"] / out["host_median_images_per_s"], 3)
        out["baseline"] = "host: the crops fetched to the host and written one at a time through Pillow -- the only form before ctpn_write_line_crops"
        net.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
