"""Batch form of ctpn/demo.py: a directory of images in, `res_<stem>.txt` (+ annotated images) out,
with the same per-image arithmetic as demo.ctpn() (reference ctpn/demo.py:55-68) but

  * image sizes come from the file headers, so the batches (grouped by the size after resize_im) are known before a pixel
    is decoded; decode (Pillow, releases the GIL) + resize_im on the GPU (ctpn_resize) of batch k+1 run on a host thread
    pool while batch k is on the GPU (the reference decodes with cv2.imread on the one Python thread, demo.py:59),
  * with --decode gpu the JPEG files are decoded and resized on the device (ctpn_decode_jpeg_batch: entropy decoding on the library's host
    pool, everything after it as HIP kernels), batches grouped by file size; other formats keep the host decoder,
  * batches go through ctpn_detect_submit / ctpn_detect_collect (the reference asserts batch == 1,
    lib/rpn_msr/proposal_layer_tf.py:51), software-pipelined over the ctx's two slots; the ctx is sized ONCE for the largest
    batch / shape of the run (growing it mid-run would destroy the slot that still holds an uncollected batch).

  * with --ragged images of one resized width and different heights share batches (ctpn_detect_submit_ragged); together with --decode gpu /
    gpu-entropy the JPEG files are grouped by their RESIZED shapes, whatever their file sizes, layouts and orientations, and decoded into
    the batch's canvas on the device (ctpn_decode_jpeg_files_ragged). Same result files.

  * with --crops DIR every detected line is also cut out as a rectified image of fixed height, `<stem>_<k>.jpg`, for a recogniser behind
    the detector (ctpn_crop_lines: on the device; batches decoded there are cropped where they lie, without fetching them).
    --crops-encode gpu | gpu-entropy: the crops are JPEG-coded and written by the library where they are cut (ctpn_write_line_crops),
    the same files as Pillow's (the default, host).

  * with --ragged --ragged-outputs (and --decode gpu / gpu-entropy) the library's writers take the ragged batches too: --encode gpu /
    gpu-entropy writes their annotated images from the canvas on the device, every image at its own size
    (ctpn_write_annotated_files_ragged; the canvas is not fetched), and --crops cuts their lines from the canvas
    (ctpn_crop_lines_ragged, ctpn_write_line_crops_ragged). Same names, same bytes as without --ragged.

  * with --crops-format png the crops are lossless `<stem>_<k>.png` files (--crops-encode gpu: ctpn_write_line_crops_png[_ragged]), and
    with --ragged-png (next to --ragged --ragged-outputs --png-encode gpu) the PNG files of the run share ragged batches too and are
    written from their canvases (ctpn_write_annotated_png_files_ragged). Same names, same decoded pixels.

  * with --ragged-pack gpu (next to --ragged and --decode gpu / gpu-entropy) the PNG files the library takes share ragged batches whose
    canvases are built on the device: decoded by the library's pool into page-locked memory, resized into the canvas by one kernel
    (ctpn_decode_png_files_ragged). Same result files; the default, host, is the run without the switch.

  * cfg.TEST.RPN_* of the loaded text.yml go into the ctx's tail parameters (ctpn_set_param), so the batched path honours the file like
    the single-image path; --connector NAME=VALUE (repeatable; TextLineCfg's names, MIN_LINE_WIDTH for TEXT_PROPOSALS_WIDTH *
    MIN_NUM_PROPOSALS) sets the connector's thresholds for the batches and for the images that take the single-image path.

    python -m ctpn_amd.ctpn.demo_batch --input data/demo --out data/results --batch 32 [--mode O] [--synthetic 0] [--no-images]
        [--connector LINE_MIN_SCORE=0.8 --connector MAX_HORIZONTAL_GAP=70]
"""
from __future__ import print_function

import argparse
import glob
import os
import sys
import time

import numpy as np

_PKG_PARENT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG_PARENT not in sys.path:
    sys.path.insert(0, _PKG_PARENT)

import ctpn_amd  # noqa: E402,F401
from ctpn_amd.ctpn import demo as D  # noqa: E402
from ctpn_amd import _binding as B  # noqa: E402
from ctpn_amd.lib.networks.factory import get_network  # noqa: E402
from ctpn_amd.lib.fast_rcnn.config import cfg, cfg_from_file  # noqa: E402
from ctpn_amd.lib.fast_rcnn.test import _scale_for  # noqa: E402
from ctpn_amd.lib.utils import image as imutil  # noqa: E402
from ctpn_amd.lib.utils.blob import im_list_to_canvas  # noqa: E402
from ctpn_amd.lib.text_connector.text_connect_cfg import Config as TextLineCfg  # noqa: E402


def list_images(path):
    if os.path.isdir(path):
        names = []
        for ext in ("*.png", "*.jpg", "*.jpeg", "*.bmp"):
            names += glob.glob(os.path.join(path, ext))
        return sorted(names)
    return sorted(glob.glob(path))


def image_size(path):
    """(h, w) of imread(path) from the file header only (no pixel decode; a JPEG's EXIF orientation taken into account like cv2.imread)."""
    return imutil.image_size(path)


def plan(names, batch):
    """-> (jobs, singles, shapes): jobs = [(resized (h, w), [names])] batched by the shape after resize_im; singles = images whose
    second rescale (TEST.SCALES / MAX_SIZE, test.py:17-24) is not the identity (they take the single-image blob path)."""
    from ctpn_amd._binding import resize_dims
    groups, singles, shapes = {}, [], {}
    for name in names:
        h, w = image_size(name)
        f = D.resize_factor((h, w), TextLineCfg.SCALE, TextLineCfg.MAX_SCALE)
        rs = (h, w) if f == 1.0 else resize_dims(h, w, f, f)
        shapes[name] = rs
        s2 = _scale_for(rs)
        if int(round(rs[0] * s2)) == rs[0] and int(round(rs[1] * s2)) == rs[1]:
            groups.setdefault(rs, []).append(name)
        else:
            singles.append(name)
    jobs = []
    for shape, members in sorted(groups.items()):
        for i in range(0, len(members), batch):
            jobs.append((shape, members[i:i + batch]))
    return jobs, singles, shapes


RAGGED_WASTE = 0.25      # plan_ragged_batches' default: see there


def plan_ragged_batches(shapes, max_batch, waste=RAGGED_WASTE):
    """Ragged batches (Context.detect_submit(..., heights=): images of one width and different heights in one call) for images of the
    given (h, w) shapes. -> (batches, alone): batches = [((hc, w), [indices into shapes])] with at least two members each, alone = the
    indices that ended without company (they go through the uniform path). A pure function.
    Per width: the images sorted by height, tallest first; the tallest remaining one opens a batch and sets its canvas height hc; the
    next joins while the batch is below max_batch and the padded rows, sum(hc - h_i), stay within waste * n * hc. Equal heights therefore
    form the plain batches they always did, whatever waste is.
    waste: a padded row costs about what a valid one does (the masks only clear it), and a lone 600 x 900 bf16 image costs about 2.4 x a
    batched one (README), so padding pays up to roughly 1 - 1 / 2.4 = 0.58 of a batch; 0.25 keeps well inside that and still joins the
    usual portrait pages at width 600 (letter 776, 3:4 800, A4 849, 9:16 1067 rows: one of each pads 18 % of the batch). It is a first
    value: tools/ragged_throughput.py measures the three forms it decides between."""
    if max_batch < 1 or not 0.0 <= waste < 1.0:
        raise ValueError("plan_ragged_batches: max_batch >= 1 and 0 <= waste < 1 required")
    by_w = {}
    for i, (h, w) in enumerate(shapes):
        by_w.setdefault(int(w), []).append((int(h), i))
    batches, alone = [], []
    for w in sorted(by_w):
        rest = sorted(by_w[w], key=lambda t: (-t[0], t[1]))
        while rest:
            hc, members, rows = rest[0][0], [rest[0][1]], rest[0][0]
            k = 1
            while k < len(rest) and len(members) < max_batch and (len(members) + 1) * hc - (rows + rest[k][0]) <= waste * (len(members) + 1) * hc:
                members.append(rest[k][1])
                rows += rest[k][0]
                k += 1
            rest = rest[k:]
            if len(members) > 1:
                batches.append(((hc, w), members))
            else:
                alone.append(members[0])
    return batches, alone


PNG_LAYOUT, OTHER_LAYOUT = (-1, 0), (0, 0)      # plan_device_jobs: layouts of the files the JPEG decoder does not take


def plan_device_jobs(entries, batch, ragged=False, waste=RAGGED_WASTE, ragged_png=False, ragged_pack="host"):
    """The batches of the device path (_run_gpu). entries: [(name, file (h, w), layout, resize_im factor, resized (h, w))] of the images that
    take the batched path; layout = (components, sampling | orientation) of a JPEG file the library takes, PNG_LAYOUT, or OTHER_LAYOUT
    (Pillow). -> jobs = [(size, kind, f, rs, names)]. A pure function.
    kind 'jpg' / 'png' / 'host': files of one FILE size (and, for JPEG, one layout and orientation), size = that (h, w), f = their factor,
    rs = their resized shape -- one decode call each takes.
    ragged: the JPEG files the library takes are planned with plan_ragged_batches on their RESIZED shapes first, whatever their file size,
    layout and orientation: kind 'ragged', size = rs = the canvas (hc, wc), f = [(file h, file w, factor)] per name
    (Context.decode_jpeg_ragged). What ends alone there, and every PNG and Pillow file, is size-grouped as without it.
    ragged_png: the PNG files are planned the same way into jobs of a kind of their own, 'ragged-png' (size, f, rs as for 'ragged'): their
    canvas is built on the host (PNG files are decoded there) and written by ctpn_write_annotated_png_files_ragged.
    ragged_pack='gpu' (with ragged): the PNG files are planned that way whether ragged_png is given or not, into jobs of kind
    'ragged-png-gpu' (size, f, rs as for 'ragged'): their canvas is built on the device (Context.decode_png_ragged). 'host' (default): the
    jobs are what they are without the argument."""
    entries = list(entries)
    jobs = []
    pack_gpu = ragged and ragged_pack == "gpu"
    if ragged_png or pack_gpu:
        pngs = [e for e in entries if tuple(e[2]) == PNG_LAYOUT and e[4][0] >= 16]
        batches, _ = plan_ragged_batches([e[4] for e in pngs], batch, waste)
        for (hc, wc), members in batches:
            jobs.append(((hc, wc), "ragged-png-gpu" if pack_gpu else "ragged-png", [(pngs[i][1][0], pngs[i][1][1], pngs[i][3]) for i in members], (hc, wc), [pngs[i][0] for i in members]))
        batched = {pngs[i][0] for _, members in batches for i in members}
        entries = [e for e in entries if e[0] not in batched]
    if ragged:
        jpegs = [e for e in entries if e[2][0] > 0 and e[4][0] >= 16]      # (a ragged image has at least one feature row)
        batches, _ = plan_ragged_batches([e[4] for e in jpegs], batch, waste)
        for (hc, wc), members in batches:
            jobs.append(((hc, wc), "ragged", [(jpegs[i][1][0], jpegs[i][1][1], jpegs[i][3]) for i in members], (hc, wc), [jpegs[i][0] for i in members]))
        batched = {jpegs[i][0] for _, members in batches for i in members}
        entries = [e for e in entries if e[0] not in batched]
    groups = {}
    for name, (h, w), layout, f, rs in entries:
        groups.setdefault((h, w, tuple(layout)), (f, rs, []))[2].append(name)
    for (h, w, layout), (f, rs, members) in sorted(groups.items()):
        for i in range(0, len(members), batch):
            jobs.append(((h, w), "jpg" if layout[0] > 0 else ("png" if layout == PNG_LAYOUT else "host"), f, rs, members[i:i + batch]))
    return jobs


def check_ragged_options(decode="host", encode="host", png_encode="host", crops_dir=None, decode_procs=0, decode_pool=None, ragged_outputs=False, ragged=True,
                         ragged_png=False, ragged_pack="host"):
    """run(..., ragged=True) with these options: ValueError for the combinations that stay uniform. The process-pool decoder fills
    shared-memory batches of one shape; the library's writers (encode / png_encode = 'gpu') and the crops take uniform device batches.
    ragged_outputs: the JPEG writer and the crops take the ragged batches of the device path as well (ctpn_write_annotated_files_ragged,
    ctpn_crop_lines_ragged, ctpn_write_line_crops_ragged) -- it needs ragged and decode='gpu' / 'gpu-entropy'; encode and crops_dir then
    pass, png_encode='gpu' stays refused unless ragged_png is given.
    ragged_png: the PNG files share ragged batches too and the PNG writer takes their canvases (ctpn_write_annotated_png_files_ragged) --
    it needs ragged, ragged_outputs and png_encode='gpu'; png_encode='gpu' then passes.
    ragged_pack: 'gpu' -- the canvases of the ragged PNG batches are built on the device (ctpn_decode_png_files_ragged); it needs ragged and
    decode='gpu' / 'gpu-entropy' and is tied to no output option: what takes a device canvas takes these. 'host' (default): no change."""
    if ragged_pack not in ("host", "gpu"):
        raise ValueError("ragged_pack must be 'host' or 'gpu'")
    if ragged_pack == "gpu" and not (ragged and decode in ("gpu", "gpu-entropy")):
        raise ValueError("ragged_pack='gpu' builds the canvases of ragged PNG batches on the device: it needs ragged=True and decode='gpu' or 'gpu-entropy'")
    if ragged_png and not (ragged and ragged_outputs and png_encode == "gpu"):
        raise ValueError("ragged_png writes the PNG files of ragged batches on the device: it needs ragged=True, ragged_outputs=True and png_encode='gpu'")
    if ragged_outputs and not ragged:
        raise ValueError("ragged_outputs writes the outputs of ragged batches: it needs ragged=True")
    if ragged_outputs and decode not in ("gpu", "gpu-entropy"):
        raise ValueError("ragged_outputs writes the outputs of ragged device batches: it needs decode='gpu' or 'gpu-entropy'")
    if decode_procs > 0 or decode_pool is not None:
        raise ValueError("ragged batches are built by the thread-pool decoder (decode='host') or on the device (decode='gpu' / 'gpu-entropy'): "
                         "the process-pool decoder stays size-grouped")
    if decode in ("gpu", "gpu-entropy"):
        if encode != "host" and not ragged_outputs:
            raise ValueError("ragged device decode does not combine with encode='gpu' / 'gpu-entropy': ctpn_write_annotated_files takes uniform batches")
        if png_encode != "host" and not ragged_png:
            raise ValueError("ragged device decode does not combine with png_encode='gpu': ctpn_write_annotated_png_files takes uniform batches")
        if crops_dir is not None and not ragged_outputs:
            raise ValueError("ragged device decode does not combine with crops_dir: ctpn_crop_lines takes uniform batches")


RPN_PARAM_NAMES = ("RPN_PRE_NMS_TOP_N", "RPN_POST_NMS_TOP_N", "RPN_NMS_THRESH", "RPN_MIN_SIZE")


def _check_uint8_feed_config(params=None):
    """The batched path feeds uint8 images; the library subtracts the reference's PIXEL_MEANS (lib/fast_rcnn/config.py:200) inside its first
    kernel (csrc/conv_first.hip, csrc/conv_first_q.hip), compiled in. The reference subtracts cfg.PIXEL_MEANS at run time (lib/fast_rcnn/test.py:7-11), so an edited
    value must not be ignored silently: it is an error here (the single-image path, lib/fast_rcnn/test.py, subtracts cfg.PIXEL_MEANS in
    Python and takes any value)."""
    built = np.array([102.9801, 115.9465, 122.7717])
    if not np.allclose(np.asarray(cfg.PIXEL_MEANS, np.float64).reshape(-1), built, rtol=0, atol=1e-6):
        raise ValueError("cfg.PIXEL_MEANS = %s, but the uint8 batch feed of libctpn_hip.so subtracts %s in its first kernel; use ctpn/demo.py's "
                         "float-blob path for other means" % (np.asarray(cfg.PIXEL_MEANS).reshape(-1).tolist(), built.tolist()))
    # ctpn_detect / ctpn_detect_submit run the proposal layer with the ctx's parameters (ctpn_set_param; defaults: the reference's TEST values
    # 12000, 1000, 0.7, 8), which run() sets from `params` -- ctpn_proposals, the single-image seam, takes cfg.TEST.RPN_* as arguments
    # (lib/fast_rcnn/test.py). The two paths of one run must agree: a cfg.TEST edit that `params` does not carry would reach only one of them
    t = cfg.TEST
    got = (int(t.RPN_PRE_NMS_TOP_N), int(t.RPN_POST_NMS_TOP_N), float(t.RPN_NMS_THRESH), float(t.RPN_MIN_SIZE))
    used = tuple(ty((params or {}).get(n, B.param_default(n))) for n, ty in zip(RPN_PARAM_NAMES, (int, int, float, float)))
    if got != used:
        raise ValueError("cfg.TEST.RPN_PRE_NMS_TOP_N / RPN_POST_NMS_TOP_N / RPN_NMS_THRESH / RPN_MIN_SIZE = %r, but the batched path "
                         "(ctpn_detect) runs the proposal layer with %r; pass the values as run(..., params=rpn_params_from_cfg()) as main() does, "
                         "or use ctpn/demo.py's single-image path, which reads cfg.TEST" % (got, used))


def rpn_params_from_cfg():
    """cfg.TEST.RPN_* (the loaded text.yml) as tail parameters of the batched path"""
    t = cfg.TEST
    return {"RPN_PRE_NMS_TOP_N": int(t.RPN_PRE_NMS_TOP_N), "RPN_POST_NMS_TOP_N": int(t.RPN_POST_NMS_TOP_N), "RPN_NMS_THRESH": float(t.RPN_NMS_THRESH),
            "RPN_MIN_SIZE": float(t.RPN_MIN_SIZE)}


def parse_connector_args(items):
    """['NAME=VALUE', ...] (--connector) -> {name: float}; names are the connector's parameters (B.CONNECTOR_PARAM_NAMES)"""
    out = {}
    for it in items or []:
        name, sep, value = it.partition("=")
        if not sep or name not in B.CONNECTOR_PARAM_NAMES:
            raise ValueError("--connector wants NAME=VALUE with NAME one of %s, got %r" % (", ".join(B.CONNECTOR_PARAM_NAMES), it))
        out[name] = float(value)
    return out


def _set_tail_params(net, params):
    """The run's tail parameters into its ctx: `params` over the defaults. Called behind ensure_capacity, which may have replaced the ctx.
    A run without params touches nothing unless an earlier run on this net left parameters behind (then they go back to the defaults)."""
    if params is None and not getattr(net, "_tail_params_set", False):
        return
    # more proposals per image than a fresh ctx holds (1000): raise the ctx's capacity first, and only then (ctpn_reserve_proposals)
    post = int((params or {}).get("RPN_POST_NMS_TOP_N", 0))
    if post > 1000:
        B.reserve_for(net.ctx, post)
    for name in B.param_names():
        net.ctx.set_param(name, (params or {}).get(name, B.param_default(name)))
    net._tail_params_set = params is not None


def _text_detector(params):
    """the single-image path's detector under the connector values of `params` (none: the plain TextDetector())"""
    from ctpn_amd.lib.text_connector.detectors import TextDetector
    conn = {k: v for k, v in (params or {}).items() if k in B.CONNECTOR_PARAM_NAMES}
    return TextDetector(config=conn) if conn else TextDetector()


def _load(name):
    img = imutil.imread(name)
    return D.resize_im(img, scale=TextLineCfg.SCALE, max_scale=TextLineCfg.MAX_SCALE)


def _decode_into(name, shm_name, batch_shape, index):
    """Worker PROCESS: decode `name` (Pillow) straight into slot `index` of the shared uint8 batch buffer if the file already has the
    batch's shape (resize_im's factor is 1: the benchmark's case); otherwise hand the decoded image back for the parent's GPU resize.
    Threads do not scale here -- Pillow's RGB conversion and the BGR copy hold the GIL (measured, profiles/r04_decode_throughput_*.json:
    1830 JPEG/s on 32 threads against 330 on one) -- processes do."""
    rgb = imutil.open_rgb(name)
    if rgb.shape[:2] != tuple(batch_shape[1:3]):
        return np.ascontiguousarray(rgb[:, :, ::-1])
    np.ndarray(batch_shape, np.uint8, buffer=_attach(shm_name).buf)[index] = rgb[:, :, ::-1]
    return None


_SHM = {}


def _attach(shm_name):
    """A worker maps each shared batch buffer ONCE (attaching per task costs an mmap of the whole batch, its page faults and a round trip to
    multiprocessing's resource tracker: measured 1343 -> see profiles/r04_decode_throughput.json)."""
    shm = _SHM.get(shm_name)
    if shm is None:
        from multiprocessing import shared_memory
        if len(_SHM) > 8:
            for old in list(_SHM.values()):
                old.close()
            _SHM.clear()
        shm = _SHM[shm_name] = shared_memory.SharedMemory(name=shm_name)
    return shm


def decode_pool(procs):
    """A pool of `procs` decode worker processes (spawned: the parent holds a HIP context), warmed up so that a timed run does not pay for
    their start-up (~1.5 s for 32 workers). Pass it to run(decode_pool=...); the caller shuts it down."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    pool = ProcessPoolExecutor(max_workers=procs, mp_context=mp.get_context("spawn"))
    list(pool.map(_warm, range(4 * procs)))
    return pool


def _warm(i):
    import PIL.Image  # noqa: F401
    time.sleep(0.02)       # long enough that every worker of the pool takes some
    return i


def _is_jpeg(name):
    return name.lower().endswith((".jpg", ".jpeg"))


def _is_png(name):
    return name.lower().endswith(".png")


def _read(name):
    with open(name, "rb") as f:
        return f.read()


def write_crops(ctx, crops_dir, names, recs, crop_h=32, max_w=512, images=None, device_ptr=None, shape=None, encode="host", heights=None, format="jpg"):
    """The text lines of one batch as rectified crops of height crop_h (ctpn_crop_lines: cut out on the device, from host images or from
    a batch that lies there), each written as <stem>_<k>.jpg -- k counts the image's lines as its res file lists them --, trimmed to its
    width, by the host writer. A line longer than max_w columns at that height is squeezed to max_w. -> number of files
    encode='gpu': the library codes and writes the files where the crops are cut (ctpn_write_line_crops: no crop visits the host or Python);
    'gpu-entropy': the same with the Huffman coding on the device too (ctpn_write_line_crops_device). Same names, same bytes.
    heights: images / device_ptr is a ragged canvas, image i in rows [0, heights[i]) of slot i (the *_ragged calls). Same names, same bytes.
    format='png': <stem>_<k>.png, lossless -- by Pillow (encode='host') or by the library (encode='gpu': ctpn_write_line_crops_png[_ragged]);
    the two writers' files decode to the same pixels. There is no 'gpu-entropy' form of it."""
    if encode not in ("host", "gpu", "gpu-entropy"):
        raise ValueError("encode must be 'host', 'gpu' or 'gpu-entropy'")
    if format not in ("jpg", "png"):
        raise ValueError("format must be 'jpg' or 'png'")
    if format == "png" and encode == "gpu-entropy":
        raise ValueError("format='png' has no encode='gpu-entropy' form: the PNG writer's codes are built on the host")
    if encode != "host":
        paths = [os.path.join(crops_dir, '{}_{}.{}'.format(os.path.basename(nm).split('.')[0], j, format)) for nm, rr in zip(names, recs) for j in range(len(rr))]
        ctx.write_line_crops(images, recs, crop_h=crop_h, max_w=max_w, device_ptr=device_ptr, shape=shape, paths=paths, quality=95,
                             entropy="device" if encode == "gpu-entropy" else "host", heights=heights, format=format)
        return len(paths)
    crops, widths = ctx.crop_lines(images, recs, crop_h=crop_h, max_w=max_w, device_ptr=device_ptr, shape=shape, heights=heights)
    k = 0
    for nm, rr in zip(names, recs):
        stem = os.path.basename(nm).split('.')[0]
        for j in range(len(rr)):
            imutil.imwrite(os.path.join(crops_dir, '{}_{}.{}'.format(stem, j, format)), crops[k, :, :widths[k]])
            k += 1
    return k


def _run_gpu(net, names, out_dir, batch, mode, write_images, log, read_threads=8, encode="host", crops_dir=None, crop_h=32, params=None, entropy="host",
             encode_entropy="host", png_encode="host", ragged=False, ragged_waste=RAGGED_WASTE, crops_encode="host", ragged_outputs=False, crops_format="jpg",
             ragged_png=False, ragged_pack="host"):
    """decode='gpu': the JPEG files of the run are decoded AND resized on the device (ctpn_decode_jpeg_batch: Huffman decoding on the ctx's
    C++ worker pool, IDCT / chroma upsampling / colour conversion / cv2.resize as HIP kernels in the ctx's copy queue, ordered against the
    forward by events) -- neither the file bytes nor the pixels pass through Python, and the pixels never exist on the host unless
    annotated images are asked for. Batches are grouped by FILE size (as cv2.imread returns it: EXIF orientation applied), chroma layout
    and orientation, all read from the headers (one size, one resize factor, one network shape per batch). PNG files are decoded by the library too, on the host by the nature of the format
    (ctpn_decode_png_files: inflate + row filters, one file per C++ thread, straight into the batch buffer that ctpn_detect_submit copies to
    the device). Files neither decoder takes (CMYK / arithmetic-coded / truncated JPEG, 16-bit PNG, other formats) go through Pillow
    (lib/utils/image.py), batched the same way; the result files are the same whichever decoder a file went through.
    encode='gpu' (with write_images): the annotated images of device-decoded batches whose output name is a JPEG's are drawn, resized by
    1 / scale and JPEG-coded by the library at collect time (ctpn_write_annotated_files: kernels in the ctx's copy queue, Huffman coding and
    file writing on its C++ pool) -- those pixels never reach the host. PNG-named outputs (unless png_encode='gpu'),
    batches of the host decoders and the single images keep Pillow's writer; the files are byte-identical either way.
    entropy='device' (--decode gpu-entropy): the Huffman decode of the JPEG batches runs on the device too (ctpn_decode_jpeg_files_device);
    a batch that call refuses -- one with a progressive file in it -- takes the host-entropy call, and what that refuses goes to Pillow, as
    with decode='gpu'.
    encode_entropy='device' (--encode gpu-entropy): encode='gpu' with the Huffman CODING on the device too (ctpn_write_annotated_files_device):
    only the files' own bytes cross to the host. The files are byte-identical.
    png_encode='gpu' (--png-encode gpu, with write_images): the PNG-named outputs of library-decoded batches -- PNG batches, which reach the
    device as host images, and device JPEG batches whose names end in .png -- are drawn, resized by 1 / scale and PNG-coded by the library
    at collect time (ctpn_write_annotated_png_files). "Host work by nature" holds for READING a PNG file (inflate is serial, un-filtering
    chains from row to row); writing one parallelises. The files are the library's own (Sub filter, one dynamic-Huffman block): they decode
    to the pixels Pillow's files decode to, but are not byte-equal to them. Default 'host': Pillow, as before.
    ragged (--ragged): the JPEG files the library takes are batched by their RESIZED shapes -- one width, different heights, whatever their file
    sizes, layouts and orientations (plan_device_jobs) -- decoded into one canvas on the device (ctpn_decode_jpeg_files_ragged) and detected
    from it (ctpn_detect_submit_ragged); annotated images are cut from the fetched canvas for the host writer. What ends alone, PNG batches
    and Pillow's files stay size-grouped. The result files are the same.
    crops_encode (--crops-encode, with crops_dir): 'gpu' / 'gpu-entropy' -- the crops are JPEG-coded and written by the library where they
    are cut (write_crops); 'host' (default): fetched and written by Pillow, as before. Same names, same bytes.
    ragged_outputs (--ragged-outputs, with ragged): encode='gpu' writes the annotated images of ragged batches too, from the canvas where it
    lies, every image resized by its own 1 / scale (ctpn_write_annotated_files_ragged[_device]; the canvas is not fetched), and crops_dir
    cuts their lines from the canvas (ctpn_crop_lines_ragged, ctpn_write_line_crops_ragged[_device]). A ragged batch that fell back to
    the host decoder hands its host canvas to the same calls. Same names, same bytes as without ragged.
    crops_format (--crops-format, with crops_dir): 'png' -- the crops are <stem>_<k>.png files (write_crops).
    ragged_png (--ragged-png, with ragged, ragged_outputs and png_encode='gpu'): the PNG files are batched by their resized shapes as well
    (plan_device_jobs, kind 'ragged-png'); a batch's canvas is built on the host, where PNG files are decoded, submitted with its heights,
    and its annotated images are written from it at collect time (ctpn_write_annotated_png_files_ragged). Same names, same pixels.
    ragged_pack='gpu' (--ragged-pack gpu, with ragged): the PNG files are batched by their resized shapes whether ragged_png is given or not
    (kind 'ragged-png-gpu'), and a batch's canvas is built on the device: the files are decoded by the library's pool into page-locked
    memory and one kernel resizes them into the canvas (ctpn_decode_png_files_ragged). The canvas is detected, written (png_encode='gpu'
    with ragged_png) and cropped (crops_dir with ragged_outputs) where it lies, and fetched for the host writer otherwise. A batch the
    library's PNG decoder does not take falls back to the host canvas. Same result files."""
    from ctpn_amd._binding import resize_dims
    mode = mode or cfg.TEST.DETECT_MODE
    os.makedirs(out_dir, exist_ok=True)
    singles = []
    t_plan = time.time()
    probed = B.jpeg_probe_files(names, read_threads)                          # the header scan: one call, C++ threads
    pngs = [i for i, nm in enumerate(names) if probed[i, 0] == 0 and nm.lower().endswith(".png")]
    png_info = dict(zip(pngs, B.png_probe_files([names[i] for i in pngs], read_threads).tolist())) if pngs else {}
    entries = []
    for i, (name, pr) in enumerate(zip(names, probed.tolist())):
        if pr[0] > 0:
            (h, w), layout = (pr[0], pr[1]), (pr[2], pr[3])
        elif png_info.get(i, [0])[0] > 0:
            (h, w), layout = tuple(png_info[i][:2]), PNG_LAYOUT
        else:
            (h, w), layout = image_size(name), OTHER_LAYOUT
        f = D.resize_factor((h, w), TextLineCfg.SCALE, TextLineCfg.MAX_SCALE)
        rs = (h, w) if f == 1.0 else resize_dims(h, w, f, f)
        s2 = _scale_for(rs)
        if int(round(rs[0] * s2)) == rs[0] and int(round(rs[1] * s2)) == rs[1]:
            entries.append((name, (h, w), layout, f, rs))
        else:
            singles.append(name)
    jobs = plan_device_jobs(entries, batch, ragged, ragged_waste, ragged_png=ragged_png, ragged_pack=ragged_pack)
    if jobs:
        net.ensure_capacity(max(len(j[4]) for j in jobs), max(j[3][0] for j in jobs), max(j[3][1] for j in jobs))
        _set_tail_params(net, params)
    results, meta, stats = {}, {}, {"gpu": 0, "png": 0, "host": 0, "enc_gpu": 0, "enc_png": 0, "enc_host": 0, "crops": 0, "rag_png": 0}
    png_batches = {}                                   # slot -> (device pointer or None, host images or None, shape, scale) of a batch whose PNG files the library writes
    dev_batches = {}                                   # slot -> (device pointer, shape, scale) of a batch whose images the library writes
    crop_src = {}                                      # slot -> what the batch's crops are cut from: device pointer + shape, or host images; heights of a ragged canvas
    rag_png_batches = {}                               # slot -> (device pointer or None, host canvas or None, shape, heights, scales) of a ragged PNG batch whose images the library writes
    rag_batches = {}                                   # slot -> (device pointer or None, host canvas or None, shape, heights, scales) of a ragged batch whose images the library writes
    # PNG batches are decoded ONE JOB AHEAD on a helper thread (the C++ decode threads hang off that call; ctypes releases the GIL), so that
    # batch k + 1 inflates while batch k is submitted and batch k - 1 collected. Three batch buffers per shape in a ring: when batch k + 1
    # starts decoding, batch k sits decoded in its buffer and batch k - 1 may still be on its way to the device. THREE slots whatever the
    # run's shapes: a slot whose shape changes is replaced (a directory of a thousand PNG sizes does not keep a thousand batch buffers).
    from concurrent.futures import ThreadPoolExecutor
    png_bufs, png_ahead, png_pool = {}, {}, ThreadPoolExecutor(max_workers=1)

    def png_decode(k):
        (h, w), _, f, rs, members = jobs[k]
        shape = (len(members), h, w, 3)
        if k % 3 not in png_bufs or png_bufs[k % 3].shape != shape:
            png_bufs[k % 3] = np.empty(shape, np.uint8)
        imgs = B.decode_png_files(members, h, w, read_threads, out=png_bufs[k % 3])      # files read, inflated and unfiltered on C++ threads
        if f != 1.0:
            imgs = B.resize_linear(imgs, f, f)
        assert tuple(imgs.shape[1:3]) == tuple(rs), (imgs.shape, rs)
        return imgs

    def png_prefetch(k):
        if k < len(jobs) and jobs[k][1] == "png" and k not in png_ahead:
            png_ahead[k] = png_pool.submit(png_decode, k)
    t0 = time.time()
    t_plan = t0 - t_plan
    pending = None

    def emit(nm):
        img, scale = meta.pop(nm)
        if write_images and img is not None:
            stats["enc_host"] += 1
            D.draw_boxes(img.copy(), nm, results[nm], scale, out_dir)
        else:
            base = os.path.basename(nm)
            B.write_result_file(os.path.join(out_dir, 'res_{}.txt'.format(base.split('.')[0])), results[nm], scale)

    def collect(job):                                  # ... and its result files are written here, while the next batch is on the GPU
        slot, members = job
        for nm, recs in zip(members, net.ctx.detect_collect(slot, mode=mode, line_capacity=1024)):
            results[nm] = recs
        if slot in dev_batches:                        # draw + resize + JPEG of the whole batch behind the C ABI; emit() writes the text files
            ptr, shape, scale = dev_batches.pop(slot)
            net.ctx.write_annotated_files(ptr, shape, [results[nm] for nm in members], scale,
                                          [os.path.join(out_dir, os.path.basename(nm)) for nm in members], entropy=encode_entropy)
            stats["enc_gpu"] += len(members)
        if slot in png_batches:                        # the same into PNG files (ctpn_write_annotated_png_files)
            ptr, host_imgs, shape, scale = png_batches.pop(slot)
            net.ctx.write_annotated_png_files(images=host_imgs, device_ptr=ptr, shape=shape, recs=[results[nm] for nm in members], scale=scale,
                                              paths=[os.path.join(out_dir, os.path.basename(nm)) for nm in members])
            stats["enc_gpu"] += len(members)
            stats["enc_png"] += len(members)
        if slot in rag_batches:                        # the same for a ragged canvas: every image at its own size (ctpn_write_annotated_files_ragged)
            ptr, host_canvas, shape, hts, scs = rag_batches.pop(slot)
            net.ctx.write_annotated_files_ragged(images=host_canvas, device_ptr=ptr, shape=shape, heights=hts, recs=[results[nm] for nm in members], scales=scs,
                                                 paths=[os.path.join(out_dir, os.path.basename(nm)) for nm in members], entropy=encode_entropy)
            stats["enc_gpu"] += len(members)
        if slot in rag_png_batches:                    # ... and into PNG files (ctpn_write_annotated_png_files_ragged)
            ptr, host_canvas, shape, hts, scs = rag_png_batches.pop(slot)
            net.ctx.write_annotated_png_files_ragged(images=host_canvas, device_ptr=ptr, shape=shape, heights=hts, recs=[results[nm] for nm in members], scales=scs,
                                                     paths=[os.path.join(out_dir, os.path.basename(nm)) for nm in members])
            stats["enc_gpu"] += len(members)
            stats["enc_png"] += len(members)
            stats["rag_png"] += 1
        if slot in crop_src:                           # (a device batch is live until the second-next decode: this is one decode from its own)
            ptr, shape, imgs, hts = crop_src.pop(slot)
            stats["crops"] += write_crops(net.ctx, crops_dir, members, [results[nm] for nm in members], crop_h, images=imgs, device_ptr=ptr, shape=shape,
                                          encode=crops_encode, heights=hts, format=crops_format)
        for nm in members:
            emit(nm)

    png_prefetch(0)
    for k, ((h, w), kind, f, rs, members) in enumerate(jobs):
        png_prefetch(k + 1)
        imgs = None
        scales = [f] * len(members)
        rag_crops = None                               # a ragged batch's crop source (ragged_outputs)
        if kind == "ragged":                           # f: (file h, file w, factor) per member; (h, w) and rs: the canvas
            sizes, scales = [t[:2] for t in f], [t[2] for t in f]
            try:
                handle = None
                if entropy == "device":
                    try:
                        handle = net.ctx.decode_jpeg_ragged(members, sizes, scales, h, w, entropy="device")
                    except B.CtpnError as e:
                        if e.code != B.CTPN_ERR_UNSUPPORTED:                   # (a progressive file in the batch: the host half's)
                            raise
                if handle is None:
                    handle = net.ctx.decode_jpeg_ragged(members, sizes, scales, h, w)
                (ptr, shape), heights = handle
                net.ctx.detect_submit(device_ptr=ptr, shape=shape, heights=heights, slot=k & 1)
                stats["gpu"] += len(members)
                lib_writes = ragged_outputs and write_images and encode == "gpu" and all(_is_jpeg(nm) for nm in members)
                if lib_writes:                         # (live until the second-next decode: collected one decode from now; not fetched)
                    rag_batches[k & 1] = (ptr, None, shape, heights, scales)
                elif write_images:
                    canvas = net.ctx.jpeg_batch_fetch(ptr, shape)
                    imgs = [canvas[i, :heights[i]] for i in range(len(members))]
                rag_crops = (ptr, shape, None, heights)
            except B.CtpnError as e:                                       # e.g. damaged entropy data: the same canvas from the host decoder
                if e.code not in (B.CTPN_ERR_UNSUPPORTED, -1):
                    raise
                rag_batches.pop(k & 1, None)
                imgs = [_load(nm)[0] for nm in members]
                canvas, heights = im_list_to_canvas(imgs)
                net.ctx.detect_submit(images=canvas, heights=heights, slot=k & 1)
                stats["host"] += len(members)
                if ragged_outputs and write_images and encode == "gpu" and all(_is_jpeg(nm) for nm in members):      # the host canvas through the same call
                    rag_batches[k & 1] = (None, canvas, canvas.shape[:3], heights, scales)
                rag_crops = (None, None, canvas, heights)
        if kind == "ragged-png-gpu":                   # the same shape of job over PNG files, the canvas built on the device (ragged_pack='gpu')
            sizes, scales = [t[:2] for t in f], [t[2] for t in f]
            try:
                (ptr, shape), heights = net.ctx.decode_png_ragged(members, sizes, scales, h, w)
                net.ctx.detect_submit(device_ptr=ptr, shape=shape, heights=heights, slot=k & 1)
                stats["png"] += len(members)
                if write_images and png_encode == "gpu":      # (live until the second-next decode or pack: collected one from now; not fetched)
                    rag_png_batches[k & 1] = (ptr, None, shape, heights, scales)
                elif write_images:
                    canvas = net.ctx.jpeg_batch_fetch(ptr, shape)
                    imgs = [canvas[i, :heights[i]] for i in range(len(members))]
                rag_crops = (ptr, shape, None, heights)
            except B.CtpnError as e:                                       # e.g. a 16-bit file: the same canvas from the host decoder
                if e.code not in (B.CTPN_ERR_UNSUPPORTED, -1):
                    raise
                rag_png_batches.pop(k & 1, None)
                kind = "ragged-png"
        if kind == "ragged-png":                       # the same shape of job over PNG files: the canvas is built on the host (ragged_png)
            scales = [t[2] for t in f]
            imgs = [_load(nm)[0] for nm in members]
            canvas, heights = im_list_to_canvas(imgs)
            net.ctx.detect_submit(images=canvas, heights=heights, slot=k & 1)
            stats["host"] += len(members)
            if write_images and png_encode == "gpu":
                rag_png_batches[k & 1] = (None, canvas, canvas.shape[:3], heights, scales)
            rag_crops = (None, None, canvas, heights)
        if kind == "jpg":
            try:
                ptr = None
                if entropy == "device":
                    try:
                        ptr, shape = net.ctx.decode_jpeg_files(members, h, w, f, f, entropy="device")      # Huffman decode on the device too
                    except B.CtpnError as e:
                        if e.code != B.CTPN_ERR_UNSUPPORTED:                   # (a progressive file in the batch: the host half's)
                            raise
                if ptr is None:
                    ptr, shape = net.ctx.decode_jpeg_files(members, h, w, f, f)      # files read + entropy-decoded on the library's pool
                assert tuple(shape[1:]) == tuple(rs), (shape, rs)
                net.ctx.detect_submit(device_ptr=ptr, shape=shape, slot=k & 1)
                stats["gpu"] += len(members)
                if write_images and encode == "gpu" and all(_is_jpeg(nm) for nm in members):      # (the output's format follows its NAME)
                    dev_batches[k & 1] = (ptr, shape, f)      # (live until the second-next decode: collected one decode from now)
                elif write_images and png_encode == "gpu" and all(_is_png(nm) for nm in members):
                    png_batches[k & 1] = (ptr, None, shape, f)
                elif write_images:
                    imgs = net.ctx.jpeg_batch_fetch(ptr, shape)
            except B.CtpnError as e:                                       # e.g. damaged entropy data: the host decoder's call
                if e.code not in (B.CTPN_ERR_UNSUPPORTED, -1):
                    raise
                kind = "host"
                dev_batches.pop(k & 1, None)
                png_batches.pop(k & 1, None)
        elif kind == "png":
            try:
                imgs = png_ahead.pop(k).result()
                net.ctx.detect_submit(images=imgs, slot=k & 1)
                stats["png"] += len(members)
                if write_images and png_encode == "gpu" and all(_is_png(nm) for nm in members):
                    png_batches[k & 1] = (None, imgs, imgs.shape, f)      # (its ring buffer is not rewritten before the second-next decode)
            except B.CtpnError as e:
                if e.code not in (B.CTPN_ERR_UNSUPPORTED, -1):
                    raise
                kind = "host"
        if kind == "host":
            imgs = np.stack([_load(nm)[0] for nm in members])
            net.ctx.detect_submit(images=imgs, slot=k & 1)
            stats["host"] += len(members)
        for i, nm in enumerate(members):
            meta[nm] = (imgs[i] if imgs is not None and write_images and (k & 1) not in png_batches and (k & 1) not in rag_batches and (k & 1) not in rag_png_batches else None,
                        scales[i])
        if pending is not None:
            collect(pending)
        if crops_dir:
            crop_src[k & 1] = rag_crops if rag_crops is not None else ((ptr, shape, None, None) if kind == "jpg" else (None, None, imgs, None))
        pending = (k & 1, members)
    if pending is not None:
        collect(pending)
    png_pool.shutdown()
    for nm in singles:
        img, scale = _load(nm)
        from ctpn_amd.lib.fast_rcnn.test import test_ctpn
        scores, boxes = test_ctpn(None, net, img)
        results[nm] = _text_detector(params).detect(boxes, scores[:, np.newaxis], img.shape[:2])
        meta[nm] = (img, scale)
        if crops_dir:
            stats["crops"] += write_crops(net.ctx, crops_dir, [nm], [results[nm]], crop_h, images=img[None], encode=crops_encode, format=crops_format)
        emit(nm)
    dt = time.time() - t0
    log('Detection of {:d} images in {:d} batches took {:.3f}s, result files included, after a header scan of {:.3f}s ({:.1f} images/s; {:d} decoded on the device, {:d} PNG files by the library, {:d} on the host)'.format(
        len(names), len(jobs) + len(singles), dt, t_plan, len(names) / max(dt, 1e-9), stats["gpu"], stats["png"], stats["host"] + len(singles)))
    if write_images:
        log('Annotated images: {:d} drawn, resized and JPEG-coded by the library (device + C++ pool), {:d} by the host writer (Pillow)'.format(
            stats["enc_gpu"], stats["enc_host"]))
        if stats["enc_png"]:
            log('... of the library\'s, {:d} are PNG files, coded on the device'.format(stats["enc_png"]))
        if stats["rag_png"]:
            log('... written from {:d} ragged PNG batches (ctpn_write_annotated_png_files_ragged)'.format(stats["rag_png"]))
    if crops_dir:
        log('Text-line crops: {:d} of height {:d} cut out on the device, written by {}'.format(
            stats["crops"], crop_h, "the host writer (Pillow)" if crops_encode == "host" else "the library (device + C++ pool)"))
    return results


def run(net, names, out_dir, batch=32, mode=None, write_images=True, log=print, decode_threads=8, decode_procs=0, decode_pool=None, decode="host",
        encode="host", crops_dir=None, crop_h=32, params=None, png_encode="host", ragged=False, ragged_waste=RAGGED_WASTE, crops_encode="host", ragged_outputs=False,
        crops_format="jpg", ragged_png=False, ragged_pack="host"):
    """-> {image name: (M,9) records}. decode_procs > 0 (or a warm decode_pool): decode in worker processes writing into shared-memory batch
    buffers (one batch ahead of the GPU) instead of on the thread pool. decode='gpu': JPEG decode + resize_im on the device (_run_gpu).
    encode='gpu' (needs decode='gpu'): the annotated JPEG images of device-decoded batches are written by the library
    (ctpn_write_annotated_files); 'gpu-entropy': the same with the Huffman coding on the device too (ctpn_write_annotated_files_device,
    byte-identical files); 'host' (default): every image through Pillow, as before.
    png_encode='gpu' (needs decode='gpu'): the PNG-named outputs of library-decoded batches are written by the library too
    (ctpn_write_annotated_png_files: PNG coding on the device); 'host' (default): Pillow, as before.
    crops_dir (needs decode='gpu'): every detected line also as a rectified crop of height crop_h, <stem>_<k>.jpg in that directory, cut out
    on the device at collect time (write_crops); None (default): nothing changes.
    crops_encode (needs crops_dir and decode='gpu'): 'gpu' -- the crops are JPEG-coded and written by the library where they are cut
    (ctpn_write_line_crops), 'gpu-entropy' -- with the Huffman coding on the device too; 'host' (default): Pillow, as before. Same files.
    params: {name: value} of the detection tail (ctpn_set_param: RPN_* and the connector's names) for the ctx of this run; the connector's
    also reach the images that take the single-image path. None: the defaults.
    ragged (off by default): images of one resized width and different heights share batches (plan_ragged_batches with ragged_waste;
    Context.detect_submit(..., heights=)) instead of one batch per resized shape. Same result files. decode='host': from resized images
    on the thread pool. decode='gpu' / 'gpu-entropy': the JPEG files the library takes are decoded into ragged canvases on the device
    whatever their file sizes, layouts and orientations (Context.decode_jpeg_ragged; see _run_gpu); PNG batches, Pillow's files and what
    ends alone stay size-grouped. Not with the process-pool decoder, and on the device path not with encode='gpu' / 'gpu-entropy',
    png_encode='gpu' or crops_dir, which take uniform batches (check_ragged_options: ValueError).
    ragged_outputs (off by default; needs ragged and decode='gpu' / 'gpu-entropy', else ValueError before any work): encode='gpu' /
    'gpu-entropy' and crops_dir (with any crops_encode) then combine with ragged -- the library writes the annotated images and the crops
    of ragged batches from their canvases (_run_gpu). png_encode='gpu' stays refused. Same names, same bytes as without ragged.
    crops_format (default 'jpg'): 'png' -- the crops are lossless <stem>_<k>.png files, by Pillow (crops_encode='host') or by the library
    (crops_encode='gpu': ctpn_write_line_crops_png, and ..._png_ragged for ragged batches); with crops_encode='gpu-entropy': ValueError.
    ragged_png (off by default; needs ragged, ragged_outputs and png_encode='gpu', else ValueError before any work): png_encode='gpu' then
    combines with ragged -- the PNG files share ragged batches and the library writes their annotated images from the canvases
    (ctpn_write_annotated_png_files_ragged). Same names, same decoded pixels as without it.
    ragged_pack ('host' by default: nothing changes; 'gpu' needs ragged and decode='gpu' / 'gpu-entropy', else ValueError before any work): the
    PNG files the library takes share ragged batches whose canvases are built on the device (Context.decode_png_ragged; see _run_gpu),
    with any output option that takes a device canvas. Same result files. Measured on a folder of PNG files of 16 sizes: 2.5 x the size-grouped
    path, 13.8 x the host canvas (tools/canvas_pack_throughput.py, profiles/canvas_pack_throughput.json)."""
    from concurrent.futures import ThreadPoolExecutor
    _check_uint8_feed_config(params)
    if params:
        parse_connector_args(["%s=%r" % (k, float(v)) for k, v in params.items() if k not in RPN_PARAM_NAMES])      # unknown names: an error before any work
    if encode not in ("host", "gpu", "gpu-entropy"):
        raise ValueError("encode must be 'host', 'gpu' or 'gpu-entropy'")
    encode_entropy = "device" if encode == "gpu-entropy" else "host"      # gpu-entropy: encode='gpu' with the Huffman coding on the device too
    if encode == "gpu-entropy":
        encode = "gpu"
    entropy = "device" if decode == "gpu-entropy" else "host"      # gpu-entropy: decode='gpu' with the Huffman decode on the device too
    if decode == "gpu-entropy":
        decode = "gpu"
    if encode == "gpu" and decode != "gpu":
        raise ValueError("encode='gpu' writes the images of device-decoded batches: it needs decode='gpu'")
    if png_encode not in ("host", "gpu"):
        raise ValueError("png_encode must be 'host' or 'gpu'")
    if png_encode == "gpu" and decode != "gpu":
        raise ValueError("png_encode='gpu' writes the images of library-decoded batches: it needs decode='gpu'")
    if crops_dir is not None and decode != "gpu":
        raise ValueError("crops_dir cuts the lines out of the batches of the device path: it needs decode='gpu'")
    if crops_encode not in ("host", "gpu", "gpu-entropy"):
        raise ValueError("crops_encode must be 'host', 'gpu' or 'gpu-entropy'")
    if crops_encode != "host" and (crops_dir is None or decode != "gpu"):
        raise ValueError("crops_encode='%s' writes the crops of crops_dir on the device: it needs crops_dir and decode='gpu'" % crops_encode)
    if crops_format not in ("jpg", "png"):
        raise ValueError("crops_format must be 'jpg' or 'png'")
    if crops_format == "png" and crops_encode == "gpu-entropy":
        raise ValueError("crops_format='png' has no crops_encode='gpu-entropy' form: the PNG writer's codes are built on the host")
    if ragged or ragged_outputs or ragged_png or ragged_pack != "host":
        check_ragged_options(decode, encode, png_encode, crops_dir, decode_procs, decode_pool, ragged_outputs=ragged_outputs, ragged=ragged, ragged_png=ragged_png,
                             ragged_pack=ragged_pack)
    if decode == "gpu":
        if crops_dir is not None:
            os.makedirs(crops_dir, exist_ok=True)
        return _run_gpu(net, names, out_dir, batch, mode, write_images, log, read_threads=decode_threads, encode=encode, crops_dir=crops_dir, crop_h=crop_h, params=params,
                        entropy=entropy, encode_entropy=encode_entropy, png_encode=png_encode, ragged=ragged, ragged_waste=ragged_waste, crops_encode=crops_encode,
                        ragged_outputs=ragged_outputs, crops_format=crops_format, ragged_png=ragged_png, ragged_pack=ragged_pack)
    if decode_procs > 0 or decode_pool is not None:
        return _run_procs(net, names, out_dir, batch, mode, write_images, log, decode_procs, decode_pool, params=params)
    mode = mode or cfg.TEST.DETECT_MODE
    os.makedirs(out_dir, exist_ok=True)
    jobs, singles, shapes = plan(names, batch)
    if ragged:      # the same images, re-batched across heights; what ends alone stays a uniform batch of one
        pooled = [nm for _, members in jobs for nm in members]
        batches, alone = plan_ragged_batches([shapes[nm] for nm in pooled], batch, ragged_waste)
        jobs = [(shape, [pooled[i] for i in members]) for shape, members in batches] + [(shapes[pooled[i]], [pooled[i]]) for i in alone]
    if jobs:      # one ctx for the whole run: largest batch x largest shape
        net.ensure_capacity(max(len(m) for _, m in jobs), max(s[0] for s, _ in jobs), max(s[1] for s, _ in jobs))
        _set_tail_params(net, params)
    results, meta = {}, {}
    t0 = time.time()
    pending = None

    def collect(job):
        slot, members = job
        lines = net.ctx.detect_collect(slot, mode=mode, line_capacity=1024)
        for nm, recs in zip(members, lines):
            results[nm] = recs

    with ThreadPoolExecutor(max_workers=max(1, decode_threads)) as pool:
        def decode(members):
            return [pool.submit(_load, nm) for nm in members]
        ahead = decode(jobs[0][1]) if jobs else []
        for k, (shape, members) in enumerate(jobs):
            loaded = [f.result() for f in ahead]
            ahead = decode(jobs[k + 1][1]) if k + 1 < len(jobs) else []      # next batch decodes while this one is on the GPU
            for nm, (img, scale) in zip(members, loaded):
                assert img.shape[:2] == tuple(shapes[nm]) and img.shape[0] <= shape[0] and img.shape[1] == shape[1], (nm, img.shape, shape)
                meta[nm] = (img, scale)
            if all(img.shape[0] == shape[0] for img, _ in loaded):
                net.ctx.detect_submit(images=np.stack([img for img, _ in loaded]), slot=k & 1)
            else:
                canvas, heights = im_list_to_canvas([img for img, _ in loaded])
                net.ctx.detect_submit(images=canvas, heights=heights, slot=k & 1)
            if pending is not None:
                collect(pending)
            pending = (k & 1, members)
        if pending is not None:
            collect(pending)
        for nm, fut in zip(singles, [pool.submit(_load, nm) for nm in singles]):
            meta[nm] = fut.result()
    for nm in singles:
        img, scale = meta[nm]
        from ctpn_amd.lib.fast_rcnn.test import test_ctpn
        scores, boxes = test_ctpn(None, net, img)
        results[nm] = _text_detector(params).detect(boxes, scores[:, np.newaxis], img.shape[:2])
    dt = time.time() - t0
    for nm in names:
        img, scale = meta[nm]
        if write_images:
            D.draw_boxes(img.copy(), nm, results[nm], scale, out_dir)
        else:
            base = os.path.basename(nm)
            B.write_result_file(os.path.join(out_dir, 'res_{}.txt'.format(base.split('.')[0])), results[nm], scale)
    log('Detection of {:d} images in {:d} batches took {:.3f}s ({:.1f} images/s)'.format(len(names), len(jobs) + len(singles), dt, len(names) / max(dt, 1e-9)))
    return results


def _run_procs(net, names, out_dir, batch, mode, write_images, log, procs, pool=None, params=None):
    from multiprocessing import shared_memory
    own_pool = pool is None
    if own_pool:
        pool = decode_pool(procs)
    mode = mode or cfg.TEST.DETECT_MODE
    os.makedirs(out_dir, exist_ok=True)
    jobs, singles, _ = plan(names, batch)
    results, meta = {}, {}
    if jobs:
        net.ensure_capacity(max(len(m) for _, m in jobs), max(s[0] for s, _ in jobs), max(s[1] for s, _ in jobs))
        _set_tail_params(net, params)
    nbytes = max([len(m) * s[0] * s[1] * 3 for s, m in jobs] + [1])
    NB = 4                                                                                  # batches k + 1, k + 2 decode, k is on the GPU, k - 1's pixels are still referenced
    shms = [shared_memory.SharedMemory(create=True, size=nbytes) for _ in range(NB)]
    t0 = time.time()
    try:
        if True:
            def decode(k):
                shape, members = jobs[k]
                bshape = (len(members), shape[0], shape[1], 3)
                return bshape, [pool.submit(_decode_into, nm, shms[k % NB].name, bshape, i) for i, nm in enumerate(members)]
            ahead = {k: decode(k) for k in range(min(2, len(jobs)))}
            pending = None
            for k, (shape, members) in enumerate(jobs):
                bshape, futs = ahead.pop(k)
                arr = np.ndarray(bshape, np.uint8, buffer=shms[k % NB].buf)
                for i, (nm, f) in enumerate(zip(members, futs)):
                    back = f.result()
                    if back is not None:                                   # not at the batch shape yet: resize_im on the GPU, in the parent
                        img, scale = D.resize_im(back, scale=TextLineCfg.SCALE, max_scale=TextLineCfg.MAX_SCALE)
                        arr[i] = img
                        meta[nm] = (None, scale)
                    else:
                        meta[nm] = (None, 1.0)
                if k + 2 < len(jobs):
                    ahead[k + 2] = decode(k + 2)                          # two batches decode while this one is on the GPU
                net.ctx.detect_submit(images=arr, slot=k & 1)
                if pending is not None:
                    slot, mem = pending
                    for nm, recs in zip(mem, net.ctx.detect_collect(slot, mode=mode, line_capacity=1024)):
                        results[nm] = recs
                pending = (k & 1, members)
            if pending is not None:
                slot, mem = pending
                for nm, recs in zip(mem, net.ctx.detect_collect(slot, mode=mode, line_capacity=1024)):
                    results[nm] = recs
    finally:
        if own_pool:
            pool.shutdown()
        for s_ in shms:
            s_.close()
            s_.unlink()
    for nm in singles:
        img, scale = _load(nm)
        from ctpn_amd.lib.fast_rcnn.test import test_ctpn
        scores, boxes = test_ctpn(None, net, img)
        results[nm] = _text_detector(params).detect(boxes, scores[:, np.newaxis], img.shape[:2])
        meta[nm] = (img, scale)
    dt = time.time() - t0
    for nm in names:
        img, scale = meta[nm]
        if write_images:
            if img is None:
                img, scale = _load(nm)
            D.draw_boxes(img.copy(), nm, results[nm], scale, out_dir)
        else:
            base = os.path.basename(nm)
            B.write_result_file(os.path.join(out_dir, 'res_{}.txt'.format(base.split('.')[0])), results[nm], scale)
    log('Detection of {:d} images in {:d} batches took {:.3f}s ({:.1f} images/s)'.format(len(names), len(jobs) + len(singles), dt, len(names) / max(dt, 1e-9)))
    return results


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--input', default='data/demo', help='directory or glob of images')
    ap.add_argument('--out', default='data/results')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--mode', default=None, choices=[None, 'H', 'O'])
    ap.add_argument('--synthetic', type=int, default=None, metavar='SEED')
    ap.add_argument('--no-images', action='store_true', help='write only res_<stem>.txt')
    ap.add_argument('--decode-threads', type=int, default=8, help='host threads decoding / resizing the next batch')
    ap.add_argument('--decode-procs', type=int, default=0, help='decode in this many worker PROCESSES (shared-memory batches) instead of threads')
    ap.add_argument('--decode', default='host', choices=['host', 'gpu', 'gpu-entropy'],
                    help="gpu: JPEG decode + resize_im on the device (ctpn_decode_jpeg_batch); gpu-entropy: the same with the Huffman decode on the device too "
                         "(ctpn_decode_jpeg_files_device; progressive files keep the host-entropy call)")
    ap.add_argument('--encode', default='host', choices=['host', 'gpu', 'gpu-entropy'],
                    help="gpu (with --decode gpu): annotated JPEG images drawn, resized and coded by the library (ctpn_write_annotated_files); "
                         "gpu-entropy: the same with the Huffman coding on the device too (ctpn_write_annotated_files_device)")
    ap.add_argument('--png-encode', default='host', choices=['host', 'gpu'],
                    help="gpu (with --decode gpu): the PNG-named annotated images of library-decoded batches drawn, resized and PNG-coded on the "
                         "device (ctpn_write_annotated_png_files); host: Pillow")
    ap.add_argument('--crops', default=None, metavar='DIR',
                    help="(with --decode gpu) also write every detected line as a rectified crop <stem>_<k>.jpg of height --crop-height into DIR (ctpn_crop_lines)")
    ap.add_argument('--crop-height', type=int, default=32)
    ap.add_argument('--crops-encode', default='host', choices=['host', 'gpu', 'gpu-entropy'],
                    help="with --crops: 'gpu' = the library JPEG-codes and writes the crops where they are cut (ctpn_write_line_crops); 'gpu-entropy' = with "
                         "the Huffman coding on the device too; 'host' (default) = Pillow. Same files")
    ap.add_argument('--ragged', action='store_true',
                    help="batch images of one resized width across heights (same result files); with --decode gpu / gpu-entropy the JPEG files "
                         "are decoded into ragged canvases on the device whatever their file sizes (not with --encode gpu, --png-encode gpu, --crops)")
    ap.add_argument('--ragged-outputs', action='store_true',
                    help="with --ragged and --decode gpu / gpu-entropy: --encode gpu / gpu-entropy and --crops take the ragged batches too "
                         "(ctpn_write_annotated_files_ragged, ctpn_crop_lines_ragged, ctpn_write_line_crops_ragged); same files")
    ap.add_argument('--crops-format', default='jpg', choices=['jpg', 'png'],
                    help="with --crops: 'png' = lossless <stem>_<k>.png crops (--crops-encode gpu: ctpn_write_line_crops_png; not with gpu-entropy)")
    ap.add_argument('--ragged-png', action='store_true',
                    help="with --ragged --ragged-outputs --png-encode gpu: the PNG files share ragged batches too and are written from their "
                         "canvases (ctpn_write_annotated_png_files_ragged); same names, same pixels")
    ap.add_argument('--ragged-pack', default='host', choices=['host', 'gpu'],
                    help="with --ragged and --decode gpu / gpu-entropy: 'gpu' = the PNG files share ragged batches whose canvases are built on the "
                         "device (ctpn_decode_png_files_ragged); 'host' (default) = as without the switch. Same result files")
    ap.add_argument('--ragged-waste', type=float, default=RAGGED_WASTE, help="padded share of a ragged batch's rows at most")
    ap.add_argument('--precision', default=None, choices=['split', 'fp32', 'fp16', 'bf16'],
                    help="arithmetic of the conv stack; default: cfg.TEST.PRECISION (text.yml: split, the parity-grade mode). bf16 is the "
                         "throughput choice (3.2 x split's rate, outside the 1e-3 / 1 px bar)")
    ap.add_argument('--rpn-post-nms-top-n', type=int, default=None, metavar='N',
                    help="cfg.TEST.RPN_POST_NMS_TOP_N for this run (the reference's default, and text.yml's: 1000; up to %d). A dense page holds more "
                         "16-pixel slices than that, and its lines break into fragments at the default" % B.POST_NMS_CAPACITY_MAX)
    ap.add_argument('--connector', action='append', default=[], metavar='NAME=VALUE', type=_connector_item,
                    help="a threshold of the text-line connector (the reference's TextLineCfg; repeatable): " + ", ".join(B.CONNECTOR_PARAM_NAMES) +
                         ". Sets the ctx's parameters for the batches and the detector of the single-image path")
    return ap


def _connector_item(text):
    try:
        parse_connector_args([text])
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return text


def main(argv=None):
    args = build_parser().parse_args(argv)
    yml = 'ctpn/text.yml' if os.path.exists('ctpn/text.yml') else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'text.yml')
    cfg_from_file(yml)
    if args.precision:
        cfg.TEST.PRECISION = args.precision
    if args.rpn_post_nms_top_n is not None:
        if not 1 <= args.rpn_post_nms_top_n <= B.POST_NMS_CAPACITY_MAX:
            raise SystemExit('--rpn-post-nms-top-n must be in 1..%d' % B.POST_NMS_CAPACITY_MAX)
        cfg.TEST.RPN_POST_NMS_TOP_N = args.rpn_post_nms_top_n      # both paths read it: rpn_params_from_cfg below, lib/fast_rcnn/test.py
    net = get_network("VGGnet_test")
    D.load_weights(net, args.synthetic)
    names = list_images(args.input)
    if not names:
        raise SystemExit('no images under ' + args.input)
    run(net, names, args.out, batch=args.batch, mode=args.mode, write_images=not args.no_images, decode_threads=args.decode_threads,
        decode_procs=args.decode_procs, decode=args.decode, encode=args.encode, png_encode=args.png_encode, crops_dir=args.crops, crop_h=args.crop_height, crops_encode=args.crops_encode,
        params=dict(rpn_params_from_cfg(), **parse_connector_args(args.connector)), ragged=args.ragged, ragged_waste=args.ragged_waste,
        ragged_outputs=args.ragged_outputs, crops_format=args.crops_format, ragged_png=args.ragged_png, ragged_pack=args.ragged_pack)
    net.close()


if __name__ == '__main__':
    main()
