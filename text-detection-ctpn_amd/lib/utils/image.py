"""Image helpers standing in for the cv2 calls on the demo path (cv2 is not installed in this image):
cv2.resize(..., INTER_LINEAR) (reference ctpn/demo.py:25,51; lib/fast_rcnn/test.py:23) runs on the GPU through
ctpn_resize (csrc/preprocess.hip; OpenCV 3.4's algorithm restated, uint8 fixed-point and float32 paths -- parity with
the real cv2 UNPINNED, bit-exact against oracle/resize_ref.py); cv2.imread / imwrite (demo.py:52,59) go through Pillow.
There is no host implementation of the resize here: without a GPU a non-identity resize raises.
"""
import numpy as np

from ..._binding import resize_dims, resize_linear


def resize_bilinear(im, fx, fy, device_id=0):
    """cv2.resize(im, None, None, fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR); (h,w,3) uint8 or float32."""
    im = np.asarray(im)
    h, w = im.shape[:2]
    if resize_dims(h, w, fx, fy) == (h, w) and fx == 1.0 and fy == 1.0:
        return im.copy()                       # every sample falls on a source pixel with weight 1: exact copy, like cv2
    return resize_linear(im, fx, fy, device_id)


def _oriented(f):
    """cv2.imread turns a JPEG by its EXIF orientation tag (OpenCV >= 3.1 unless IMREAD_IGNORE_ORIENTATION; the reference calls it with the
    default flags, ctpn/demo.py:59); Pillow leaves that to the caller. JPEG only: that is where OpenCV 3.x looks for EXIF."""
    if f.format == "JPEG" and f.getexif().get(0x0112, 1) != 1:
        from PIL import ImageOps
        return ImageOps.exif_transpose(f)
    return f


def open_rgb(path):
    """(h, w, 3) RGB uint8 of an image file the way cv2.imread(path) sees it (orientation applied, alpha dropped), before the BGR flip."""
    from PIL import Image
    with Image.open(path) as f:
        if f.format == "PNG" and f.mode in ("I", "I;16", "I;16B"):
            # a 16-bit gray PNG: libpng hands cv2.imread(IMREAD_COLOR) the high byte of every sample (png_set_strip_16); Pillow's
            # convert("RGB") would clip at 255 instead
            g = (np.asarray(f).astype(np.uint16) >> 8).astype(np.uint8)
            return np.repeat(g[:, :, None], 3, axis=2)
        return np.asarray(_oriented(f).convert("RGB"))


def image_size(path):
    """(h, w) of what imread(path) returns, from the file header only (no pixel decode)."""
    from PIL import Image
    with Image.open(path) as f:
        w, h = f.size
        if f.format == "JPEG" and f.getexif().get(0x0112, 1) in (5, 6, 7, 8):
            w, h = h, w
    return h, w


def imread(path):
    """BGR uint8 HWC like cv2.imread(path). PNG files go through the library's decoder (ctpn_png_decode: reading is host work by the nature of the format,
    libdeflate + row filters, byte-equal to Pillow's result at half its time); what it does not take (16-bit PNG) and every other format
    through Pillow."""
    if str(path).lower().endswith(".png"):
        from ..._binding import CtpnError, png_decode
        try:
            with open(path, "rb") as f:
                return png_decode(f.read())
        except CtpnError:
            pass
    return np.ascontiguousarray(open_rgb(path)[:, :, ::-1])


def imwrite(path, bgr):
    """cv2.imwrite(path, img) with its default parameters (reference ctpn/demo.py:52): JPEG at quality 95 (IMWRITE_JPEG_QUALITY's default; Pillow's
    own default would be 75) with libjpeg's default 4:2:0 sampling, PNG at compression level 1 (3.x: IMWRITE_PNG_COMPRESSION = 1 -- lossless
    either way). The format follows the file name's extension, as in OpenCV."""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]))
    ext = path.rsplit(".", 1)[-1].lower() if "." in path else ""
    if ext in ("jpg", "jpeg", "jpe"):
        im.save(path, quality=95, subsampling=2)
    elif ext == "png":
        im.save(path, compress_level=1)
    else:
        im.save(path)


def imencode_jpeg_batch(ctx, images, quality=95, device_ptr=None, shape=None, entropy="host"):
    """cv2.imencode('.jpg', img, [IMWRITE_JPEG_QUALITY, quality]) for a batch of BGR uint8 images of one size, on the GPU
    (ctpn_encode_jpeg_batch): (n, h, w, 3) on the host, or device_ptr + shape -> list of n bytes objects, byte-equal to what imwrite above
    puts into a .jpg file at the same quality. entropy="device": the Huffman coding on the device too (ctpn_encode_jpeg_batch_device)."""
    return ctx.encode_jpeg_batch(images, quality=quality, device_ptr=device_ptr, shape=shape, entropy=entropy)


def imwrite_jpeg_batch(ctx, paths, images, quality=95, device_ptr=None, shape=None, entropy="host"):
    """imwrite for a batch of JPEG files: encoded by imencode_jpeg_batch, one file per image."""
    paths = list(paths)
    files = imencode_jpeg_batch(ctx, images, quality=quality, device_ptr=device_ptr, shape=shape, entropy=entropy)
    assert len(files) == len(paths)
    for path, data in zip(paths, files):
        with open(path, "wb") as f:
            f.write(data)


def imencode_png_batch(ctx, images, device_ptr=None, shape=None):
    """cv2.imencode('.png', img) for a batch of BGR uint8 images of one size, on the GPU (ctpn_encode_png_batch): (n, h, w, 3) on the host,
    or device_ptr + shape -> list of n bytes objects. Lossless: every decoder returns the pixels; the bytes are this library's own (Sub
    filter, run-length and row-above matches, one dynamic-Huffman block), not Pillow's or cv2's."""
    return ctx.encode_png_batch(images, device_ptr=device_ptr, shape=shape)


def imwrite_png_batch(ctx, paths, images, device_ptr=None, shape=None):
    """imwrite for a batch of PNG files: encoded by imencode_png_batch, one file per image."""
    paths = list(paths)
    files = imencode_png_batch(ctx, images, device_ptr=device_ptr, shape=shape)
    assert len(files) == len(paths)
    for path, data in zip(paths, files):
        with open(path, "wb") as f:
            f.write(data)


def imwrite_annotated_ragged(ctx, paths, canvas, heights, recs, scales, quality=95, device_ptr=None, shape=None, entropy="host"):
    """draw_boxes + cv2.resize(1 / scale) + imwrite for a RAGGED batch, on the GPU (ctpn_write_annotated_files_ragged): canvas (n, hc, w, 3)
    BGR uint8 on the host (lib/utils/blob.py im_list_to_canvas), or device_ptr + shape = (n, hc, w) for a canvas that is on the device
    already; image i is rows [0, heights[i]) of slot i, resized by 1 / scales[i] and written to paths[i] at its own size, byte-equal to
    the uniform batch writer's file of that image alone. entropy="device": the Huffman coding on the device too."""
    ctx.write_annotated_files_ragged(images=canvas, device_ptr=device_ptr, shape=shape, heights=heights, recs=recs, scales=scales, paths=list(paths),
                                     quality=quality, entropy=entropy)


def imencode_png_mixed(ctx, images):
    """cv2.imencode('.png', img) for a list of BGR uint8 images of ANY mix of sizes in one call, on the GPU (ctpn_encode_png_mixed) -> list of
    bytes objects, each byte-equal to imencode_png_batch of that image alone."""
    return ctx.encode_png_mixed(images)


def imwrite_annotated_png_ragged(ctx, paths, canvas, heights, recs, scales, device_ptr=None, shape=None):
    """imwrite_annotated_ragged for PNG-named files (ctpn_write_annotated_png_files_ragged): lossless, image i byte-equal to the uniform PNG
    writer's file of that image alone. canvas: (n, hc, w, 3) on the host (PNG files are decoded there), or device_ptr + shape."""
    ctx.write_annotated_png_files_ragged(images=canvas, device_ptr=device_ptr, shape=shape, heights=heights, recs=recs, scales=scales, paths=list(paths))


def crop_text_lines(ctx, images, recs, line_counts=None, crop_h=32, max_w=512, pad_value=0, device_ptr=None, shape=None):
    """The detected text lines of a batch as rectified images of height crop_h, one per line, for a recogniser -- cut out on the GPU
    (ctpn_crop_lines): the quadrilateral of every record mapped bilinearly onto crop_h x width pixels with cv2.resize's INTER_LINEAR uint8
    arithmetic, border replicated. images: (n, h, w, 3) BGR uint8 on the host, or device_ptr + shape for a batch that is on the device
    already. -> (crops (total, crop_h, max_w, 3), widths (total,)); crop k is crops[k, :, :widths[k]]."""
    return ctx.crop_lines(images, recs, line_counts, crop_h=crop_h, max_w=max_w, pad_value=pad_value, device_ptr=device_ptr, shape=shape)


def draw_line(img, p0, p1, color, thickness=2):
    """Bresenham-free dense line rasteriser (enough for the annotated demo output)."""
    x0, y0 = p0
    x1, y1 = p1
    n = int(max(abs(x1 - x0), abs(y1 - y0))) + 1
    xs = np.rint(np.linspace(x0, x1, n)).astype(np.int64)
    ys = np.rint(np.linspace(y0, y1, n)).astype(np.int64)
    r = max(thickness // 2, 0)
    h, w = img.shape[:2]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            yy, xx = ys + dy, xs + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            img[yy[ok], xx[ok]] = color
