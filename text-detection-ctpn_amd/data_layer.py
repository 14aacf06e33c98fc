"""The training data layer over the C ABI (include/ctpn_hip_data_layer.h): what the reference does to a labelled folder before a step sees it.

split_labels is lib/prepare_training_data/split_label.py:36-104 for a whole label set (ctpn_split_labels), train_page one decoded page
resized, mirrored and mean-subtracted (ctpn_train_page), train_boxes imdb.append_flipped_images and minibatch.py:29-32 for one page's strips
(ctpn_train_boxes). DataLayer chains them in lib/roi_data_layer/layer.py's visiting order: the label database stays in HBM, the page, the
blob and the boxes of every step are written by kernels, and a worker thread decodes the next file meanwhile.

Departures from the reference's pipeline, both on purpose: its second resize (prep_im_for_blob) runs on the float image after the mean
subtraction and its first is followed by a JPEG round trip through re_image/; here both resizes run on uint8 and no file is rewritten.
RANDOM_DOWNSAMPLE, ASPECT_GROUPING, dontcare_areas and gt_ishard are not built (split_label.py's labels carry none)."""
import collections
import ctypes as C
import os
import queue
import threading

import numpy as np

from . import _binding as B
from .targets import _dev_ptr, _is_torch

Record = collections.namedtuple("Record", "image_dev blob_dev gt_dev hw page flipped im_scale")


def _rule(h, w, target, max_size):
    """the factor rule split_label.py:27-29 and prep_im_for_blob (blob.py:26-31) share: the short side to `target`, the long side capped"""
    lo, hi = min(int(h), int(w)), max(int(h), int(w))
    f = float(target) / float(lo)
    if np.round(f * hi) > max_size:
        f = float(max_size) / float(hi)
    return f


def split_label_dims(h, w, scale=600, max_scale=1200):
    """split_label.py:27-31 for an h x w file -> (factor, (resized h, resized w)): the short side to 600 unless the long side would pass
    1200, the size cv2.resize gives (ctpn_resize_dims: round half to even)"""
    f = _rule(h, w, scale, max_scale)
    return f, B.resize_dims(h, w, f, f)


def prep_scale(h, w, target_size=600, max_size=1000):
    """prep_im_for_blob's im_scale (blob.py:26-31) for an h x w page"""
    return _rule(h, w, target_size, max_size)


def read_quads(path):
    """An ICDAR-style label file -> (Q, 8) float64: x1,y1,x2,y2,x3,y3,x4,y4 per line, further comma fields ignored (split_label.py:37).
    Blank lines are skipped; a line without eight numbers is an error that names the file and the line."""
    quads = []
    with open(path, encoding="utf-8-sig") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            parts = line.strip().lower().split(",")
            try:
                if len(parts) < 8:
                    raise ValueError
                q = [float(v) for v in parts[:8]]
                if not all(np.isfinite(q)):
                    raise ValueError
                quads.append(q)
            except ValueError:
                raise ValueError("%s:%d: expected `x1,y1,x2,y2,x3,y3,x4,y4[,...]`, got %r" % (path, no, line.rstrip("\r\n")))
    return np.array(quads, np.float64).reshape(-1, 8)


def quad_label_path(labels_dir, image_path):
    """gt_<stem>.txt (split_label.py:19) or <stem>.txt under labels_dir, or None"""
    stem = os.path.splitext(os.path.basename(image_path))[0]
    for name in ("gt_" + stem + ".txt", stem + ".txt"):
        p = os.path.join(labels_dir, name)
        if os.path.exists(p):
            return p
    return None


def split_labels(page_dims, quads, quad_offsets, device_id=0, on_device=False, want_quad_offsets=False):
    """ctpn_split_labels. page_dims: (pages, 4) ints (file h, file w, resized h, resized w); quads: (Q, 8) float64, numpy or (on_device) a
    torch tensor on cuda:device_id; quad_offsets: pages + 1 ints -> (strips (S, 4) float32 -- a torch tensor on the device with on_device,
    else numpy --, strip_offsets (pages + 1,) int32 numpy[, quad_strip_offsets (Q + 1,) int32 of strips' kind])."""
    lib = B.load_library()
    dims = np.ascontiguousarray(page_dims, dtype=np.int32).reshape(-1, 4)
    offs = np.ascontiguousarray(quad_offsets, dtype=np.int32).reshape(-1)
    pages = int(dims.shape[0])
    if offs.shape[0] != pages + 1:
        raise ValueError("split_labels: quad_offsets holds pages + 1 ints")
    nq = int(offs[-1]) if pages else 0
    i32p = C.POINTER(C.c_int)
    strip_offs = np.zeros((pages + 1,), np.int32)
    if on_device:
        import torch
        dev = torch.device("cuda", int(device_id))
        if not _is_torch(quads):
            quads = torch.from_numpy(np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)).to(dev)
        if int(quads.shape[0]) != nq:
            raise ValueError("split_labels: quads' rows differ from quad_offsets' total")
        p_q = _dev_ptr(quads, torch.float64, device_id, "quads")
        qso = torch.empty((nq + 1,), dtype=torch.int32, device=dev) if want_quad_offsets else None
        p_qso = None if qso is None else C.c_void_p(qso.data_ptr())
        torch.cuda.current_stream(dev).synchronize()      # the call runs on a stream of its own
    else:
        quads = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)
        if quads.shape[0] != nq:
            raise ValueError("split_labels: quads' rows differ from quad_offsets' total")
        p_q = quads.ctypes.data_as(C.c_void_p) if nq else None
        qso = np.zeros((nq + 1,), np.int32) if want_quad_offsets else None
        p_qso = None if qso is None else qso.ctypes.data_as(C.c_void_p)
    call = lambda p_s, cap: lib.ctpn_split_labels(int(device_id), pages, dims.ctypes.data_as(i32p), p_q, offs.ctypes.data_as(i32p), 1 if on_device else 0,      # noqa: E731
                                                  p_s, cap, strip_offs.ctypes.data_as(i32p), p_qso)
    B._check(call(None, 0))      # the probe
    total = int(strip_offs[-1])
    if on_device:
        strips = torch.empty((total, 4), dtype=torch.float32, device=dev)
        p_s = C.c_void_p(strips.data_ptr()) if total else None
    else:
        strips = np.empty((total, 4), np.float32)
        p_s = strips.ctypes.data_as(C.c_void_p) if total else None
    if total:
        B._check(call(p_s, total))
    return (strips, strip_offs, qso) if want_quad_offsets else (strips, strip_offs)


def train_page(image, factor, flip=False, device_id=0, want_blob=True):
    """ctpn_train_page: image (h, w, 3) uint8 BGR -- a numpy array (its rows may be strided) or a torch tensor on cuda:device_id -- ->
    (image_out (oh, ow, 3) uint8, blob_out (oh, ow, 3) float32 or None), torch tensors on the device: ctpn_resize(image, factor), mirrored
    after the resize where flip is set, and that page minus PIXEL_MEANS."""
    import torch
    lib = B.load_library()
    dev = torch.device("cuda", int(device_id))
    if _is_torch(image):
        if not image.is_cuda or image.device.index != int(device_id) or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or \
                image.stride(2) != 1 or image.stride(1) != 3:
            raise ValueError("train_page: an (h, w, 3) uint8 tensor with dense rows on cuda:%d" % device_id)
        h, w, pitch, ptr, on_dev = int(image.shape[0]), int(image.shape[1]), int(image.stride(0)) if image.shape[0] > 1 else 3 * int(image.shape[1]), image.data_ptr(), 1
        torch.cuda.current_stream(dev).synchronize()
    else:
        a = np.asarray(image)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("train_page: an (h, w, 3) uint8 image")
        if a.strides[2] != 1 or a.strides[1] != 3 or (a.shape[0] > 1 and a.strides[0] < 3 * a.shape[1]):
            a = np.ascontiguousarray(a)
        image = a      # kept alive over the call
        h, w, pitch, ptr, on_dev = int(a.shape[0]), int(a.shape[1]), int(a.strides[0]) if a.shape[0] > 1 else 3 * int(a.shape[1]), a.ctypes.data, 0
    f = float(factor)
    oh, ow = B.resize_dims(h, w, f, f) if (f > 0.0 and f != 1.0) else (h, w)
    out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev)
    blob = torch.empty((oh, ow, 3), dtype=torch.float32, device=dev) if want_blob else None
    B._check(lib.ctpn_train_page(int(device_id), C.c_void_p(ptr), on_dev, h, w, pitch, f, 1 if flip else 0, C.c_void_p(out.data_ptr()),
                                 None if blob is None else C.c_void_p(blob.data_ptr()), oh, ow))
    return out, blob


def train_boxes(strips, page_width, flip=False, scale=1.0, device_id=0):
    """ctpn_train_boxes: strips (G, 4) float32 x1, y1, x2, y2 -> gt boxes (G, 5) float32, numpy -> numpy, a torch tensor on cuda:device_id ->
    a tensor there: the uint16 flip about page_width where flip is set, every coordinate x scale, the class 1.0."""
    lib = B.load_library()
    if _is_torch(strips):
        import torch
        g = int(strips.shape[0])
        p_in = _dev_ptr(strips.reshape(-1, 4), torch.float32, device_id, "strips")
        out = torch.empty((g, 5), dtype=torch.float32, device=strips.device)
        p_out = C.c_void_p(out.data_ptr()) if g else None
        torch.cuda.current_stream(strips.device).synchronize()
        on_dev = 1
    else:
        strips = B._f32(strips).reshape(-1, 4)
        g = int(strips.shape[0])
        out = np.empty((g, 5), np.float32)
        p_in, p_out, on_dev = (strips.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 0) if g else (None, None, 0)
    B._check(lib.ctpn_train_boxes(int(device_id), p_in, g, int(page_width), 1 if flip else 0, float(scale), on_dev, p_out))
    return out


class DataLayer(object):
    """lib/roi_data_layer/layer.py's RoIDataLayer with imdb.append_flipped_images, over the three calls above.

    image_paths: the pages' files; quads_per_page: one (Q_i, 8) array per page (read_quads). At construction the layer reads the files'
    sizes from their headers (no image is decoded), runs split_labels once for the whole set and keeps the strips and their offsets in HBM:
    the resident label database. label_scale, label_max_size: split_label.py's 600 and 1200; scales, max_size: cfg.TRAIN.SCALES, MAX_SIZE.

    next() -> Record(image_dev (h, w, 3) uint8, blob_dev (h, w, 3) float32, gt_dev (G, 5) float32, (h, w), page, flipped, im_scale).
    The page is train_page by split_label_dims' factor with the entry's flip; then, only where prep_im_for_blob's rule on the resized size
    gives a factor other than 1, a second train_page pass by that factor without flip, on uint8 like the first; the blob comes from the last
    pass; the boxes are train_boxes on the page's slice of the resident strips with scale = that second factor (im_scale; 1.0 without one).

    The order is the reference's: a np.random.RandomState(seed) of the layer's own; entries 0 .. N-1 plain and N .. 2N-1 mirrored where
    flipped is set; a new permutation at construction and whenever cur + 1 >= len (so the last entry of a permutation is never served);
    one randint(0, len(scales), 1) per record, after its index. The layer draws one record ahead, in that same order, to know which file to
    read next. The sequence equals the reference's after np.random.seed(seed) only when nothing else draws from numpy's global generator
    in between -- the reference's anchor subsampling does, so a run of the reference with RPN_BATCHSIZE on visits another order.

    prefetch: one worker thread reads and decodes the NEXT entry's file (imutil.imread) while the caller steps; it makes no GPU call and
    touches no ctx -- every device call stays on the caller's thread -- and the records are the same bytes with and without it. close()
    joins the thread; the layer is a context manager."""

    def __init__(self, device_id, image_paths, quads_per_page, flipped=True, seed=3, scales=(600,), max_size=1000, prefetch=True, label_scale=600,
                 label_max_size=1200):
        from .lib.utils import image as imutil
        self._imread = imutil.imread
        self.device_id = int(device_id)
        self.paths = [str(p) for p in image_paths]
        n = len(self.paths)
        if n == 0 or len(quads_per_page) != n:
            raise ValueError("DataLayer: at least one page, one quad array per page")
        self.scales, self.max_size, self.flipped = tuple(int(s) for s in scales), int(max_size), bool(flipped)
        if not self.scales:
            raise ValueError("DataLayer: scales is empty")
        dims, self.factors = np.zeros((n, 4), np.int32), []
        for i, p in enumerate(self.paths):
            h, w = imutil.image_size(p)
            f, (rh, rw) = split_label_dims(h, w, label_scale, label_max_size)
            dims[i] = (h, w, rh, rw)
            self.factors.append(f)
        self.page_dims = dims
        quads = [np.asarray(q, np.float64).reshape(-1, 8) for q in quads_per_page]
        offs = np.zeros((n + 1,), np.int32)
        offs[1:] = np.cumsum([q.shape[0] for q in quads])
        self.strips_dev, self.strip_offsets = split_labels(dims, np.concatenate(quads, axis=0), offs, self.device_id, on_device=True)
        self._rng = np.random.RandomState(seed)
        self._len = n * (2 if self.flipped else 1)
        self._shuffle()
        self._pending = self._draw()
        self._prefetch = bool(prefetch)
        self._thread, self._asked = None, None
        if self._prefetch:
            self._requests, self._results = queue.Queue(), queue.Queue()
            self._thread = threading.Thread(target=self._worker, name="ctpn-data-layer", daemon=True)
            self._thread.start()

    # ---- the order: layer.py:14-27, minibatch.py:12
    def _shuffle(self):
        self._perm = self._rng.permutation(np.arange(self._len))
        self._cur = 0

    def _draw(self):
        if self._cur + 1 >= self._len:
            self._shuffle()
        ind = int(self._perm[self._cur])
        self._cur += 1
        return ind, int(self._rng.randint(0, high=len(self.scales), size=1)[0])

    def second_factor(self, page, scale_ind=0):
        """prep_im_for_blob's factor for `page` at scales[scale_ind], on its resized size"""
        return prep_scale(int(self.page_dims[page, 2]), int(self.page_dims[page, 3]), self.scales[scale_ind], self.max_size)

    def page_shape(self, page, scale_ind=0):
        """(h, w) of the record `page` gives at scales[scale_ind]"""
        rh, rw = int(self.page_dims[page, 2]), int(self.page_dims[page, 3])
        f = self.second_factor(page, scale_ind)
        return (rh, rw) if f == 1.0 else B.resize_dims(rh, rw, f, f)

    def max_shape(self):
        """(the largest h, the largest w) any record can have: what a ctx's capacity must cover"""
        shapes = [self.page_shape(p, s) for p in range(len(self.paths)) for s in range(len(self.scales))]
        return max(s[0] for s in shapes), max(s[1] for s in shapes)

    # ---- the files
    def _worker(self):
        while True:
            page = self._requests.get()
            if page is None:
                return
            try:
                self._results.put((page, self._imread(self.paths[page]), None))
            except Exception as e:      # handed to the caller's thread, raised by the next() that wanted the page
                self._results.put((page, None, e))

    def _image(self, page):
        if self._asked is not None:
            got, img, err = self._results.get()
            self._asked = None
            if got == page:
                if err is not None:
                    raise err
                return img
        return self._imread(self.paths[page])

    def next(self):
        if self.strips_dev is None:
            raise ValueError("DataLayer: closed")
        ind, scale_ind = self._pending
        self._pending = self._draw()
        n = len(self.paths)
        page, flip = ind % n, ind >= n
        img = self._image(page)
        if self._prefetch:
            self._asked = self._pending[0] % n
            self._requests.put(self._asked)
        fh, fw, rh, rw = (int(v) for v in self.page_dims[page])
        if img.shape[0] != fh or img.shape[1] != fw:
            raise ValueError("%s: decoded as %d x %d, its header said %d x %d" % (self.paths[page], img.shape[0], img.shape[1], fh, fw))
        second = self.second_factor(page, scale_ind)
        image_dev, blob_dev = train_page(img, self.factors[page], flip, self.device_id, want_blob=second == 1.0)
        if second != 1.0:
            image_dev, blob_dev = train_page(image_dev, second, False, self.device_id)
        o0, o1 = int(self.strip_offsets[page]), int(self.strip_offsets[page + 1])
        gt_dev = train_boxes(self.strips_dev[o0:o1], rw, flip, second, self.device_id)
        return Record(image_dev, blob_dev, gt_dev, (int(image_dev.shape[0]), int(image_dev.shape[1])), page, bool(flip), float(second))

    __next__ = next

    def __iter__(self):
        return self

    def close(self):
        if self._thread is not None:
            self._requests.put(None)
            self._thread.join()
            self._thread = None
        self.strips_dev = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
