"""TEST INFRASTRUCTURE ONLY: the training data layer restated in numpy, from the definitions in include/ctpn_hip_data_layer.h.

  split_quad / split_labels   lib/prepare_training_data/split_label.py:36-104: the scaling in IEEE double (divide, then multiply, truncate),
                              the stable sort by x, pt1 .. pt4, the clamps, and the strip lists built the way the definition words them
                              (x_left / x_right, then the deletion) -- not the closed form csrc/data_layer_dev.h counts with
  flip_boxes / train_boxes    imdb.append_flipped_images on uint16 boxes and minibatch.py:31
  train_page                  oracle/resize_ref.py's resize, mirrored after it, and the float64 blob rounded once
  order                       layer.py:14-27 and minibatch.py:12 on a RandomState
tests/test_data_layer.py holds this file against the recorded results of the reference's own code (tests/golden/data_layer.npz)."""
import numpy as np

from oracle import resize_ref

PIXEL_MEANS = np.array([102.9801, 115.9465, 122.7717], np.float64)


def parse_quads(text):
    """a label file's text -> (Q, 8) float64"""
    rows = [[float(v) for v in line.strip().lower().split(",")[:8]] for line in text.splitlines() if line.strip()]
    return np.array(rows, np.float64).reshape(-1, 8)


def scale(v, file_size, resized_size):
    return int(np.float64(v) / np.float64(file_size) * np.float64(resized_size))


def quad_span(q8, dims4):
    """-> xmin, xmax, ymin, ymax on the resized page"""
    fh, fw, rh, rw = (int(v) for v in dims4)
    xs = [scale(q8[2 * k], fw, rw) for k in range(4)]
    ys = [scale(q8[2 * k + 1], fh, rh) for k in range(4)]
    order = sorted(range(4), key=lambda k: xs[k])      # sorted() is stable
    x, y = [xs[k] for k in order], [ys[k] for k in order]
    (pt1, pt3) = ((x[0], y[0]), (x[1], y[1])) if y[0] < y[1] else ((x[1], y[1]), (x[0], y[0]))
    (pt2, pt4) = ((x[2], y[2]), (x[3], y[3])) if y[2] < y[3] else ((x[3], y[3]), (x[2], y[2]))
    xmin, ymin = min(pt1[0], pt2[0]), min(pt1[1], pt2[1])
    xmax, ymax = max(pt2[0], pt4[0]), max(pt3[1], pt4[1])
    return max(xmin, 0), min(xmax, rw - 1), max(ymin, 0), min(ymax, rh - 1)


def strips_x(xmin, xmax):
    """the (x1, x2) list of one quad"""
    if xmin == xmax:
        return []      # the extension: the reference stops here
    start = -(-xmin // 16) * 16      # ceil(xmin / 16) * 16 ...
    if start == xmin:
        start = xmin + 16            # ... the first multiple of 16 above xmin
    lefts = [xmin] + list(range(start, xmax, 16))
    rights = [start - 1] + [v + 15 for v in lefts[1:-1]] + [xmax]
    # where no multiple of 16 lies strictly between, rights is one longer than lefts: the pairs are (lefts[i], rights[i])
    return [(a, b) for a, b in zip(lefts, rights) if a != b]


def split_quad(q8, dims4):
    xmin, xmax, ymin, ymax = quad_span(q8, dims4)
    return [(a, ymin, b, ymax) for a, b in strips_x(xmin, xmax)]


def split_labels(page_dims, quads, quad_offsets):
    """-> strips (S, 4) float32, strip_offsets (pages + 1,), quad_strip_offsets (Q + 1,)"""
    dims = np.asarray(page_dims).reshape(-1, 4)
    quads = np.asarray(quads, np.float64).reshape(-1, 8)
    rows, page_offs, quad_offs = [], [0], [0]
    for p in range(dims.shape[0]):
        for q in range(int(quad_offsets[p]), int(quad_offsets[p + 1])):
            rows += split_quad(quads[q], dims[p])
            quad_offs.append(len(rows))
        page_offs.append(len(rows))
    return np.array(rows, np.float32).reshape(-1, 4), np.array(page_offs, np.int32), np.array(quad_offs, np.int32)


def flip_boxes(boxes_u16, width):
    """imdb.py:88-95 on a uint16 array, in explicit modulo-2^16 integer arithmetic"""
    b = np.asarray(boxes_u16).astype(np.int64).copy()
    x1, x2 = b[:, 0].copy(), b[:, 2].copy()
    b[:, 0] = (int(width) - x2 - 1) % 65536
    b[:, 2] = (int(width) - x1 - 1) % 65536
    b[b[:, 2] < b[:, 0], 0] = 0
    return b.astype(np.uint16)


def train_boxes(strips, width, flip, scale_):
    s = np.asarray(strips, np.float32).reshape(-1, 4)
    assert ((s >= 0) & (s <= 65535)).all()
    b = s.astype(np.uint16)
    if flip:
        b = flip_boxes(b, width)
    out = np.empty((b.shape[0], 5), np.float32)
    out[:, :4] = b.astype(np.float64) * np.float64(scale_)
    out[:, 4] = 1.0
    return out


def train_page(image, factor, flip):
    """-> (image_out uint8, blob float32)"""
    img = np.asarray(image)
    out = resize_ref.resize_linear(img, factor, factor) if (factor > 0 and factor != 1) else img.copy()
    if flip:
        out = np.flip(out, axis=1)
    out = np.ascontiguousarray(out)
    return out, (out.astype(np.float64) - PIXEL_MEANS).astype(np.float32)


def order(length, seed, count, n_scales=1):
    """-> [(index, scale index)] * count: RoIDataLayer over `length` entries, one randint per record after its index"""
    rs = np.random.RandomState(seed)
    perm, cur, out = rs.permutation(np.arange(length)), 0, []
    for _ in range(count):
        if cur + 1 >= length:
            perm, cur = rs.permutation(np.arange(length)), 0
        ind = int(perm[cur])
        cur += 1
        out.append((ind, int(rs.randint(0, high=n_scales, size=1)[0])))
    return out
