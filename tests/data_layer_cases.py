"""TEST INFRASTRUCTURE ONLY: the label sets and page shapes tests/test_data_layer.py (the kernels' text on the host) and
tests/test_gpu_data_layer.py (the kernels) share."""
import numpy as np

import data_layer_ref as R

# h, w, factor: whole 16-byte groups at factor 1; odd sizes at factor 1 (1173 bytes: a last group of 5); the case at which resize-then-mirror
# and mirror-then-resize differ (42 x 62); a reduction (20 x 32); an enlargement (66 x 100: 19800 bytes, the last group half full)
PAGE_CASES = [(16, 16, 1.0), (17, 23, 1.0), (31, 45, 1.37), (40, 64, 0.5), (33, 50, 2.0)]


def label_set(golden):
    """the fixture as split_labels' arguments and the reference's strips in one array"""
    stems = [str(s) for s in golden["stems"]]
    quads = [R.parse_quads(str(golden["text_" + s])) for s in stems]
    offs = np.zeros(len(stems) + 1, np.int32)
    offs[1:] = np.cumsum([q.shape[0] for q in quads])
    want = np.concatenate([golden["strips_" + s] for s in stems], axis=0).astype(np.float32)
    want_offs = np.zeros(len(stems) + 1, np.int32)
    want_offs[1:] = np.cumsum([golden["strips_" + s].shape[0] for s in stems])
    return golden["page_dims"], np.concatenate(quads, axis=0), offs, want, want_offs


def many_quads(n, seed):
    """one page (450 x 700 -> 600 x 933) of n quads at fractional positions, points in every order, some tied in x, some outside; none with
    xmin == xmax is left to chance: the restatement gives no strip there, as the header defines"""
    rs = np.random.RandomState(seed)
    x0, y0 = rs.uniform(-30, 690, n), rs.uniform(-20, 440, n)
    bw, bh = rs.uniform(1, 200, n), rs.uniform(4, 40, n)
    q = np.stack([x0, y0, x0 + bw, y0 + rs.uniform(-4, 4, n), x0 + bw + rs.uniform(-4, 4, n), y0 + bh, x0 + rs.uniform(-4, 4, n), y0 + bh], axis=1).reshape(n, 4, 2)
    q = np.round(q * 4) / 4
    tie = rs.rand(n) < 0.3
    q[tie, 2, 0] = q[tie, 1, 0]
    for i in range(n):
        q[i] = q[i][rs.permutation(4)]
    return np.array([[450, 700, 600, 933]], np.int32), q.reshape(n, 8), np.array([0, n], np.int32)


def big_label_set(golden):
    """the fixture's first page, a page with 0 quads, then a page of 301 quads -- more than one 256-thread workgroup, strips past one
    2048-wide scan run -- whose last quad is degenerate (xmin == xmax: no strip)"""
    dims, quads, offs, _, _ = label_set(golden)
    d1, q1, _ = many_quads(300, 7)
    dims2 = np.concatenate([dims[:1], dims[1:2], d1], axis=0)
    quads2 = np.concatenate([quads[: offs[1]], q1, [[7, 5, 7, 9, 7, 30, 7, 40]]], axis=0)
    offs2 = np.array([0, offs[1], offs[1], offs[1] + 301], np.int32)
    return dims2, quads2, offs2
