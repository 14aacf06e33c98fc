"""The PNG writer's file definition restated in plain Python for tests/test_png_encode.py and tests/test_gpu_png_encode.py: the filtered
stream (Sub on every row, RGB order) and the tokeniser's RULE -- pieces of 256 bytes, greedy, two candidates per position -- and nothing of
the Huffman construction. Also the image set both test files use: the smallest shapes at which the writer can go wrong."""
import io
import os

import numpy as np

P = 256


def filtered(bgr):
    """h * (1 + 3 w) bytes: per row the filter type 1 and raw[x] - raw[x - 3] (raw[x] for x < 3), raw = the row's pixels in RGB order"""
    h, w, _ = bgr.shape
    rgb = np.ascontiguousarray(bgr[:, :, ::-1]).reshape(h, 3 * w).astype(np.uint8)
    f = rgb.copy()
    f[:, 3:] = rgb[:, 3:] - rgb[:, :-3]
    return np.concatenate([np.full((h, 1), 1, np.uint8), f], 1).reshape(-1)


def tokenise(s, stride, far=True):
    """-> dict(lit, near, far, covered, l2_gt, l1_gt, tie): literal count, matches by distance (1 / stride), the bytes the tokens cover,
    and how often a match was chosen with L2 > L1, L1 > L2, L1 = L2. far=False: matches at distance stride disabled (the size test)"""
    s = bytes(s)
    n = len(s)
    far = far and stride <= 32768
    out = dict(lit=0, near=0, far=0, covered=0, l2_gt=0, l1_gt=0, tie=0, lengths=[])
    for p0 in range(0, n, P):
        p1 = min(p0 + P, n)
        i = p0
        while i < p1:
            l1 = 0
            if i >= 1:
                b = s[i - 1]
                while i + l1 < p1 and l1 < 258 and s[i + l1] == b:
                    l1 += 1
            l2 = 0
            if far and i >= stride:
                while i + l2 < p1 and l2 < 258 and s[i + l2] == s[i + l2 - stride]:
                    l2 += 1
            L = max(l1, l2)
            if L >= 3:
                out["near" if l1 >= l2 else "far"] += 1
                out["l2_gt" if l2 > l1 else ("l1_gt" if l1 > l2 else "tie")] += 1
                out["lengths"].append(L)
                out["covered"] += L
                i += L
            else:
                out["lit"] += 1
                out["covered"] += 1
                i += 1
    return out


def document_page(h=300, w=450, seed=0):
    """light paper with rows of dark glyph boxes (the structure of a scan: long runs, rows that repeat the row above)"""
    rng = np.random.default_rng(seed)
    doc = np.full((h, w, 3), 245, np.uint8)
    for r in range(h // 15, h - 20, 24):
        for c in range(w // 22, w - 20, 9):
            if rng.random() < 0.8:
                doc[r:r + 14, c:c + 6] = rng.integers(0, 80)
    return doc


def flat(h, w, v=7):
    return np.full((h, w, 3), v, np.uint8)


def repeated_rows():
    """rows that repeat the row above, with the change placed so that all three outcomes of max(L1, L2) occur"""
    rng = np.random.default_rng(5)
    im = np.zeros((8, 100, 3), np.uint8)
    im[0] = rng.integers(0, 256, (100, 3), dtype=np.uint8)      # noise
    im[1] = im[0]                                               # the row above, no runs: L2 > L1
    im[2] = 90                                                  # flat under noise: L1 > L2
    im[3] = 90                                                  # flat under flat: L1 = L2
    im[4] = 90
    im[4, 50:] = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    im[5] = im[4]
    im[5, 20] = (1, 2, 3)                                       # a change inside a run
    im[6] = im[5]
    im[6, 70] = (9, 9, 9)                                       # ... and inside the noise
    im[7] = im[6]
    return im


def _demo_crops():
    from PIL import Image
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo_files.npz"))
    out = {}
    for name in g["names"]:
        key = str(name).replace(".", "_")
        im = np.asarray(Image.open(io.BytesIO(g["file_" + key].tobytes())).convert("RGB"))[:, :, ::-1]
        out["demo-" + key] = np.ascontiguousarray(im[:250, :300])
    return out


_CACHE = {}


def images():
    """name -> (h, w, 3) BGR uint8; computed once"""
    if _CACHE:
        return _CACHE
    rng = np.random.default_rng(11)
    few = lambda h, w: rng.integers(0, 3, (h, w, 3), dtype=np.uint8)      # few values: literals, short runs and matches mixed
    s = _CACHE
    s["1x1"] = np.array([[[1, 2, 3]]], np.uint8)
    s["1x700"] = few(1, 700)
    s["700x1"] = few(700, 1)
    for w in (84, 85, 86):                                                # stride 256 at 85: pieces aligned to rows, one off either side
        s["9x%d" % w] = few(9, w)
        s["9x%d-page" % w] = np.ascontiguousarray(document_page(40, 450, seed=w)[10:19, :w])
    # a stream of 255 / 256 bytes, and the first sizes behind 256 that exist: h (1 + 3 w) = 257 has no solution (257 is prime and
    # 1 + 3 w = 257 has none), so 258 and 259 (= 1 x 86) stand for "one piece and a little"
    s["n255-3x28"] = few(3, 28)
    s["n256-1x85"] = few(1, 85)
    s["n256-64x1"] = few(64, 1)
    s["n258-6x14"] = few(6, 14)
    s["n259-1x86"] = few(1, 86)
    s["flat-40x700"] = flat(40, 700)                                      # runs cut at piece ends, many pieces per word
    s["repeated-rows"] = repeated_rows()
    s["noise-64x96"] = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)  # no match, literals at their longest
    s["2x10922"] = np.repeat(few(1, 10922), 2, axis=0)                    # stride 32767: the far distance at its limit, used over a whole row
    s["2x10923"] = np.repeat(few(1, 10923), 2, axis=0)                    # stride 32770: distance 1 only, S = the dummy
    s.update(_demo_crops())
    s["page-300x450"] = document_page()
    for h in (1023, 1024, 1025):                                          # one piece per row: the scan kernel's step of 1024 pieces, one off either side
        s["scan-%dx85" % h] = few(h, 85)
    return s


def stream_bytes(h, w):
    return h * (1 + 3 * w)
