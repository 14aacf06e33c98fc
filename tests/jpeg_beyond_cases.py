"""JPEG files whose dequantised coefficients leave the range a forward DCT of 8-bit pixels can produce: the cases of tests/test_jpeg.py,
tests/test_jpeg_ragged.py and their GPU twins for the IDCT's 16-bit arithmetic (csrc/jpeg_pixel.h; oracle/jpeg_ref.py idct_islow).

Every file is valid baseline / extended / progressive JPEG, the parser takes it and Pillow decodes it without a warning. Out of range the
pin is libjpeg-turbo's x86 SIMD code, so the committed vectors (tests/golden/jpeg_beyond_cases.npz, oracle/make_jpeg_beyond_golden.py) carry
Pillow's pixels; the CPU tests also ask the Pillow installed where they run.

Families (cases() -> {name: Case}; the name's first letter is the family):
  a  Pillow's own files (40 x 56 scene; 4:4:4, 4:2:2, 4:2:0, gray; sequential and progressive) and one 4:4:0 file of util_jpeg's encoder,
     with the DQT entries rewritten: x 8, x 16, all 64, all 255 (with_dqt; saturating at 255).
  b  Coefficient-level files (encode_coefficients), gray: flat blocks with |DC x q| on both sides of 8192 and of 32768 (the whole-block
     shortcut wraps row 0 << 2 to 16 bits where the general path would saturate), blocks whose only AC lies in row 0 (shortcut) or in
     column 0 (general path), and a 35-block file mixing all three kinds inside one workgroup of 32 blocks.
  c  One coefficient per block, at each of the 64 positions in turn (4:4:4, 72 blocks): products +-32767, +-32768, +-40000 (the 16-bit
     wrap of coef x q), +-8192 (row 0 << 2 wraps) and 8176 (inside for rows 0 and 4; elsewhere pass 1 saturates, and where it saturates
     column 4 at -32768, pass 2's in0 - in4 = 32768 wraps). A lone coefficient fills one workspace column, so pass 1's saturation alone cannot
     change a pixel (pass 2 saturates the same sample anyway); c-pass1-saturation-edge therefore pairs the coefficient under test at
     (row r, column 0) -- the smallest product whose pass-1 result passes 32767 and the one below it, both signs, r = 1 .. 7 -- with a
     slightly smaller partner at (r, 4), so that pass 2's in0 - in4 shows the saturated value at full resolution.
     Controls (in range at every position: both arithmetics give one picture): c-p5904-control, c-m5904-control.
  d  16-bit tables (Pq = 1 under an SOF1 frame), flat: 256, 4096, 32768, 65535, each against coefficients +-1, +-2, +-1023 at the DC, a
     row-0 and an inner position; 1023 x 65535 is the largest AC product the Huffman tables of the writer reach (int16 x uint16 stays
     inside 31 bits whatever the file holds). Control: d-q256-control (coefficients +-1, +-2 only).
  e  Layouts: the b, c and d patterns spread over all three planes of 4:2:0, 4:2:2 and 4:4:0 files, EXIF orientations (a turned Pillow
     file, a turned coefficient file), restart intervals (Pillow's and the coefficient writer's).
Nothing was left out: Pillow and the library's parser take every family, Pq = 1 under SOF1 included.
"""
import functools
from collections import namedtuple

import numpy as np

from util_jpeg import encode, encode_coefficients, encode_custom, scene, with_dqt, with_exif_orientation

Case = namedtuple("Case", "data control")

# the in-range controls: exempt from "the full-width arithmetic must differ from Pillow somewhere"; at most a quarter of the table
CONTROLS = ("c-p5904-control", "c-m5904-control", "d-q256-control")

_DQT_OPS = {"x8": lambda v: v * 8, "x16": lambda v: v * 16, "all64": lambda v: 64, "all255": lambda v: 255}


def _one(pos, v, dc=0):
    b = np.zeros(64, np.int64)
    b[0] = dc
    b[pos] = v
    return b


def _shapes(h, w, hs, vs, gray):
    """block grid (rows, columns) of every component: whole MCUs"""
    if gray:
        return [(-(-h // 8), -(-w // 8))]
    my, mx = -(-h // (8 * vs)), -(-w // (8 * hs))
    return [(my * vs, mx * hs), (my, mx), (my, mx)]


def _spread(protos, h, w, hs=1, vs=1, gray=False, skip=0):
    """The prototype blocks, cycled (from number `skip` on), over every block of every component in component order."""
    out, n = [], skip
    for (bh, bw) in _shapes(h, w, hs, vs, gray):
        a = np.zeros((bh, bw, 64), np.int64)
        for i in range(bh * bw):
            a[i // bw, i % bw] = protos[n % len(protos)]
            n += 1
        out.append(a)
    return out


def _file(protos, q, h, w, hs=1, vs=1, gray=False, pq=0, restart=0, skip=0):
    blocks = _spread(protos, h, w, hs, vs, gray, skip)
    return encode_coefficients(blocks, [np.full(64, q) if np.isscalar(q) else q] * len(blocks), h, w, hs, vs, pq=pq, restart=restart)


# ---- family b: q = 64 everywhere
def _flat_protos():
    return [_one(0, dc) for dc in (127, 128, 129, -128, -129, 511, 512, 513, -512, -513)]      # x 64: 8128 8192 8256 ... 32704 32768 32832


def _row0_protos():
    return [_one(1 + k % 7, v, dc) for k, (v, dc) in enumerate([(127, 0), (128, 0), (-128, 3), (-129, 0), (512, -5), (-512, 0), (640, 0), (1023, 9)])]


def _col0_protos():
    return [_one(8 * (1 + k % 7), v, dc) for k, (v, dc) in enumerate([(127, 0), (128, 0), (-128, 3), (-129, 0), (512, -5), (-512, 0), (640, 0), (1023, 9)])]


def _mixed_protos():
    f, r, c = _flat_protos(), _row0_protos(), _col0_protos()
    return [x for k in range(10) for x in (f[k], r[k % 8], c[k % 8])]


# ---- family c
def _single_protos(v):
    return [_one(p, v) for p in range(64)]


_GAIN = (8192, 11363, 10703, 11362, 8192, 11362, 10704, 11363)      # largest |pass-1 output| per unit of a coefficient in row r, x 2^11


def _saturation_edge_protos(q=16):
    out = []
    for r in range(1, 8):
        c = next(c for c in range(1, 1024) if (c * q * _GAIN[r] + 1024) >> 11 > 32767)      # the smallest coefficient whose result passes 32767
        for v in (c - 1, c, -(c - 1), -c):
            b = np.zeros(64, np.int64)
            b[8 * r], b[8 * r + 4] = v, v - 3 if v > 0 else v + 3
            out.append(b)
    return out


# ---- family d
def _d_protos(values=(1, -1, 2, -2, 1023, -1023)):
    return [_one(p, v) for p in (0, 3, 17) for v in values]


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case(data, control)}, in a fixed order."""
    t = {}
    # a
    k = 0
    for lay, (sub, gray) in (("444", (0, False)), ("422", (1, False)), ("420", (2, False)), ("gray", (2, True))):
        for op in ("x8", "x16", "all64", "all255"):
            prog = bool(k & 1) ^ bool(k & 4)
            quality = 95 if op in ("x8", "all64") else 75
            t["a-%s-%s-%s" % (lay, "progressive" if prog else "sequential", op)] = with_dqt(encode(scene(40, 56, 3, gray), quality, sub, progressive=prog), _DQT_OPS[op])
            k += 1
    t["a-440-x16"] = with_dqt(encode_custom(scene(40, 56, 3), 1, 2, q=8), _DQT_OPS["x16"])
    # b
    t["b-flat-dc-edges"] = _file(_flat_protos(), 64, 16, 40, gray=True)
    t["b-row0-ac"] = _file(_row0_protos(), 64, 16, 32, gray=True)
    t["b-col0-ac"] = _file(_col0_protos(), 64, 16, 32, gray=True)
    t["b-mixed-one-workgroup"] = _file(_mixed_protos(), 64, 40, 56, gray=True)
    # c
    for name, v, q in (("p32767", 217, 151), ("m32767", -217, 151), ("p32768", 256, 128), ("m32768", -256, 128), ("p40000", 160, 250), ("m40000", -160, 250),
                       ("p8192", 512, 16), ("m8192", -512, 16), ("p5904-control", 369, 16), ("m5904-control", -369, 16), ("p8176", 511, 16)):
        t["c-" + name] = _file(_single_protos(v), q, 32, 48)
    t["c-pass1-saturation-edge"] = _file(_saturation_edge_protos(), 16, 32, 56, gray=True)
    # d
    for q in (256, 4096, 32768, 65535):
        t["d-q%d" % q] = _file(_d_protos(), q, 24, 48, gray=True, pq=1)
    t["d-q256-control"] = _file(_d_protos((1, -1, 2, -2, 1, -2)), 256, 24, 48, gray=True, pq=1)
    # e
    for lay, (hs, vs) in (("420", (2, 2)), ("422", (2, 1)), ("440", (1, 2))):
        t["e-b-mixed-" + lay] = _file(_mixed_protos(), 64, 32, 32, hs, vs)
        t["e-c-p32768-" + lay] = _file(_single_protos(256), 128, 32, 32, hs, vs, skip=40)
        t["e-d-q65535-" + lay] = _file(_d_protos(), 65535, 32, 32, hs, vs, pq=1)
    t["e-c-m40000-420"] = _file(_single_protos(-160), 250, 32, 32, 2, 2)
    t["e-d-q4096-440"] = _file(_d_protos(), 4096, 32, 32, 1, 2, pq=1, skip=5)
    t["e-c-saturation-edge-422"] = _file(_saturation_edge_protos(), 16, 32, 32, 2, 1)
    t["e-a-420-x16-orientation6"] = with_exif_orientation(t["a-420-progressive-x16"], 6)
    t["e-b-mixed-422-orientation5"] = with_exif_orientation(_file(_mixed_protos(), 64, 32, 24, 2, 1, skip=7), 5)      # stored 32 x 24, shown 24 x 32
    t["e-b-mixed-420-restart2"] = _file(_mixed_protos(), 64, 32, 32, 2, 2, restart=2, skip=3)
    t["e-a-444-all255-restart3"] = with_dqt(encode(scene(40, 56, 4), 75, 0, restart_marker_blocks=3), _DQT_OPS["all255"])
    assert set(CONTROLS) <= set(t) and 4 * len(CONTROLS) <= len(t)
    return {k: Case(v, k in CONTROLS) for k, v in t.items()}


# one ragged call's worth (tests/test_jpeg_ragged.py, tests/test_gpu_jpeg_ragged.py): five layouts, three heights, one shown width, factor 1
RAGGED = ("e-b-mixed-420", "b-row0-ac", "e-d-q65535-440", "e-b-mixed-422-orientation5", "e-c-p32768-422")
RAGGED_HC, RAGGED_WC = 32, 32


def family(letter):
    return {k: c for k, c in cases().items() if k[0] == letter}
