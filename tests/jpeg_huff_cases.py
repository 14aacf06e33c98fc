"""Shared by tests/test_jpeg_huff_host.py (CPU) and tests/test_gpu_jpeg_huff.py: the files the device Huffman decoder is tested on, the
damaged variants of them, and a bytewise restatement of what the library's host side does to a scan (marker walk, byte unstuffing, restart
segments). Expected coefficients never come from here: they are ctpn_jpeg_entropy_decode's."""
import numpy as np

from util_jpeg import encode, encode_custom, scene


def noise(h, w, seed, gray=False):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if gray else (h, w, 3), dtype=np.uint8)


def cases():
    """name -> bytes. Scans shorter than one subsequence, blocks longer than one (noise at quality 100: up to 1660 bits), many FF bytes to
    unstuff, codes longer than 9 bits, hundreds of blocks per subsequence (flat, quality 20), optimised tables, restart intervals of one
    MCU, of one MCU row and of 5 MCUs on a 7-MCU-wide image (a short last interval), sizes that are no multiple of the MCU."""
    out = {"8x8-flat-gray": encode(np.full((8, 8), 77, np.uint8), 90)}
    for q in (100, 95):
        n3, n1 = noise(64, 48, q), noise(64, 48, q + 1, gray=True)
        out["64x48-noise-q%d-gray" % q] = encode(n1, q)
        out["64x48-noise-q%d-444" % q] = encode(n3, q, 0)
        out["64x48-noise-q%d-420" % q] = encode(n3, q, 2)
        out["64x48-noise-q%d-422" % q] = encode(n3, q, 1)
        out["64x48-noise-q%d-440" % q] = encode_custom(n3, 1, 2, q=1 if q == 100 else 2)      # (its three components share one table pair)
    out["96x64-flat-q20"] = encode(np.full((96, 64, 3), (90, 140, 200), np.uint8), 20, 2)
    out["50x70-q30-420-optimize"] = encode(scene(50, 70, 11), 30, 2, optimize=True)
    out["64x48-noise-q95-444-optimize"] = encode(noise(64, 48, 3), 95, 0, optimize=True)
    out["45x61-q85-420-restart-1mcu"] = encode(scene(45, 61, 12), 85, 2, restart_marker_blocks=1)
    out["45x61-q85-444-restart-row"] = encode(scene(45, 61, 13), 85, 0, restart_marker_rows=1)
    out["32x112-q90-420-restart-5-of-7"] = encode(scene(32, 112, 14), 90, 2, restart_marker_blocks=5)
    out["37x53-440-restart2"] = encode_custom(scene(37, 53, 2), 1, 2, q=10, restart=2)
    out["1x1-q90-420"] = encode(scene(1, 1, 15), 90, 2)
    out["17x9-q90-420"] = encode(scene(17, 9, 16), 90, 2)
    out["33x47-q95-444"] = encode(scene(33, 47, 17), 95, 0)
    return out


def parse(data):
    """The frame of a sequential file, read bytewise the way the library's parser walks the markers: dict(ncomp, h, w, hs, vs, td, ta, dri,
    dht={(class, id): (counts, vals)}, scan=offset of the entropy-coded data), or None if the headers do not get that far."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    i, f, dht, dri = 2, None, {}, 0
    while i + 4 <= len(data):
        if data[i] != 0xFF:
            return None
        m = data[i + 1]
        i += 2
        if m == 0xFF:
            i -= 1
            continue
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            return None
        L = (data[i] << 8) | data[i + 1]
        if L < 2 or i + L > len(data):
            return None
        s = data[i + 2: i + L]
        i += L
        if m == 0xC4:
            j = 0
            while j + 17 <= len(s):
                counts = list(s[j + 1: j + 17])
                nv = sum(counts)
                dht[(s[j] >> 4, s[j] & 15)] = (counts, list(s[j + 17: j + 17 + nv]))
                j += 17 + nv
        elif m == 0xDD:
            dri = (s[0] << 8) | s[1]
        elif m in (0xC0, 0xC1):
            nc = s[5]
            f = {"h": (s[1] << 8) | s[2], "w": (s[3] << 8) | s[4], "ncomp": nc, "hs": [s[7 + 3 * k] >> 4 for k in range(nc)], "vs": [s[7 + 3 * k] & 15 for k in range(nc)]}
        elif m == 0xC2:
            return None
        elif m == 0xDA:
            if f is None or s[0] != f["ncomp"]:
                return None
            f["td"] = [s[2 + 2 * k] >> 4 for k in range(f["ncomp"])]
            f["ta"] = [s[2 + 2 * k] & 15 for k in range(f["ncomp"])]
            if f["ncomp"] == 1:
                f["hs"], f["vs"] = [1], [1]
            f["mcux"] = -(-f["w"] // (8 * f["hs"][0]))
            f["mcuy"] = -(-f["h"] // (8 * f["vs"][0]))
            f["dri"], f["dht"], f["scan"] = dri, dht, i
            return f
    return None


def unstuff_segments(scan, dri, total_mcus):
    """The one pass the host may make over a scan's bytes, restated bytewise: FF 00 -> FF, stop at the first marker that is not RSTn (at any
    marker without a restart interval, and at a lone FF that ends the file), cut at every RSTn; at most the segments the frame needs.
    Returns (bytes, [(first byte, bits, first MCU, MCUs)])."""
    need = -(-total_mcus // dri) if dri else 1
    out, segs, start, i = bytearray(), [], 0, 0

    def close():
        nonlocal start
        m0 = len(segs) * dri if dri else 0
        segs.append((start, (len(out) - start) * 8, m0, min(dri, total_mcus - m0) if dri else total_mcus))
        start = len(out)
    while i < len(scan) and len(segs) < need:
        b = scan[i]
        if b != 0xFF:
            out.append(b)
            i += 1
        elif i + 1 >= len(scan):
            break
        elif scan[i + 1] == 0:
            out.append(0xFF)
            i += 2
        elif dri and 0xD0 <= scan[i + 1] <= 0xD7:
            close()
            i += 2
        else:
            break
    if len(segs) < need:
        close()
    return bytes(out), segs


def damaged(data, flips=200, seed=0):
    """[(label, bytes)]: the file truncated at 40 % and at 90 % of its length, and with `flips` seeded single-bit flips inside its scan."""
    out = [("cut40", data[: len(data) * 4 // 10]), ("cut90", data[: len(data) * 9 // 10])]
    f = parse(data)
    lo, hi = f["scan"], len(data) - 2          # (the EOI marker stays)
    rng = np.random.default_rng(seed)
    for k in range(flips):
        pos = int(rng.integers(lo * 8, hi * 8))
        b = bytearray(data)
        b[pos >> 3] ^= 0x80 >> (pos & 7)
        out.append(("flip%d@%d" % (k, pos), bytes(b)))
    return out


# the two damaged files that also run on the GPU (tests/test_gpu_jpeg_huff.py), by name: tests/test_jpeg_huff_host.py runs the sanitised
# emulation on exactly these bytes
GPU_TRUNCATED = ("64x48-noise-q95-420", "cut90")


def gpu_damaged_files():
    """(truncated file, file with an invalid code): the first is GPU_TRUNCATED; the second is 64x48-noise-q95-444 with sixty-four 1-bits
    written over the start of its scan's second half: a code and its value bits take 31 of them at most, the next code then starts inside the
    run and finds sixteen 1-bits -- no code of a JPEG table is all ones."""
    c = cases()
    cut = dict(damaged(c[GPU_TRUNCATED[0]], flips=0))[GPU_TRUNCATED[1]]
    d = c["64x48-noise-q95-444"]
    at = (parse(d)["scan"] + len(d)) // 2
    bad = bytearray(d)
    bad[at: at + 16] = b"\xff\x00" * 8          # (FF 00 is a stuffed FF)
    return cut, bytes(bad)
