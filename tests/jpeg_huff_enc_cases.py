"""Shared by tests/test_jpeg_huff_enc_host.py (CPU) and tests/test_gpu_jpeg_huff_enc.py: the coefficient sets the device Huffman coder is
tested on -- the smallest that can go wrong -- in the form ctpn_jpeg_entropy_encode takes them (natural order, the eight layout ints, the
3 x 64 tables). Expected bytes never come from here: they are ctpn_jpeg_entropy_encode's (host_file). What is restated here is only what
it takes to BUILD a case: the scan order of the blocks, and the bit count of a stream (to find totals with a given remainder)."""
import ctypes as C

import numpy as np

from ctpn_amd import _binding as B
import jpeg_huff_cases as H

SCAN_ITEMS = 1024      # csrc/jpeg_huff_enc_dev.h JHE_SCAN_ITEMS: items one workgroup of the prefix sum takes per step
HEADER_BYTES = 623     # SOI .. SOS of the files this library writes


def zigzag_order():
    """natural index of the k-th coefficient of the zig-zag sequence, from the walk itself (ITU-T T.81 figure 5)"""
    order, (y, x), up = [], (0, 0), True
    for _ in range(64):
        order.append(8 * y + x)
        if up:
            if x == 7:
                y, up = y + 1, False
            elif y == 0:
                x, up = x + 1, False
            else:
                y, x = y - 1, x + 1
        else:
            if y == 7:
                x, up = x + 1, True
            elif x == 0:
                y, up = y + 1, True
            else:
                y, x = y + 1, x - 1
    return np.array(order)


ZZ = zigzag_order()


def grid(h, w, hs, vs):
    return -(-w // (8 * hs)), -(-h // (8 * vs))


def block_count(h, w, hs, vs):
    mcux, mcuy = grid(h, w, hs, vs)
    return mcux * mcuy * (hs * vs + 2)


def scan_slots(h, w, hs, vs):
    """index, in the [component][block rows][block columns] layout, of every block in scan order: MCU by MCU, the luma blocks of the MCU
    row-major, then Cb, then Cr"""
    mcux, mcuy = grid(h, w, hs, vs)
    base = [0, mcux * mcuy * hs * vs, mcux * mcuy * (hs * vs + 1)]
    out = []
    for my in range(mcuy):
        for mx in range(mcux):
            for by in range(vs):
                for bx in range(hs):
                    out.append(base[0] + (my * vs + by) * (mcux * hs) + mx * hs + bx)
            out.append(base[1] + my * mcux + mx)
            out.append(base[2] + my * mcux + mx)
    return np.array(out)


def case(h, w, hs, vs, scan_blocks_zz):
    """scan_blocks_zz: (blocks, 64) values in ZIG-ZAG order, blocks in SCAN order (missing ones are zero) -> (coef natural, layout8, qt)"""
    n = block_count(h, w, hs, vs)
    blk = np.zeros((n, 64), np.int16)
    src = np.asarray(scan_blocks_zz, np.int16).reshape(-1, 64)
    assert src.shape[0] <= n
    blk[: src.shape[0]] = src
    nat = np.zeros_like(blk)
    nat[:, ZZ] = blk
    lay = np.zeros_like(nat)
    lay[scan_slots(h, w, hs, vs)] = nat
    mcux, mcuy = grid(h, w, hs, vs)
    layout = np.array([h, w, 3, hs, mcux * hs, mcux, mcuy * vs, mcuy], np.int32)
    return lay.reshape(-1), layout, np.ones((3, 64), np.uint16)


def sparse_blocks(n, seed, density=0.15, dc=200, big=0.1):
    """n blocks (zig-zag): DC within +-dc, AC non-zero with probability `density`, a share `big` of them up to +-1023"""
    rng = np.random.default_rng(seed)
    small = rng.integers(-7, 8, (n, 64))
    large = rng.integers(-1023, 1024, (n, 64))
    v = np.where(rng.random((n, 64)) < big, large, small) * (rng.random((n, 64)) < density)
    v[:, 0] = rng.integers(-dc, dc + 1, n)
    return v.astype(np.int16)


def block(dc=0, **at):
    """one block in zig-zag order: block(5, k1=3, k63=-1)"""
    b = np.zeros(64, np.int16)
    b[0] = dc
    for k, v in at.items():
        b[int(k[1:])] = v
    return b


def host_file(c):
    """(status, bytes or None, message) of ctpn_jpeg_entropy_encode for the case"""
    lib = B.load_library()
    coef, l8, qt = (np.ascontiguousarray(a) for a in c)
    args = (B._ptr(coef, C.c_int16), B._ptr(l8, C.c_int), B._ptr(qt.reshape(-1), C.c_uint16))
    n = C.c_size_t(0)
    rc = lib.ctpn_jpeg_entropy_encode(*args, None, 0, C.byref(n))
    if rc != B.CTPN_ERR_CAPACITY:
        return rc, None, lib.ctpn_last_error().decode()
    out = np.zeros(n.value, np.uint8)
    rc = lib.ctpn_jpeg_entropy_encode(*args, B._ptr(out, C.c_uint8), out.size, C.byref(n))
    assert rc == 0 and n.value == out.size
    return 0, out.tobytes(), ""


def unstuffed_bits(data):
    """bits of a file's scan body before the padding, counted from the file itself: its DHT segments give the code lengths, the decoder of
    tests/jpeg_huff_cases.py the frame; the coefficients are the host half's. Used to FIND cases, never as an expected value."""
    f = H.parse(data)
    lens = {}
    for key, (counts, vals) in f["dht"].items():
        k = 0
        for l in range(1, 17):
            for _ in range(counts[l - 1]):
                lens[(key, vals[k])] = l
                k += 1
    coef = entropy_decode(data)[0].reshape(-1, 64)
    hs, vs = f["hs"][0], f["vs"][0]
    slots = scan_slots(f["h"], f["w"], hs, vs)
    bpm, bits, pred = hs * vs + 2, 0, [0, 0, 0]
    for s, slot in enumerate(slots):
        j = s % bpm
        c = 0 if j < hs * vs else j - hs * vs + 1
        blk = coef[slot][ZZ]
        d = int(blk[0]) - pred[c]
        pred[c] = int(blk[0])
        t = abs(d).bit_length()
        bits += lens[((0, f["td"][c]), t)] + t
        run = 0
        for v in blk[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                bits += lens[((1, f["ta"][c]), 0xF0)]
                run -= 16
            t = abs(int(v)).bit_length()
            bits += lens[((1, f["ta"][c]), (run << 4) | t)] + t
            run = 0
        if run:
            bits += lens[((1, f["ta"][c]), 0)]
    return bits


def entropy_decode(data):
    """(coef natural, qt, layout8) of ctpn_jpeg_entropy_decode, the coefficient array cut to the frame"""
    lib = B.load_library()
    h, w = B.jpeg_probe(data)[:2]
    cap = int(lib.ctpn_jpeg_coef_capacity(h, w))
    coef, qt, l8 = np.zeros(cap, np.int16), np.zeros((3, 64), np.uint16), np.zeros(8, np.int32)
    keep, ptr, n = B._bytes_ptr(data)
    B._check(lib.ctpn_jpeg_entropy_decode(ptr, n, B._ptr(coef, C.c_int16), cap, B._ptr(qt.reshape(-1), C.c_uint16), B._ptr(l8, C.c_int)))
    return coef[: (int(l8[4]) * int(l8[6]) + 2 * int(l8[5]) * int(l8[7])) * 64], qt, l8


def _find(make, want, what):
    """the first k in 1 .. 1023 for which the host's file of make(k) has the property"""
    for k in range(1, 1024):
        c = make(k)
        st, data, _ = host_file(c)
        if st == 0 and want(data):
            return c
    raise AssertionError("no case found: " + what)


_CACHE = {}


def cases():
    """name -> (coef, layout8, qt). OUT_OF_RANGE names the two whose flag must be raised."""
    if _CACHE:
        return _CACHE
    out = _CACHE
    # tiny and edge sizes: one MCU whose luma blocks are mostly dummies in a real file; partial, whole and one-more MCUs
    out["1x1-420"] = case(1, 1, 2, 2, sparse_blocks(6, 1))
    for h in (15, 16, 17):
        for w in (15, 16, 17):
            out["%dx%d-420" % (h, w)] = case(h, w, 2, 2, sparse_blocks(block_count(h, w, 2, 2), 100 + 31 * h + w))
    # zero and non-zero patterns
    out["all-zero"] = case(16, 16, 2, 2, [])
    out["only-ac63"] = case(8, 8, 1, 1, [block(3, k63=5), block(0, k63=-1), block(-2, k63=1023)])
    out["zero-runs"] = case(8, 24, 1, 1, [block(1, **{"k%d" % (r + 1): 2, "k63": -3}) for r in (15, 16, 31, 32, 48)] + [block(0, k16=1), block(0, k17=1), block(0, k49=1)])
    full = np.array([1023 if k % 2 else -1023 for k in range(64)], np.int16)
    mx = []
    for m in range(4):      # per MCU Y, Cb, Cr: the DC alternates between 1023 and -1024 (differences of 1023, then -2047 / +2047)
        b = full.copy()
        b[0] = 1023 if m % 2 == 0 else -1024
        mx += [b, b, b]
    out["max-block"] = case(8, 32, 1, 1, mx)
    # 0xFF production: positive values 2^k - 1 behind 16-bit codes (every 16-bit code of K.5 / K.6 starts with nine 1-bits)
    ff = []
    for m in range(6):
        b = np.zeros(64, np.int16)
        b[0] = 255 if m % 2 == 0 else 0
        for k in range(2, 64, 2):
            b[k] = (1 << (1 + (k + m) % 10)) - 1      # run 1, sizes 1 .. 10
        ff.append(b)
    out["ff-runs"] = case(8, 16, 1, 1, ff)
    out["ff-dense"] = case(16, 16, 2, 2, np.concatenate([np.zeros((6, 1), np.int16), np.full((6, 63), 1023, np.int16)], 1))
    pad = lambda k: case(8, 8, 1, 1, [block(k, k1=k, k2=1023, k5=255, k63=1), block(k, k1=1), block(-k, k3=k, k63=1023)])
    out["last-byte-ff"] = _find(pad, lambda d: d[-4:] == b"\xff\x00\xff\xd9" and unstuffed_bits(d) % 8 != 0, "a padded last byte of 0xFF")
    out["no-padding"] = _find(pad, lambda d: unstuffed_bits(d) % 8 == 0, "a whole number of bytes")
    # scan boundaries: exactly what one workgroup of the prefix sum takes per step, the smallest counts behind it (a block count is
    # a multiple of 3, 4 or 6 and 1025 is none: 1026 = 171 MCUs of 4:2:0, 1028 = 257 MCUs of 4:2:2), and a count that ends mid-MCU in a step
    assert block_count(128, 256, 2, 1) == SCAN_ITEMS and block_count(8, 4112, 2, 1) == SCAN_ITEMS + 4 and block_count(256, 272, 2, 2) == 1632
    assert block_count(16, 2736, 2, 2) == SCAN_ITEMS + 2
    out["scan-exact-422"] = case(128, 256, 2, 1, sparse_blocks(SCAN_ITEMS, 11))
    out["scan-plus-two-420"] = case(16, 2736, 2, 2, sparse_blocks(SCAN_ITEMS + 2, 14))
    out["scan-plus-one-mcu-422"] = case(8, 4112, 2, 1, sparse_blocks(SCAN_ITEMS + 4, 12))
    out["256x272-dense-420"] = case(256, 272, 2, 2, sparse_blocks(1632, 13, 0.9, 1000, 0.5))      # > 64 KB of stream: several steps of the chunk sum too
    # the four layouts
    for name, (hs, vs) in (("444", (1, 1)), ("422", (2, 1)), ("440", (1, 2)), ("420", (2, 2))):
        out["33x47-" + name] = case(33, 47, hs, vs, sparse_blocks(block_count(33, 47, hs, vs), 20 + hs + 2 * vs, 0.3))
    # real files: the three-component files of the decoder's cases, as the host half decodes them
    for name, data in H.cases().items():
        if H.parse(data)["ncomp"] == 3:
            coef, qt, l8 = entropy_decode(data)
            out["file-" + name] = (coef, l8, qt)
    # outside what baseline JPEG codes: the flag must be raised and the host half's verdict returned
    out["dc-diff-2048"] = case(8, 16, 1, 1, [block(1024), block(0), block(0), block(-1024)])
    out["ac-1024"] = case(8, 8, 1, 1, [block(0, k7=1024)])
    return out


OUT_OF_RANGE = ("dc-diff-2048", "ac-1024")
