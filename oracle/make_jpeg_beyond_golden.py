"""Generates tests/golden/jpeg_beyond_cases.npz: the files of tests/jpeg_beyond_cases.py (bytes) and Pillow's decode of each, turned by the
EXIF orientation, in cv2.imread's channel order.

    python -m oracle.make_jpeg_beyond_golden          (from the repo root, in the build container)

These files carry dequantised coefficients beyond what a forward DCT of 8-bit pixels produces. There libjpeg-turbo's answer belongs to its
x86 SIMD islow IDCT (16-bit lanes); a build that runs without SIMD follows jidctint.c's masked range-limit table and gives other pixels. So
for these cases the committed vectors ARE the pin: they must be made where Pillow's libjpeg-turbo runs with SIMD (x86-64, JSIMD_FORCENONE
unset), which the recipe checks through a file whose picture tells the two apart. Made from Pillow alone; nothing of the reference tree.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def main():
    import PIL
    from PIL import features
    import jpeg_beyond_cases as BC
    from oracle import jpeg_ref as J
    from util_jpeg import cv2_like_bgr
    out, names = {}, []
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # every file is meant to be valid: a warning from Pillow stops the recipe
        for name, c in BC.cases().items():
            names.append(name)
            out["file_" + name] = np.frombuffer(c.data, np.uint8)
            out["bgr_" + name] = cv2_like_bgr(c.data)
    # the decoder that made the vectors is the SIMD one: the model of its 16-bit lanes reproduces a case the full-width C arithmetic does not
    probe = "b-flat-dc-edges"
    if not np.array_equal(J.imread_bgr(BC.cases()[probe].data), out["bgr_" + probe]):
        raise SystemExit("this Pillow's libjpeg-turbo does not decode like the x86 SIMD islow IDCT: make the vectors on x86-64 with SIMD on")
    out["names"] = np.array(names)
    out["decoder"] = np.array("Pillow %s, libjpeg-turbo %s (libjpeg API %s), x86-64 SIMD" % (PIL.__version__, features.version("libjpeg_turbo"), features.version("jpg")))
    path = os.path.join(ROOT, "tests", "golden", "jpeg_beyond_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(names), "cases,", str(out["decoder"]))


if __name__ == "__main__":
    main()
