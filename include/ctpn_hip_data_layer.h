/* libctpn_hip.so, the training data layer: what the reference does to a labelled folder before a training step sees it -- split_label.py's
 * 16-px strips for a whole label set, a decoded page resized / mirrored / mean-subtracted, a page's strips as the step's gt boxes. Part of
 * the training-side header: include ctpn_hip_train.h, which includes this file (it can also be included alone). Additive to ABI version 10;
 * the binding declares these calls in _declare_data_layer. */
#ifndef CTPN_HIP_DATA_LAYER_H
#define CTPN_HIP_DATA_LAYER_H

#include "ctpn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Three stateless calls in ctpn_anchor_targets' conventions -- no ctx; device_id; a non-blocking stream of the
 * call's own; on_device = 1: the tensor-sized arrays are pointers into that device's memory and nothing tensor-sized crosses to the host;
 * CTPN_ERR_ARG before any device work; CTPN_ERR_NODEVICE without a device (there is no CPU fallback). Kernels: csrc/data_layer.hip; their
 * per-thread text, which tests/data_layer_host.cpp compiles for the host: csrc/data_layer_dev.h. */

/* lib/prepare_training_data/split_label.py:36-104 for a whole label set in one call: every quadrilateral of every page cut into 16-px strips.
 * page_dims: pages x 4 ints (file h, file w, resized h, resized w), each in 1 .. 65535; quads: Q x 8 doubles, the eight numbers of a label
 * line as float(text) (x1, y1, .. x4, y4), page p's lines at [quad_offsets[p], quad_offsets[p + 1]); quad_offsets: pages + 1 ints from 0,
 * never falling (Q = the last, at most 2^18). page_dims, quad_offsets and strip_offsets are always the host's; quads, strips and
 * quad_strip_offsets follow on_device.
 * strips: S x 4 floats x1, y1, x2, y2, whole numbers in resized-page coordinates, in quad order and within a quad left to right;
 * strip_offsets: pages + 1 ints, page p's strips at [strip_offsets[p], strip_offsets[p + 1]); quad_strip_offsets (may be null): Q + 1 ints,
 * the same per quad. capacity_strips = 0 is the probe: the offsets are filled and nothing else is written. 0 < capacity_strips < S:
 * CTPN_ERR_CAPACITY with the offsets filled and strips untouched.
 * Three passes: the strips of every quad counted, an exclusive scan of the counts (csrc/wg_scan.h; no atomics, so a strip's place is a
 * function of the input alone), the strips written. The call synchronises after the scan -- the total decides what follows -- and at its end.
 * The arithmetic is the reference's, in its order:
 *   a coordinate is int(v / file_w * resized_w) (y: the heights) in IEEE double -- one division, then one multiplication, truncated towards
 *   zero (a NaN, or a value beyond +-2^30 after the scaling, saturates there: Python would raise or carry a bignum);
 *   the four points are sorted by x, stably; of the left two the upper is pt1 and the lower pt3 (y[0] < y[1] ? 0 : 1), of the right two the
 *   upper is pt2 and the lower pt4; xmin = min(pt1.x, pt2.x), xmax = max(pt2.x, pt4.x), ymin = min(pt1.y, pt2.y), ymax = max(pt3.y, pt4.y);
 *   xmin and ymin are raised to 0, xmax and ymax lowered to resized w - 1 and h - 1 (and nothing else: xmin may lie right of the page).
 * The strip rule, quirks kept. With start = the first multiple of 16 above xmin and m_1 = start < m_2 < .. < m_k the multiples of 16
 * strictly between xmin and xmax, the strips (x1, x2) are (xmin, start - 1), (m_1, m_1 + 15), .. (m_k-1, m_k-1 + 15), (m_k, xmax), and then
 * the first is deleted where xmin == start - 1:
 *   (5, 100) -> (5, 15) (16, 31) .. (80, 95) (96, 100);  (3, 17) -> (3, 15) (16, 17);  (16, 33) -> (16, 31) (32, 33);
 *   (31, 48) -> (32, 48) alone: the first strip has x_left == x_right and is deleted, and the last is 17 wide;
 *   k = 0 (no multiple of 16 strictly between): ONE strip (xmin, start - 1), which ignores xmax -- (3, 10), (3, 15) and (3, 16) all give
 *   (3, 15), (16, 32) gives (16, 31), and x2 may lie beyond the page (x2 = 15 on a page 12 wide); with xmin % 16 == 15 it is deleted as
 *   well and nothing is written: (15, 16) gives no strip;
 *   xmin == xmax stops the reference (np.delete out of bounds); here, as an extension, it gives no strip.
 * y1 = ymin and y2 = ymax on every strip of a quad. */
int ctpn_split_labels(int device_id, int pages, const int* page_dims, const double* quads, const int* quad_offsets, int on_device, float* strips,
                      long long capacity_strips, int* strip_offsets, int* quad_strip_offsets);

/* One decoded page -> what a step reads, in one pass. image: h x w x 3 BGR uint8 on the host (image_on_device = 0) or the device, rows pitch
 * bytes apart (pitch >= 3 w); neither the pointer nor the pitch needs any alignment. factor: fx = fy of the resize; <= 0 or 1: no resize.
 * image_out (device): out_h x out_w x 3 uint8 = ctpn_resize(image, factor) with each row mirrored left to right where flip = 1 -- resize
 * first, mirror after, the order of the reference's pipeline (split_label.py resizes the file, minibatch.py:137-138 mirrors the resized
 * file); the two orders differ because the sample positions are rounded to float32. The per-sample arithmetic is csrc/resize_pixel.h's.
 * blob_out (device, 4-byte aligned, may be null): out_h x out_w x 3 float32 = (double)pixel - PIXEL_MEANS[c] rounded once: the conv1_1 blob
 * of the backward pass. out_h, out_w: ctpn_resize_dims' result for (h, w, factor, factor), else CTPN_ERR_ARG. A host image crosses in one
 * copy, pitch included, through a page-locked block of the call. Stores are 16 bytes wide where the output is 16-byte aligned, 4 otherwise
 * (image_out at an odd address: single bytes). Returns when both outputs are complete. */
int ctpn_train_page(int device_id, const uint8_t* image, int image_on_device, int h, int w, long long pitch, double factor, int flip, uint8_t* image_out,
                    float* blob_out, int out_h, int out_w);

/* imdb.append_flipped_images (lib/datasets/imdb.py:84-100) and minibatch.py:29-32 for one page's strips. strips: g x 4 floats (x1, y1, x2, y2)
 * -> gt_boxes_out: g x 5 floats (x1, y1, x2, y2, 1.0); both follow on_device. The reference holds boxes as uint16 (pascal_voc.py:134): a
 * value outside 0 .. 65535 is CTPN_ERR_ARG (host strips: before any device work; device strips: found by the kernel, whose rows for such
 * strips stay unwritten), page_width is in 1 .. 65535. flip = 1: x1' = page_width - x2 - 1 and x2' = page_width - x1 - 1 in uint16
 * arithmetic, which wraps -- reachable: the one-strip quirk above writes x2 = 15 on a page 12 wide -- then x1' = 0 where x2' < x1'. Then
 * every coordinate times scale in double, rounded once to float32. */
int ctpn_train_boxes(int device_id, const float* strips, int g, int page_width, int flip, double scale, int on_device, float* gt_boxes_out);


#ifdef __cplusplus
}
#endif
#endif /* CTPN_HIP_DATA_LAYER_H */
