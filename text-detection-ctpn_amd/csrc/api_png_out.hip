// C ABI of libctpn_hip.so, PNG output unit: PNG writing of a batch on the device (kernels: png_enc.hip) -- the cv2.imwrite end of the
// PNG-named result images of ctpn/demo.py:28-52 (outlines and resize: api_out_stage.hip) --, and the host form of the same file
// (png_enc_dev.h: one text for both, so the two forms cannot disagree about a file). The coder takes a TABLE of images of any sizes and
// pitches over one device source (png_code_table: ctpn_encode_png_mixed, the ragged annotated writer of api_out_ragged.hip, the crop
// files of api_crops.hip); the uniform calls are tables of equal sizes at pitch 3 w.
#include "ctx.h"
#include "png_enc_dev.h"

namespace ctpn {

// a finished file to the caller's buffer or to a file of its own. Runs on a worker thread: nothing may leave it
static void png_deliver(const uint8_t* file, size_t bytes, uint8_t* out, size_t capacity, size_t* bytes_out, const char* path, int& st, std::string& msg) {
  if (path) {
    write_file(path, file, bytes, st, msg);
  } else {
    *bytes_out = bytes;
    if (bytes > capacity) { st = CTPN_ERR_CAPACITY; msg = "the file needs " + std::to_string(bytes) + " bytes, the buffer holds " + std::to_string(capacity); return; }
    std::memcpy(out, file, bytes);
  }
}

static bool png_size_ok(int h, int w) { return h > 0 && w > 0 && h <= 65535 && w <= 65535; }
static int png_device_size_check(const std::string& who, int h, int w) {      // the device form's bound on an image
  return (uint64_t)h * (1u + 3u * (uint64_t)w) <= PNGE_MAX_STREAM ? CTPN_OK : fail(CTPN_ERR_ARG, who + ": h (1 + 3 w) above 2^27: ctpn_png_encode takes such images");
}

// (ctx.h) the device form's bounds on a table, host arithmetic only: every size, every image's stream, the work items and the pieces
int png_table_check(const std::string& who, int n, const int* heights, const int* widths) {
  PngeTotals t = PngeTotals();
  for (int i = 0; i < n; ++i) {
    const std::string img = who + ": image " + std::to_string(i);
    if (!png_size_ok(heights[i], widths[i])) return fail(CTPN_ERR_ARG, img + ": bad size");
    if (int rc = png_device_size_check(img, heights[i], widths[i])) return rc;
    PngeImg d;
    pnge_describe(d, heights[i], widths[i]);
    t.pieces += d.npieces; t.items += pnge_groups(d);
  }
  return pnge_totals_ok(t) ? CTPN_OK : fail(CTPN_ERR_ARG, who + ": more than 2^31 - 1 work items or 2^32 pieces in one call");
}

// (ctx.h) n images over ONE device source px (complete in the ctx's copy queue, or produced in it): image i is heights[i] x widths[i] x 3
// at px + offsets[i], rows pitches[i] bytes apart -> n files, in the caller's buffers (out) or in files (paths). Every buffer is laid out
// by pnge_layout's prefix sums: a call costs the sum of its images, not n times the largest
int png_code_table(ctpn_ctx* c, const char* who, const uint8_t* px, int n, const int* heights, const int* widths, const size_t* pitches, const size_t* offsets, uint8_t* const* out,
                   const size_t* capacities, size_t* bytes_out, const char* const* paths) {
  int rc;
  if ((rc = png_table_check(who, n, heights, widths))) return rc;
  auto& P = c->pnge;
  hipStream_t qs = c->stream_c;
  if (int rc = P.ev_done.ensure()) return rc;
  c->pnge_stats[0] = c->pnge_stats[1] = c->pnge_stats[2] = c->pnge_stats[3] = 0;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_img = 0, o_hist = up(o_img + (size_t)n * sizeof(PngeImg)), o_res = o_hist + (size_t)n * PNGE_NSYM * 4, o_codes = up(o_res + (size_t)n * sizeof(PngeRes)),
               host_total = o_codes + (size_t)n * sizeof(PngeCodes);
  if ((rc = P.host.grow(host_total))) return rc;
  uint8_t* host = P.host.as<uint8_t>();
  PngeImg* imgs = (PngeImg*)(host + o_img);
  uint32_t* hist = (uint32_t*)(host + o_hist);
  PngeRes* res = (PngeRes*)(host + o_res);
  PngeCodes* codes = (PngeCodes*)(host + o_codes);
  for (int i = 0; i < n; ++i) pnge_describe(imgs[i], heights[i], widths[i]);
  PngeTotals t;
  pnge_layout(imgs, (size_t)n, t);
  for (int i = 0; i < n; ++i) { imgs[i].pix_off = offsets[i]; imgs[i].pitch = pitches[i]; }      // the caller's source, not the dense packing
  const size_t o_len = up(host_total), o_words = up(o_len + (size_t)t.pieces * sizeof(PngeLen)), dev_total = o_words + (size_t)t.words * 4;
  if ((rc = P.dev.grow(dev_total))) return rc;
  uint8_t* dev = P.dev.as<uint8_t>();
  // histograms -> the host, which builds every image's code and block header; one copy brings them back
  CTPN_HIP_TRY(hipMemcpyAsync(dev + o_img, imgs, (size_t)n * sizeof(PngeImg), hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipMemsetAsync(dev + o_hist, 0, (size_t)n * (PNGE_NSYM * 4 + sizeof(PngeRes)), qs));      // counters and result records
  if ((rc = launch_png_hist((const PngeImg*)(dev + o_img), px, (uint32_t*)(dev + o_hist), n, t.items, qs))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(hist, dev + o_hist, (size_t)n * PNGE_NSYM * 4, hipMemcpyDeviceToHost, qs));
  CTPN_HIP_TRY(hipEventRecord(P.ev_done, qs));
  CTPN_HIP_TRY(hipEventSynchronize(P.ev_done));
  c->pnge_stats[3] += (long long)n * PNGE_NSYM * 4;
  c->pool->run(n, [&](int i) { pnge_build_codes(imgs[i], hist + (size_t)i * PNGE_NSYM, codes[i]); });
  CTPN_HIP_TRY(hipMemcpyAsync(dev + o_codes, codes, (size_t)n * sizeof(PngeCodes), hipMemcpyHostToDevice, qs));
  CTPN_HIP_TRY(hipMemsetAsync(dev + o_words, 0, (size_t)t.words * 4, qs));      // the write pass ORs shared words into it
  if ((rc = launch_png_code((const PngeImg*)(dev + o_img), px, (const PngeCodes*)(dev + o_codes), (PngeLen*)(dev + o_len), (uint32_t*)(dev + o_words),
                            (PngeRes*)(dev + o_res), n, t.items, qs))) return rc;
  // the result records first, then exactly the bytes they name
  CTPN_HIP_TRY(hipMemcpyAsync(res, dev + o_res, (size_t)n * sizeof(PngeRes), hipMemcpyDeviceToHost, qs));
  CTPN_HIP_TRY(hipEventRecord(P.ev_done, qs));
  CTPN_HIP_TRY(hipEventSynchronize(P.ev_done));
  c->pnge_stats[3] += (long long)n * (long long)sizeof(PngeRes);
  std::vector<size_t> at((size_t)n, 0), back_at((size_t)n, 0);
  std::vector<char> on_host((size_t)n, 0);
  size_t file_total = 0, back_total = 0;
  for (int i = 0; i < n; ++i) {
    if (res[i].flag || (uint64_t)res[i].bytes > imgs[i].nwords * 4) { on_host[i] = 1; back_at[i] = back_total; back_total += (size_t)heights[i] * widths[i] * 3; continue; }
    at[i] = file_total;
    file_total += up((size_t)PNGE_FRAME_BYTES + res[i].bytes);
  }
  if ((rc = P.file_host.grow(file_total))) return rc;
  uint8_t* file_host = P.file_host.as<uint8_t>();
  std::vector<uint8_t> back;      // the pixels of the images the host form codes (none, unless a flag is raised), each a dense block
  try { back.resize(back_total); } catch (const std::exception& e) { return fail(CTPN_ERR_CAPACITY, std::string(who) + ": " + e.what()); }
  for (int i = 0; i < n; ++i) {
    if (on_host[i]) {
      ++c->pnge_stats[1];
      const size_t row = (size_t)widths[i] * 3;
      CTPN_HIP_TRY(hipMemcpy2DAsync(back.data() + back_at[i], row, px + offsets[i], pitches[i], row, (size_t)heights[i], hipMemcpyDeviceToHost, qs));
      c->pnge_stats[3] += (long long)(row * heights[i]);
      continue;
    }
    ++c->pnge_stats[0]; c->pnge_stats[2] += imgs[i].npieces;
    CTPN_HIP_TRY(hipMemcpyAsync(file_host + at[i] + PNGE_FRAME_FRONT, dev + o_words + (size_t)imgs[i].word0 * 4, res[i].bytes, hipMemcpyDeviceToHost, qs));
    c->pnge_stats[3] += (long long)res[i].bytes;
  }
  CTPN_HIP_TRY(hipEventRecord(P.ev_done, qs));
  CTPN_HIP_TRY(hipEventSynchronize(P.ev_done));
  std::vector<int> st((size_t)n, CTPN_OK);
  std::vector<std::string> msg((size_t)n);
  c->pool->run(n, [&](int i) {
    uint8_t* o = paths ? nullptr : out[i];
    const size_t cap = paths ? 0 : capacities[i];
    size_t* bo = paths ? nullptr : bytes_out + i;
    const char* path = paths ? paths[i] : nullptr;
    const int h = heights[i], w = widths[i];
    try {
      if (on_host[i]) {
        size_t need = 0;
        (void)pnge_encode_host(back.data() + back_at[i], h, w, nullptr, 0, &need, png_crc32);
        std::vector<uint8_t> file(need);
        (void)pnge_encode_host(back.data() + back_at[i], h, w, file.data(), need, &need, png_crc32);
        png_deliver(file.data(), need, o, cap, bo, path, st[i], msg[i]);
      } else {
        uint8_t* file = file_host + at[i];
        pnge_frame(file, h, w, res[i].bytes, res[i].adler, png_crc32);
        png_deliver(file, (size_t)PNGE_FRAME_BYTES + res[i].bytes, o, cap, bo, path, st[i], msg[i]);
      }
    } catch (const std::exception& e) { st[i] = CTPN_ERR_CAPACITY; msg[i] = e.what(); }
  });
  return first_failure(who, st, msg);
}

// the uniform calls: n images of h x w x 3, dense at px -- a table of equal sizes at pitch 3 w
static int png_code(ctpn_ctx* c, const char* who, const uint8_t* px, int n, int h, int w, uint8_t* const* out, const size_t* capacities, size_t* bytes_out, const char* const* paths) {
  const size_t per_px = (size_t)h * w * 3;
  std::vector<int> heights((size_t)n, h), widths((size_t)n, w);
  std::vector<size_t> pitches((size_t)n, (size_t)w * 3), offsets((size_t)n);
  for (int i = 0; i < n; ++i) offsets[i] = (size_t)i * per_px;
  return png_code_table(c, who, px, n, heights.data(), widths.data(), pitches.data(), offsets.data(), out, capacities, bytes_out, paths);
}

}  // namespace ctpn

extern "C" {

size_t ctpn_png_encode_capacity(int h, int w) { return png_size_ok(h, w) ? pnge_capacity(h, w) : 0; }

int ctpn_png_encode(const uint8_t* bgr, int h, int w, uint8_t* out, size_t capacity, size_t* bytes_out) {
  if (!bgr || !bytes_out || (!out && capacity)) return fail(CTPN_ERR_ARG, "ctpn_png_encode: null pointer");
  if (!png_size_ok(h, w)) return fail(CTPN_ERR_ARG, "ctpn_png_encode: bad size");
  try {
    if (!pnge_encode_host(bgr, h, w, out, out ? capacity : 0, bytes_out, png_crc32))
      return fail(CTPN_ERR_CAPACITY, "ctpn_png_encode: the file needs " + std::to_string(*bytes_out) + " bytes, the buffer holds " + std::to_string(capacity));
  } catch (const std::exception& e) { return fail(CTPN_ERR_CAPACITY, std::string("ctpn_png_encode: ") + e.what()); }
  return CTPN_OK;
}

int ctpn_encode_png_batch(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, uint8_t* const* out, const size_t* capacities, size_t* bytes_out) {
  const std::string who("ctpn_encode_png_batch");
  if (!c || !images || !out || !capacities || !bytes_out) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (n <= 0 || !png_size_ok(h, w)) return fail(CTPN_ERR_ARG, who + ": empty batch / bad size");
  int rc;
  if ((rc = png_device_size_check(who, h, w))) return rc;
  for (int i = 0; i < n; ++i) if (!out[i] && capacities[i]) return fail(CTPN_ERR_ARG, who + ": null output pointer");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + ": post-processing-only ctx");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  const uint8_t* px;
  if ((rc = stage_pixels(c, images, images_on_device, (size_t)n * h * w * 3, 256, c->stage.img_dev, c->stream_c, px))) return rc;
  return png_code(c, "ctpn_encode_png_batch", px, n, h, w, out, capacities, bytes_out, nullptr);
}

int ctpn_encode_png_mixed(ctpn_ctx* c, const uint8_t* source, int source_on_device, size_t source_bytes, int n, const int* heights, const int* widths, const size_t* pitches,
                          const size_t* offsets, uint8_t* const* out, const size_t* capacities, size_t* bytes_out) {
  const std::string who("ctpn_encode_png_mixed");
  if (!c || !source || !heights || !widths || !pitches || !offsets || !out || !capacities || !bytes_out) return fail(CTPN_ERR_ARG, who + ": null pointer");
  if (n <= 0) return fail(CTPN_ERR_ARG, who + ": empty batch");
  const size_t limit = (size_t)1 << 40;      // (offset + row * pitch cannot wrap)
  for (int i = 0; i < n; ++i) {
    const std::string img = who + ": image " + std::to_string(i);
    if (!png_size_ok(heights[i], widths[i])) return fail(CTPN_ERR_ARG, img + ": bad size");
    if (pitches[i] < (size_t)widths[i] * 3) return fail(CTPN_ERR_ARG, img + ": the pitch is below 3 * width");
    if (pitches[i] >= limit || offsets[i] >= limit) return fail(CTPN_ERR_ARG, img + ": pitch or offset of 2^40 bytes or more");
    if (!out[i] && capacities[i]) return fail(CTPN_ERR_ARG, img + ": null output pointer");
    if (!source_on_device) {
      const size_t span = (size_t)(heights[i] - 1) * pitches[i] + (size_t)widths[i] * 3;
      if (pitches[i] > source_bytes || offsets[i] > source_bytes || span > source_bytes - offsets[i]) return fail(CTPN_ERR_ARG, img + " does not lie inside source_bytes");
    }
  }
  int rc;
  if ((rc = png_table_check(who, n, heights, widths))) return rc;
  if (c->postproc_only) return fail(CTPN_ERR_STATE, who + ": post-processing-only ctx");
  CTPN_HIP_TRY(hipSetDevice(c->device));
  const uint8_t* px;
  if ((rc = stage_pixels(c, source, source_on_device, source_bytes, 0, c->stage.img_dev, c->stream_c, px))) return rc;
  return png_code_table(c, "ctpn_encode_png_mixed", px, n, heights, widths, pitches, offsets, out, capacities, bytes_out, nullptr);
}

int ctpn_write_annotated_png_files(ctpn_ctx* c, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs, int line_capacity,
                                   const int* line_counts, double scale, const char* const* paths) {
  const uint8_t* px;
  int dh, dw;
  if (int rc = annotate_batch(c, "ctpn_write_annotated_png_files", "PNG", png_device_size_check, images, images_on_device, n, h, w, recs, line_capacity, line_counts, scale, paths, px, dh, dw)) return rc;
  return png_code(c, "ctpn_write_annotated_png_files", px, n, dh, dw, nullptr, nullptr, nullptr, paths);
}

int ctpn_png_encode_device_stats(ctpn_ctx* c, long long* out4) {
  if (!c || !out4) return fail(CTPN_ERR_ARG, "ctpn_png_encode_device_stats: null pointer");
  std::memcpy(out4, c->pnge_stats, sizeof(c->pnge_stats));
  return CTPN_OK;
}

}  // extern "C"
