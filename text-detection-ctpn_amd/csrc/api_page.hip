// C ABI of libctpn_hip.so, page unit: a page larger than the network input as tiles at native resolution -- the plan and the merge (host
// arithmetic, no device), the cut (page.hip), the page form of the connector's NMS (nms.hip) and the page-level text-line tail. All five are
// stateless: no ctx is read, so they may be called whatever a ctx's slots are doing. The definitions: include/ctpn_hip.h, "pages in tiles".
#include "ctx.h"
#include "page_dev.h"

#include <cmath>

namespace {
using namespace ctpn;

struct PageNmsCache {
  std::mutex mu;
  Stream stream;
  int cap = 0;       // boxes the blocks have room for
  int units = 0;     // ... and partition units the histogram block has
  DevBuf boxes, spill, list, hist, colbase, alive, keep, count;
};
// one per device, for the life of the process, like ctpn_nms's cache (api_proposals.hip): allocated once and deliberately never destroyed
PageNmsCache* const g_page_nms = new PageNmsCache[16];

int page_device(int device_id, const char* who) {
  const int ndev = ctpn_device_count();
  if (ndev <= 0) return fail(CTPN_ERR_NODEVICE, std::string(who) + ": no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev || device_id >= 16) return fail(CTPN_ERR_ARG, std::string(who) + ": device_id out of range");
  return CTPN_OK;
}

// The page form's domain (common.h, launch_nms_columns' PRECONDITION, on the boxes themselves): every box's x-extent inside [16 c, 16 c + 16] of
// its column c = int(x1) >> 4 < 1024, so boxes two columns apart are disjoint and neighbours share one pixel column; and of two neighbouring
// columns at least one holds no box narrower than 10 px, so that shared column is at most 1/10 of the wider box: IoU < 0.1 <= thresh whatever
// the heights. (A page's merged proposals are 16 or 17 px wide; only a clipped last column is thinner.) -> ncols, or 0 outside the domain
int page_nms_columns(const float* boxes, int n, int dim) {
  std::vector<float> wmin(NMS_PAGE_MAXCOL, 1e30f);
  int ncols = 0;
  for (int i = 0; i < n; ++i) {
    const float x1 = boxes[(size_t)i * dim], y1 = boxes[(size_t)i * dim + 1], x2 = boxes[(size_t)i * dim + 2], y2 = boxes[(size_t)i * dim + 3];
    if (!(x1 >= 0.f && x1 < 16.f * NMS_PAGE_MAXCOL) || !std::isfinite(y1) || !std::isfinite(y2)) return 0;
    const int c = (int)x1 >> 4;
    if (!(x2 >= x1 && x2 <= (float)(16 * c + 16))) return 0;
    wmin[c] = std::min(wmin[c], x2 - x1 + 1.f);
    ncols = std::max(ncols, c + 1);
  }
  for (int c = 0; c + 1 < ncols; ++c)
    if (wmin[c] < 10.f && wmin[c + 1] < 10.f) return 0;
  return ncols;
}

}  // namespace

extern "C" {

int ctpn_page_plan(int page_h, int page_w, int tile_h, int tile_w, int overlap, int* tiles8, int capacity, int* count_out, int* grid2) {
  if (!count_out) return fail(CTPN_ERR_ARG, "ctpn_page_plan: count_out is null");
  *count_out = 0;
  if (!pg_plan_ok(page_h, page_w, tile_h, tile_w, overlap))
    return fail(CTPN_ERR_ARG, "ctpn_page_plan: page sides 16 .. 16384, tile sides multiples of 16, overlap a multiple of 32 in 0 .. min(tile_h, tile_w) / 2");
  const int ky = pg_axis_tiles(page_h, tile_h, overlap), kx = pg_axis_tiles(page_w, tile_w, overlap);
  *count_out = ky * kx;
  if (grid2) { grid2[0] = ky; grid2[1] = kx; }
  if (!tiles8) return CTPN_OK;
  if (ky * kx > capacity) return fail(CTPN_ERR_CAPACITY, "ctpn_page_plan: more tiles than capacity");
  PgTile* out = reinterpret_cast<PgTile*>(tiles8);
  for (int j = 0; j < ky; ++j)
    for (int i = 0; i < kx; ++i) {
      PgTile& d = out[j * kx + i];
      pg_axis_tile(page_h, tile_h, overlap, ky, j, d.oy, d.valid_h, d.own_y0, d.own_y1);
      pg_axis_tile(page_w, tile_w, overlap, kx, i, d.ox, d.valid_w, d.own_x0, d.own_x1);
    }
  return CTPN_OK;
}

int ctpn_page_cut(int device_id, const uint8_t* page, int page_on_device, int page_h, int page_w, long long pitch_bytes, const int* tiles8, int first, int n,
                  int tile_h, int tile_w, uint8_t* out, int out_on_device, long long capacity_bytes) {
  if (!page || !tiles8 || !out || first < 0 || n <= 0) return fail(CTPN_ERR_ARG, "ctpn_page_cut: null pointer / empty range of tiles");
  if (page_h < PG_MIN_SIDE || page_h > PG_MAX_SIDE || page_w < PG_MIN_SIDE || page_w > PG_MAX_SIDE || pitch_bytes < 3LL * page_w)
    return fail(CTPN_ERR_ARG, "ctpn_page_cut: page sides 16 .. 16384, pitch_bytes >= 3 page_w");
  if (tile_h < 16 || tile_h > PG_MAX_SIDE || tile_w < 16 || tile_w > PG_MAX_SIDE || (tile_h & 15) || (tile_w & 15))
    return fail(CTPN_ERR_ARG, "ctpn_page_cut: tile sides are multiples of 16");
  const PgTile* tiles = reinterpret_cast<const PgTile*>(tiles8) + first;
  for (int t = 0; t < n; ++t)
    if (!pg_tile_ok(tiles[t], page_h, page_w, tile_h, tile_w)) return fail(CTPN_ERR_ARG, "ctpn_page_cut: a tile's valid part lies outside the page or the tile");
  const long long need = (long long)n * tile_h * tile_w * 3;
  if (capacity_bytes < need) return fail(CTPN_ERR_CAPACITY, "ctpn_page_cut: capacity_bytes too small");
  if (out_on_device && ((uintptr_t)out & 3)) return fail(CTPN_ERR_ARG, "ctpn_page_cut: a device tile buffer is 4-byte aligned");
  int rc = page_device(device_id, "ctpn_page_cut");
  if (rc) return rc;
  CTPN_HIP_TRY(hipSetDevice(device_id));
  Stream st;
  DevBuf dpage, dtiles, dout;      // released before the stream, on every way out
  if ((rc = st.ensure())) return rc;
  const uint8_t* p_in = page;
  if (!page_on_device) {
    const size_t pbytes = (size_t)(page_h - 1) * (size_t)pitch_bytes + (size_t)page_w * 3;      // to the last pixel's last byte, and no further
    if ((rc = dpage.alloc(pbytes))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(dpage.get(), page, pbytes, hipMemcpyHostToDevice, st));
    p_in = dpage.as<uint8_t>();
  }
  if ((rc = dtiles.alloc((size_t)n * sizeof(PgTile)))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(dtiles.get(), tiles, (size_t)n * sizeof(PgTile), hipMemcpyHostToDevice, st));
  uint8_t* d_out = out;
  if (!out_on_device) { if ((rc = dout.alloc((size_t)need))) return rc; d_out = dout.as<uint8_t>(); }
  if ((rc = launch_page_cut(p_in, pitch_bytes, dtiles.as<PgTile>(), n, tile_h, tile_w, d_out, st))) return rc;
  if (!out_on_device) CTPN_HIP_TRY(hipMemcpyAsync(out, dout.get(), (size_t)need, hipMemcpyDeviceToHost, st));
  CTPN_HIP_TRY(hipStreamSynchronize(st));
  return CTPN_OK;
}

int ctpn_page_merge(const int* tiles8, int n_tiles, const float* rois, int roi_capacity, const int* roi_counts, int page_h, int page_w, float min_size,
                    float* boxes_out, float* scores_out, int* src_out, int capacity, int* count_out) {
  if (!count_out) return fail(CTPN_ERR_ARG, "ctpn_page_merge: count_out is null");
  *count_out = 0;
  if (!tiles8 || !rois || !roi_counts || n_tiles <= 0 || roi_capacity <= 0 || page_h <= 0 || page_w <= 0 || capacity < 0)
    return fail(CTPN_ERR_ARG, "ctpn_page_merge: bad arguments");
  if (capacity > 0 && (!boxes_out || !scores_out || !src_out)) return fail(CTPN_ERR_ARG, "ctpn_page_merge: null output");
  if ((long long)n_tiles * roi_capacity > 0x7fffffffLL) return fail(CTPN_ERR_ARG, "ctpn_page_merge: tiles x roi_capacity does not fit src_out");
  const PgTile* tiles = reinterpret_cast<const PgTile*>(tiles8);
  const float xmax = (float)(page_w - 1), ymax = (float)(page_h - 1);
  long long cnt = 0;
  for (int t = 0; t < n_tiles; ++t) {
    const PgTile& d = tiles[t];
    if (roi_counts[t] < 0 || roi_counts[t] > roi_capacity) return fail(CTPN_ERR_ARG, "ctpn_page_merge: a tile's roi count exceeds roi_capacity");
    const float oy = (float)d.oy, ox = (float)d.ox, cy_lo = (float)(d.own_y0 - d.oy), cy_hi = (float)(d.own_y1 - d.oy);
    for (int r = 0; r < roi_counts[t]; ++r) {
      const float* p = rois + ((size_t)t * roi_capacity + r) * 5;
      const float x1 = p[1], y1 = p[2], x2 = p[3], y2 = p[4];
      if (!(x1 >= 0.f && x1 < 32768.f)) continue;      // (no column)
      const int col = (((int)x1 >> 4) << 4) + d.ox;
      if (col < d.own_x0 || col >= d.own_x1) continue;
      const float cy = (y1 + y2) * 0.5f;
      if (!(cy_lo <= cy && cy < cy_hi)) continue;
      const float X1 = x1 + ox, Y1 = y1 + oy;
      float X2 = x2 + ox, Y2 = y2 + oy;
      X2 = X2 > xmax ? xmax : X2;
      Y2 = Y2 > ymax ? ymax : Y2;
      if (X2 - X1 + 1.f < min_size || Y2 - Y1 + 1.f < min_size) continue;
      if (cnt < capacity) {
        float* b = boxes_out + (size_t)cnt * 4;
        b[0] = X1; b[1] = Y1; b[2] = X2; b[3] = Y2;
        scores_out[cnt] = p[0];
        src_out[cnt] = t * roi_capacity + r;
      }
      ++cnt;
    }
  }
  *count_out = (int)cnt;
  if (cnt > capacity) return fail(CTPN_ERR_CAPACITY, "ctpn_page_merge: more proposals than capacity");
  return CTPN_OK;
}

int ctpn_page_nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim, float thresh, int device_id) {
  if (!keep_out || !num_out) return fail(CTPN_ERR_ARG, "ctpn_page_nms: null output");
  *num_out = 0;
  if (boxes_num == 0) return CTPN_OK;
  if (!boxes_host || boxes_num < 0 || boxes_dim < 4) return fail(CTPN_ERR_ARG, "ctpn_page_nms: boxes must be N x (>=4)");
  if (boxes_num > NMS_PAGE_MAXN || !(thresh >= 0.1f)) return fail(CTPN_ERR_ARG, "ctpn_page_nms: at most 2^20 boxes, thresh >= 0.1 (ctpn_nms takes anything)");
  const int ncols = page_nms_columns(boxes_host, boxes_num, boxes_dim);
  if (ncols < 1) return fail(CTPN_ERR_ARG, "ctpn_page_nms: a box outside the column decomposition's domain (x-extent inside its 16-px column; ctpn_nms takes anything)");
  int rc = page_device(device_id, "ctpn_page_nms");
  if (rc) return rc;
  PageNmsCache& nc = g_page_nms[device_id];
  std::lock_guard<std::mutex> lk(nc.mu);
  CTPN_HIP_TRY(hipSetDevice(device_id));
  if ((rc = nc.stream.ensure())) return rc;
  const int units = nms_page_units(boxes_num);
  if (nc.cap < boxes_num || nc.units < units) {
    const size_t cap = std::max<size_t>({(size_t)boxes_num, (size_t)nc.cap, 32768});
    const int un = std::max(units, nms_page_units((int)std::min<size_t>(cap, NMS_PAGE_MAXN)));
    nc.cap = 0;
    if ((rc = nc.boxes.grow(cap * 4 * sizeof(float))) || (rc = nc.spill.grow(cap * 4 * sizeof(float))) || (rc = nc.list.grow(cap * sizeof(int))) ||
        (rc = nc.keep.grow(cap * sizeof(int))) || (rc = nc.alive.grow((cap + 31) / 32 * sizeof(unsigned))) ||
        (rc = nc.hist.grow((size_t)NMS_PAGE_MAXCOL * un * sizeof(unsigned))) || (rc = nc.colbase.grow((NMS_PAGE_MAXCOL + 1) * sizeof(unsigned))) ||
        (rc = nc.count.grow(sizeof(int))))
      return rc;
    nc.cap = (int)cap;
    nc.units = un;
  }
  std::vector<float> b4((size_t)boxes_num * 4);
  for (int i = 0; i < boxes_num; ++i) std::memcpy(&b4[(size_t)i * 4], boxes_host + (size_t)i * boxes_dim, 4 * sizeof(float));
  CTPN_HIP_TRY(hipMemcpyAsync(nc.boxes.get(), b4.data(), b4.size() * sizeof(float), hipMemcpyHostToDevice, nc.stream));
  if ((rc = launch_nms_page_columns(nc.boxes.as<float>(), boxes_num, ncols, thresh, nc.list.as<int>(), nc.hist.as<unsigned>(), nc.colbase.as<unsigned>(),
                                    nc.spill.as<float>(), nc.alive.as<unsigned>(), nc.keep.as<int>(), nc.count.as<int>(), nc.stream)))
    return rc;
  int nk = 0;
  CTPN_HIP_TRY(hipMemcpyAsync(&nk, nc.count.get(), sizeof(int), hipMemcpyDeviceToHost, nc.stream));
  CTPN_HIP_TRY(hipStreamSynchronize(nc.stream));
  if (nk < 0 || nk > boxes_num) return fail(CTPN_ERR_HIP, "ctpn_page_nms: device returned an impossible keep count");
  CTPN_HIP_TRY(hipMemcpyAsync(keep_out, nc.keep.get(), (size_t)nk * sizeof(int), hipMemcpyDeviceToHost, nc.stream));
  CTPN_HIP_TRY(hipStreamSynchronize(nc.stream));
  *num_out = nk;
  return CTPN_OK;
}

int ctpn_page_text_lines(const float* boxes, const float* scores, int r, int page_h, int page_w, int mode, int device_id, const double* cfg8, int nms_form,
                         double* recs_out, int capacity, int* count_out) {
  if (!count_out) return fail(CTPN_ERR_ARG, "ctpn_page_text_lines: count_out is null");
  *count_out = 0;
  if (r > 0 && (!boxes || !scores)) return fail(CTPN_ERR_ARG, "ctpn_page_text_lines: null input");
  if (nms_form != 0 && nms_form != 1) return fail(CTPN_ERR_ARG, "ctpn_page_text_lines: nms_form is 0 (ctpn_nms) or 1 (ctpn_page_nms)");
  ConnectorCfg cfg = default_connector_cfg();
  int rc = connector_cfg_from8(cfg8, cfg);
  if (rc) return rc;
  std::vector<double> recs;
  rc = text_lines_host(boxes, scores, r, page_h, page_w, mode, device_id, cfg, recs, nms_form == 1 ? ctpn_page_nms : ctpn_nms);
  if (rc) return rc;
  const int cnt = (int)(recs.size() / 9);
  *count_out = cnt;
  if (cnt > capacity) return fail(CTPN_ERR_CAPACITY, "ctpn_page_text_lines: more lines than capacity");
  if (cnt && !recs_out) return fail(CTPN_ERR_ARG, "ctpn_page_text_lines: recs_out is null");
  if (cnt) std::memcpy(recs_out, recs.data(), recs.size() * sizeof(double));
  return CTPN_OK;
}

}  // extern "C"
