// Pages larger than the network input, detected as tiles at native resolution (include/ctpn_hip.h, ctpn_page_*): the plan's arithmetic and the
// per-thread text of page.hip's kernel as host + device functions. The kernel calls pg_cut_thread with its thread index; tests/page_host.cpp
// compiles this same text with g++ under ASan + UBSan and calls it from a loop over those indices.
//   PgTile          one tile of a plan, in page coordinates: the record of ctpn_page_plan's tiles8
//   pg_axis_tiles   tiles along one axis of length L, tile T, overlap V
//   pg_axis_tile    tile j of k along that axis: origin, valid extent, owned range [own0, own1)
//   pg_pixel        one page pixel, read byte by byte: no alignment of the page or of its pitch is assumed
//   pg_cut_thread   four consecutive pixels of one row of one tile, stored as three aligned dwords
// Along an axis: L <= T is one tile at 0; otherwise the stride is S = T - V and k = ceil((L - T) / S) + 1 tiles sit at j S, so the last
// tile's valid part min(T, L - origin) is wider than V. Tile j owns [origin_j + V / 2, origin_{j+1} + V / 2), from 0 for the first and to L
// for the last: the owned ranges partition the axis, every owned range lies inside its tile's valid part, and with T a multiple of 16 and V
// of 32 all origins and all bounds but L are multiples of 16 -- the page's anchor grid is every tile's.
// Nothing here includes a HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ inline
#else
#define PG_HD inline
#endif

namespace ctpn {

struct PgTile { int oy, ox, valid_h, valid_w, own_y0, own_y1, own_x0, own_x1; };

constexpr int PG_THREADS = 256;
constexpr int PG_MIN_SIDE = 16, PG_MAX_SIDE = 16384;
// what a tile holds outside the page: round(PIXEL_MEANS), BGR (conv_first_q.hip's m) -- the q-image's zero, i.e. im_list_to_blob's padding
constexpr uint32_t PG_FILL = 103u | (116u << 8) | (123u << 16);

PG_HD bool pg_plan_ok(int page_h, int page_w, int tile_h, int tile_w, int overlap) {
  if (page_h < PG_MIN_SIDE || page_h > PG_MAX_SIDE || page_w < PG_MIN_SIDE || page_w > PG_MAX_SIDE) return false;
  if (tile_h < 16 || tile_h > PG_MAX_SIDE || tile_w < 16 || tile_w > PG_MAX_SIDE || (tile_h & 15) || (tile_w & 15)) return false;
  const int t = tile_h < tile_w ? tile_h : tile_w;
  return overlap >= 0 && (overlap & 31) == 0 && overlap <= t / 2;
}

PG_HD int pg_axis_tiles(int L, int T, int V) {
  if (L <= T) return 1;
  const int S = T - V;
  return (L - T + S - 1) / S + 1;
}

PG_HD void pg_axis_tile(int L, int T, int V, int k, int j, int& origin, int& valid, int& own0, int& own1) {
  const int S = T - V;
  origin = j * S;
  valid = T < L - origin ? T : L - origin;
  own0 = j == 0 ? 0 : origin + V / 2;
  own1 = j == k - 1 ? L : origin + S + V / 2;
}

// is d a tile a cut may read: inside the page, no larger than the tile buffer
PG_HD bool pg_tile_ok(const PgTile& d, int page_h, int page_w, int tile_h, int tile_w) {
  return d.oy >= 0 && d.ox >= 0 && d.valid_h >= 1 && d.valid_w >= 1 && d.valid_h <= tile_h && d.valid_w <= tile_w && d.oy <= page_h - d.valid_h &&
         d.ox <= page_w - d.valid_w;
}

// pixel (y, x) of the page, 0 <= y < page_h and 0 <= x < page_w: B | G << 8 | R << 16
PG_HD uint32_t pg_pixel(const uint8_t* page, long long pitch, int y, int x) {
  const uint8_t* p = page + (long long)y * pitch + (long long)x * 3;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// threads a cut of n tiles takes: one per four pixels (tile_w is a multiple of 16: the four share a row, and there is no tail)
PG_HD long long pg_cut_groups(int n, int tile_h, int tile_w) { return (long long)n * tile_h * (tile_w / 4); }

// Thread index grp: pixels 4 grp .. 4 grp + 3 of out's linear order (n x tile_h x tile_w x 3 bytes, 4-byte aligned).
PG_HD void pg_cut_thread(const uint8_t* page, long long pitch, const PgTile* tiles, int n, int tile_h, int tile_w, uint8_t* out, long long grp) {
  const int gw = tile_w / 4;
  const long long per = (long long)tile_h * gw;
  if (grp < 0 || grp >= per * n) return;
  const int t = (int)(grp / per);
  const int rem = (int)(grp - (long long)t * per);
  const int y = rem / gw, x0 = (rem - y * gw) * 4;
  const PgTile d = tiles[t];
  uint32_t px[4];
  for (int k = 0; k < 4; ++k) px[k] = (y < d.valid_h && x0 + k < d.valid_w) ? pg_pixel(page, pitch, d.oy + y, d.ox + x0 + k) : PG_FILL;
  uint32_t* o = reinterpret_cast<uint32_t*>(out + (grp * 4) * 3);
  o[0] = px[0] | (px[1] << 24);
  o[1] = (px[1] >> 8) | (px[2] << 16);
  o[2] = (px[2] >> 16) | (px[3] << 8);
}

}  // namespace ctpn
