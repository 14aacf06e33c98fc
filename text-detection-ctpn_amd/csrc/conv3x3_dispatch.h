// c3_dispatch: which kernel family (conv3x3_tiled.h, conv3x3_persistent.h) a layer takes.
#pragma once
#include "conv3x3_tiled.h"
#include "conv3x3_persistent.h"
namespace ctpn {

// Kernel family for one layer. Co <= 64 (conv1_2 outside the 16-bit modes' weights-in-registers kernel): the non-persistent kernel on
// 256 x 64 tiles; Co % 128 == 0 with ReLU (every other layer of the network): persistent workgroups, flat windows where the map is small
// enough, else 8 x 32 or 16 x 16 patches -- whichever covers the map with fewer tiles; anything else (debug entry point): non-persistent
// 256 x 128 tiles.
template <typename T, bool SPLIT = false>
static int c3_dispatch(const Conv3& g, bool pool, hipStream_t s) {
  using OT = typename std::conditional<SPLIT, float, T>::type;      // staging type of the non-persistent kernel's LDS epilogue
  const bool flat = c3_flat_ok(g, pool);
  // conv1_2 in split precision (option conv_p64, default 1): the persistent kernel's 64-channel form, 3.56 ms against the
  // non-persistent kernel's 4.53 at batch 32 (same box: 1145 against 1115 images/s, profiles/r06_ab_split_conv1.txt). NOT fp32: exact-fp32
  // MFMAs are 16 x slower per flop, the per-tile fixed costs the persistent form removes are 1 % there (measured: 352.3 against 353.4
  // images/s at batch 8)
  if constexpr (SPLIT) {
    if (g.Co == 64 && g.relu && g.opt_p64 != 0)
      return pool ? c3_launch_p<T, false, true, 32, SPLIT, 64>(g, s) : c3_launch_p<T, false, false, 32, SPLIT, 64>(g, s);
  }
  if (g.Co <= 64)
    return pool ? c3_launch<T, OT, 64, 4, 1, false, true, 2, 3, 32, SPLIT>(g, s) : c3_launch<T, OT, 64, 4, 1, false, false, 2, 3, 32, SPLIT>(g, s);
  const bool persist = g.Co % 128 == 0 && g.relu;      // the persistent kernel's epilogue has the ReLU built in
  // 16 x 16 patches where they cover the map with fewer tiles. (Round 6 also tried choosing by ROUNDS of the persistent walk for one-image
  // problems -- conv3_x of one 600 x 900 image is 266 8 x 32-patch tiles on 256 CUs, two rounds for ten tiles, against 280 16 x 16-patch tiles =
  // one round + a half-tile tail: measured 45.0 / 28.2 / 45.4 / 46.7 us for conv2_2 .. conv3_3 against 39.0 / 29.3 / 48.2 / 45.5 with this
  // rule -- the 16 x 16 kernel's tile is slower than the 8 x 32 kernel's by what the tail saves; profiles/r06_timeline_sync_1image_tiling_by_rounds.txt.)
  const bool tw16 = !flat && c3_tiles2d(g, pool, 16) < c3_tiles2d(g, pool, 32);
  if (persist) {
    if (flat) {
      // one image per call (conv5_x / rpn_conv of a 600 x 900 image: 36 tiles of 256 x 128): 64-pixel x 128-channel items, one round on the machine
      int dev = 0, ncu = 0;
      const long long m_total = (long long)g.N * (g.H + 2) * (g.W + 2), tn = (g.Co + 127) / 128;
      const long long t256 = (m_total + 255) / 256 * tn, t64 = (m_total + 63) / 64 * tn;
      if (g.opt_small != 0 && 2 * (g.W + 2) + 66 <= 37 * 8 && current_device(dev) == CTPN_OK && device_cu_count(dev, ncu) == CTPN_OK && 2 * t256 <= ncu && t64 <= ncu)
        return c3_launch_p<T, true, false, 32, SPLIT, 128, 64>(g, s);
      return c3_launch_p<T, true, false, 32, SPLIT>(g, s);
    }
    if (tw16) return pool ? c3_launch_p<T, false, true, 16, SPLIT>(g, s) : c3_launch_p<T, false, false, 16, SPLIT>(g, s);
    {
      // one or two images per call: 8 x 32 patches with a half-tile tail where the walk's last round is at most half full (conv3_x of one
      // 600 x 900 image: 266 tiles on 256 CUs -- the ten tiles of the second round as twenty halves: 1.59 rounds instead of 2).
      // (At batch 32 -- conv3_x: 33 rounds + 64 tiles -- the same form measured -0.5 % images/s in bf16, +0.2 % in split precision, round 6 on
      // the final tree: the tail it shortens is where the forked edge kernels run. Not used there.)
      int dev = 0, ncu = 0;
      if (g.opt_small != 0 && g.N <= 2 && current_device(dev) == CTPN_OK && device_cu_count(dev, ncu) == CTPN_OK && ncu > 0) {
        const long long t = c3_tiles2d(g, pool, 32) * g.N * ((g.Co + 127) / 128);
        const long long G = t < ncu ? t : ncu, full = t / G, r = t % G;
        if (2 * t <= ncu || (r > 0 && 2 * r <= G && full <= 3))
          return pool ? c3_launch_p<T, false, true, 32, SPLIT, 128, 256, true>(g, s) : c3_launch_p<T, false, false, 32, SPLIT, 128, 256, true>(g, s);
      }
    }
    return pool ? c3_launch_p<T, false, true, 32, SPLIT>(g, s) : c3_launch_p<T, false, false, 32, SPLIT>(g, s);
  }
  if constexpr (SPLIT) {
    return fail(CTPN_ERR_ARG, "conv3x3 (split precision): Co must be <= 64 or a multiple of 128, with ReLU");
  } else {
    if (flat) return c3_launch<T, T, 128, 4, 2, true, false, 2, 3>(g, s);
    if (tw16) return pool ? c3_launch<T, T, 128, 4, 2, false, true, 2, 3, 16>(g, s) : c3_launch<T, T, 128, 4, 2, false, false, 2, 3, 16>(g, s);
    return pool ? c3_launch<T, T, 128, 4, 2, false, true, 2, 3>(g, s) : c3_launch<T, T, 128, 4, 2, false, false, 2, 3>(g, s);
  }
}
}  // namespace ctpn
