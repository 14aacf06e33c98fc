// c3_dispatch: the launch of the kernel family (conv3x3_tiled.h, conv3x3_persistent.h) that the layer's plan names.
#pragma once
#include "conv3x3_tiled.h"
#include "conv3x3_persistent.h"
namespace ctpn {

// form: C3Plan::main_form (conv3x3_plan.h, where the rules and their measurements are). Co <= 64 (conv1_2 outside the 16-bit modes'
// weights-in-registers kernel): the non-persistent kernel on 256 x 64 tiles, or the persistent kernel's 64-channel form in split precision;
// Co % 128 == 0 with ReLU (every other layer of the network): persistent workgroups, flat windows where the map is small enough, else 8 x 32
// or 16 x 16 patches; anything else (debug entry point): non-persistent 256 x 128 tiles.
template <typename T, bool SPLIT = false>
static int c3_dispatch(const Conv3& g, bool pool, int form, hipStream_t s, int ncu) {
  // ncu: the CU count the launch is laid out for (launch_conv3x3: the device's, or a test launch's override). The persistent forms' walk:
  const C3Walk wk = c3_walk(form, g.N, g.H, g.W, g.Co, pool, g.out != nullptr, g.w_cover, ncu);
  using OT = typename std::conditional<SPLIT, float, T>::type;      // staging type of the non-persistent kernel's LDS epilogue
  switch (form) {
    case C3M_P64:
      if constexpr (SPLIT) return pool ? c3_launch_p<T, false, true, 32, SPLIT, 64>(g, s, wk) : c3_launch_p<T, false, false, 32, SPLIT, 64>(g, s, wk);
      break;
    case C3M_T64:
      return pool ? c3_launch<T, OT, 64, 4, 1, false, true, 2, 3, 32, SPLIT>(g, s) : c3_launch<T, OT, 64, 4, 1, false, false, 2, 3, 32, SPLIT>(g, s);
    case C3M_P_FLAT64:
      if (!pool) return c3_launch_p<T, true, false, 32, SPLIT, 128, 64>(g, s, wk);
      break;
    case C3M_P_FLAT:
      if (!pool) return c3_launch_p<T, true, false, 32, SPLIT>(g, s, wk);
      break;
    case C3M_P_16X16:
      return pool ? c3_launch_p<T, false, true, 16, SPLIT>(g, s, wk) : c3_launch_p<T, false, false, 16, SPLIT>(g, s, wk);
    case C3M_P_8X32_HALF:
      return pool ? c3_launch_p<T, false, true, 32, SPLIT, 128, 256, true>(g, s, wk) : c3_launch_p<T, false, false, 32, SPLIT, 128, 256, true>(g, s, wk);
    case C3M_P_8X32:
      return pool ? c3_launch_p<T, false, true, 32, SPLIT>(g, s, wk) : c3_launch_p<T, false, false, 32, SPLIT>(g, s, wk);
    case C3M_T_FLAT:
      if constexpr (!SPLIT) { if (!pool) return c3_launch<T, T, 128, 4, 2, true, false, 2, 3>(g, s); }
      break;
    case C3M_T_16X16:
      if constexpr (!SPLIT) return pool ? c3_launch<T, T, 128, 4, 2, false, true, 2, 3, 16>(g, s) : c3_launch<T, T, 128, 4, 2, false, false, 2, 3, 16>(g, s);
      break;
    case C3M_T_8X32:
      if constexpr (!SPLIT) return pool ? c3_launch<T, T, 128, 4, 2, false, true, 2, 3>(g, s) : c3_launch<T, T, 128, 4, 2, false, false, 2, 3>(g, s);
      break;
    default: break;
  }
  return fail(CTPN_ERR_ARG, "conv3x3: the plan names no kernel of this precision");
}
}  // namespace ctpn
