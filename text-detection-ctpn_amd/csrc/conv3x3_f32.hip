// conv3x3 kernels instantiated for exact-fp32 MFMAs (CTPN_PREC_FP32: the correctness-gate path), see conv3x3_base.h
#include "conv3x3_dispatch.h"
namespace ctpn {
int c3_run_f32(const Conv3& g, bool pool, int form, hipStream_t s, int ncu) { return c3_dispatch<float>(g, pool, form, s, ncu); }
}  // namespace ctpn
