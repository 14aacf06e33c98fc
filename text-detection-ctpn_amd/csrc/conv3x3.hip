// launch_conv3x3: layer-level decisions of the tap-reuse 3x3 convolution (kernels: conv3x3_{tiled,persistent,wr,edge}.h, instantiated per arithmetic type in
// conv3x3_{f32,bf16,f16,split}.hip) -- which kernel family a layer takes, what happens to the ragged pixel columns of a 2D tiling, and the
// per-device resources the kernels share.
//
// Replaces tf.nn.conv2d + bias_add + relu of Network.conv (reference lib/networks/network.py:160-183) and the Network.max_pool that
// follows it where one does (network.py:189-196; VGGnet_test.py:23,26,30,34).
#include "conv3x3_base.h"

namespace ctpn {

// dump pages (where lanes outside the image store, so that every wave issues the same number of stores) and tile-claim counters of the
// weights-in-registers kernel, per device, shared by its bf16 and fp16 instantiations
int c3_wr_resources(int dev, hipStream_t s, char** dump_out, unsigned** claim_out) {
  static char* dump[CTPN_MAX_DEV] = {nullptr};
  static unsigned* claims[CTPN_MAX_DEV] = {nullptr};
  static unsigned ticket[CTPN_MAX_DEV] = {0};
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (!dump[dev]) CTPN_HIP_TRY(hipMalloc((void**)&dump[dev], (size_t)1024 * 4096));
  // tile-claim counters: zero when idle (the kernel re-arms them on exit). Every launch takes the next of 64 slots, so two
  // launches in flight on different streams never share one.
  if (!claims[dev]) {
    CTPN_HIP_TRY(hipMalloc((void**)&claims[dev], 64 * 64 * sizeof(unsigned)));       // 64 launch slots x (8 groups x 4 slices x 2 words)
    // zeroed ON THE LAUNCH STREAM and waited for: the ctx streams are non-blocking, so a plain hipMemset (null stream) is not ordered
    // with the launch that follows -- the first conv1_2 of a process could start claiming tiles from counters that were not zero yet (seen in
    // round 3 as a first forward that differed from the second; a one-time wait, the counters re-arm themselves afterwards)
    CTPN_HIP_TRY(hipMemsetAsync(claims[dev], 0, 64 * 64 * sizeof(unsigned), s));
    CTPN_HIP_TRY(hipStreamSynchronize(s));
  }
  *dump_out = dump[dev];
  *claim_out = claims[dev] + (size_t)(ticket[dev]++ % 64) * 64;
  return CTPN_OK;
}

// Guard of the LDS-DMA helpers' m0 contract (conv3x3_base.h: c3_glds16_saddr declares m0 clobbered, c3_glds16_asm saves and restores it):
// every wave stages `rounds` 1-KiB tiles of `src` into LDS with BOTH forms, interleaved with ordinary LDS traffic and a wave-uniform loop
// the compiler is free to schedule around them, and copies what arrived to out_clobber / out_keep. The two must be the source bytes.
__global__ __launch_bounds__(256) void c3_lds_dma_check_kernel(const char* __restrict__ src, char* __restrict__ out_clobber,
                                                              char* __restrict__ out_keep, int tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  char* a = smem + wave * 2048;          // clobber form lands here
  char* b = a + 1024;                    // save / restore form here
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem + (uint32_t)wave * 2048u;
  for (int t = blockIdx.x * 4 + wave; t < tiles; t += gridDim.x * 4) {
    const int tu = __builtin_amdgcn_readfirstlane(t);                 // wave-uniform by construction; pinned to an SGPR for the "s" operand
    const char* g = src + (size_t)tu * 1024;
    c3_glds16_saddr(g, (uint32_t)lane * 16u, (uint32_t)__builtin_amdgcn_readfirstlane((int)lds0));
    c3_glds16_asm(g + lane * 16, (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds0 + 1024u)));
    c3_wait_vm<0>();
    __builtin_amdgcn_sched_barrier(0);
    const uint4 va = *(const uint4*)(a + lane * 16), vb = *(const uint4*)(b + lane * 16);
    *(uint4*)(out_clobber + (size_t)t * 1024 + lane * 16) = va;
    *(uint4*)(out_keep + (size_t)t * 1024 + lane * 16) = vb;
    __builtin_amdgcn_s_waitcnt(0);       // the LDS reads above are done before the next round's DMA overwrites the tiles
  }
}

int launch_lds_dma_check(const void* src, void* out_clobber, void* out_keep, int tiles, hipStream_t s) {
  if (tiles <= 0) return fail(CTPN_ERR_ARG, "lds_dma_check: no tiles");
  const int grid = tiles < 1024 ? (tiles + 3) / 4 : 256;
  hipLaunchKernelGGL(c3_lds_dma_check_kernel, dim3(grid), dim3(256), 4 * 2048, s, (const char*)src, (char*)out_clobber, (char*)out_keep, tiles);
  CTPN_HIP_TRY(hipGetLastError());
  return CTPN_OK;
}

// conv1_2 as the launch api_forward.hip may hand a q-image to: the weights-in-registers kernel's pooled form without a full-resolution output
bool conv1_fusable(DType t, int n, int h, int w, int ci, int co, bool pool, bool keep_full) {
  return dtype_is_half(t) && ci == 64 && co == 64 && pool && !keep_full && n >= 1;
}

// in/out: bordered NHWC of dtype t; pool_out != nullptr fuses the 2x2/2 VALID max-pool (out may then be nullptr).
// t == SPLIT: ci / co are the layer's channel counts; pixels hold [hi(c) | lo(c)] bf16 planes, weight rows [hi | hi | lo] per tap
// (pack_transpose_split); dup_hi: the output pixel is [hi | lo | hi] (the layer that feeds the LSTM input-projection GEMM).
// q1 / q1_frags (conv1_2 of the 16-bit modes, uint8 feed, production path): conv1_1 is computed inside the launch's window stage from the
// batch's q-image (conv3x3_wr_kernel FUSE); `in` (conv1_1's map) is not touched
// cu_count (test launches, ctpn_debug_conv3x3_walk): the plan and the walk of the main launch as on a device of that many CUs, 1 .. the device's
// own; 0 = the device's, what every product caller passes. The strips do not depend on it.
int launch_conv3x3(const void* in, const void* wt, const float* bias, void* out, void* pool_out, DType t, int n, int h, int w,
                   int ci, int co, int relu, hipStream_t s, int dup_hi, const void* q1, const void* q1_frags, int split_opts, int cu_count) {
  const int bke = (t == DType::F32) ? 32 : 64;
  if (ci <= 0 || ci % bke != 0) return fail(CTPN_ERR_ARG, "conv3x3: Ci must be a multiple of the 128-byte strip");
  const int epc = (t == DType::F32) ? 4 : 8;
  if (co % epc != 0) return fail(CTPN_ERR_ARG, "conv3x3: Co must be a multiple of a 16-byte chunk");
  if (!out && !pool_out) return fail(CTPN_ERR_ARG, "conv3x3: no output");
  if (dup_hi && t != DType::SPLIT) return fail(CTPN_ERR_ARG, "conv3x3: dup_hi is a split-precision layout");
  Conv3 g{};
  g.in = in; g.wt = wt; g.bias = bias; g.out = out; g.pool_out = pool_out;
  g.N = n; g.H = h; g.W = w; g.Ci = ci; g.Co = co; g.relu = relu;
  g.in_pitch = ci; g.out_pitch = co; g.a_wrap = 0; g.dup_hi = 0;
  if (t == DType::SPLIT) {
    if (!bias) return fail(CTPN_ERR_ARG, "conv3x3 (split precision): bias required");
    g.Ci = 3 * ci; g.in_pitch = 2 * ci; g.a_wrap = 2 * ci / 64; g.out_pitch = (dup_hi ? 3 : 2) * co; g.dup_hi = dup_hi ? 1 : 0;
  }
  const bool pool = pool_out != nullptr;
  // Everything that depends on the layer's shape -- the main kernel, which ragged columns go to a strip and through which kernel, in the
  // layer's stream or forked, the edge kernel's K split -- is the plan's (conv3x3_plan.h; ctpn_debug_conv3x3_plan reports the same struct)
  const bool split = t == DType::SPLIT;
  int dev = 0, ncu = 0, rc;
  if ((rc = current_device(dev)) || (rc = device_cu_count(dev, ncu))) return rc;
  if (cu_count < 0 || cu_count > ncu) return fail(CTPN_ERR_ARG, "conv3x3: cu_count is 1 .. the device's CU count, or 0 for the device's");
  if (cu_count) ncu = cu_count;
  const C3Plan plan = c3_plan(t, n, h, w, ci, co, pool, out != nullptr, dup_hi, relu != 0, bias != nullptr, split_opts, ncu);
  if (plan.main_form == C3M_NONE) return fail(CTPN_ERR_ARG, "conv3x3 (split precision): Co must be <= 64 or a multiple of 128, with ReLU");
  const bool strip = plan.strip != C3S_NONE, edge = plan.strip == C3S_EDGE, edge_pool = plan.strip == C3S_EDGE_POOL;
  const int r = plan.strip_cols;
  g.w_cover = plan.w_cover;
  if (q1) {
    if (!conv1_fusable(t, n, h, w, ci, co, pool, out != nullptr) || !q1_frags || strip) return fail(CTPN_ERR_ARG, "conv3x3: the fused conv1_1 form is conv1_2's pooled 16-bit launch");
    g.q1 = q1; g.q1_frags = q1_frags;
  }
  // The strip (a few dozen workgroups) runs on its own stream, forked after the previous layer and joined before the next,
  // so it shares the machine with the main launch instead of adding 35-50 us of a nearly empty GPU per layer.
  // split_opts bit 2 (two forwards overlapping freely on two streams: a measurement mode, api_ctx.hip two_forwards_mode): the machine behind
  // the main launch is not empty then and every fork / join pair is 7 to 13 us of this stream standing still, so the strip follows the main
  // launch in the layer's own stream -- the same kernel in the same form (plan.deep) on the same columns: only the stream differs, the stored
  // bytes cannot.
  static hipStream_t sstream[16] = {nullptr};
  static hipEvent_t ev_fork[16] = {nullptr}, ev_join[16] = {nullptr};
  static std::mutex strip_mu[16];     // the helper stream and its two events are per device, shared by every ctx on it
  std::unique_lock<std::mutex> strip_lock;
  const bool deep = strip && plan.deep != 0;      // the edge kernels' deep form, behind the main launch: no fork, no join
  const bool instream = deep || (strip && (split_opts & 4) != 0);
  auto run_edge = [&](void* dst, bool pooled) -> int {
    hipStream_t es = instream ? s : sstream[dev];
    if (split) return c3_edge_split(in, wt, bias, dst, n, h, w, ci, co, relu, r, pooled, es, true, dup_hi, plan.edge_ks);      // always the deep form
    return t == DType::F16 ? c3_edge_f16(in, wt, bias, dst, n, h, w, ci, co, relu, r, pooled, es, deep)
                           : c3_edge_bf16(in, wt, bias, dst, n, h, w, ci, co, relu, r, pooled, es, deep);
  };
  auto run_strip = [&](hipStream_t es) -> int {
    if (edge_pool) {
      if ((rc = run_edge(pool_out, true))) return rc;
      if (out && (rc = run_edge(out, false))) return rc;
    } else if (edge) {
      if ((rc = run_edge(out, false))) return rc;
    } else {
      IGemm ig{};
      ig.a = in; ig.wt = wt; ig.bias = bias; ig.out = out;
      ig.M = (long long)n * h * r; ig.Ci = ci; ig.ntaps = 9; ig.Co = co;
      ig.a_plain = 0; ig.H = h; ig.W = w; ig.rx0 = w - r; ig.rw = r; ig.out_bordered = 1; ig.ldc = co; ig.relu = relu;
      if ((rc = launch_igemm(ig, t, t, es))) return rc;
    }
    return CTPN_OK;
  };
  if (strip && !instream) {
    strip_lock = std::unique_lock<std::mutex>(strip_mu[dev]);   // held until the join is enqueued (event waits capture the record made before them)
    if (!sstream[dev]) {
      CTPN_HIP_TRY(hipStreamCreateWithFlags(&sstream[dev], hipStreamNonBlocking));
      CTPN_HIP_TRY(hipEventCreateWithFlags(&ev_fork[dev], hipEventDisableTiming));
      CTPN_HIP_TRY(hipEventCreateWithFlags(&ev_join[dev], hipEventDisableTiming));
    }
    CTPN_HIP_TRY(hipEventRecord(ev_fork[dev], s));
    CTPN_HIP_TRY(hipStreamWaitEvent(sstream[dev], ev_fork[dev], 0));
    if ((rc = run_strip(sstream[dev]))) return rc;
    CTPN_HIP_TRY(hipEventRecord(ev_join[dev], sstream[dev]));
  }
  switch (t) {
    case DType::F32: rc = c3_run_f32(g, pool, plan.main_form, s, ncu); break;
    case DType::BF16: rc = c3_run_bf16(g, pool, plan.main_form, s, ncu); break;
    case DType::F16: rc = c3_run_f16(g, pool, plan.main_form, s, ncu); break;
    default: rc = c3_run_split(g, pool, plan.main_form, s, ncu); break;
  }
  if (rc) return rc;
  if (instream) { if ((rc = run_strip(s))) return rc; }
  else if (strip) CTPN_HIP_TRY(hipStreamWaitEvent(s, ev_join[dev], 0));
  return CTPN_OK;
}

}  // namespace ctpn
