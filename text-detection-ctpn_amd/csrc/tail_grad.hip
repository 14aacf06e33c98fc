// The backward pass through the recurrent tail: BiLSTM, lstm_o FC, the two heads (include/ctpn_hip.h, "the recurrent tail: forward with saved
// activations, backward"; the per-thread text, the saved block's layout and the d_tail offsets: tail_grad_dev.h). The forward with saved
// activations is bilstm.hip's own exact-gate kernel body (launch_bilstm_save) between the forward's GEMM launches; the three data-gradient
// products go through launch_igemm on the weights in TF's own layout, which IS the transposed packed layout. New here:
//   bptt_kernel        the backward recurrence. One workgroup = 16 feature-map rows of one direction for all T steps, walked against the
//                      direction; 8 waves, wave w owns hidden units [16w, 16w + 16) and holds the matching 16 rows of Wh ([128 units][512 gate
//                      columns]) in 128 VGPRs per lane for the whole kernel. Per step dh[unit][row] = d_lstm_out + sum_c Wh[unit][c] dz_next[row][c]
//                      as 128 v_mfma_f32_16x16x4_f32 in four independent chains (summed in a fixed order), the C/D layout leaves each lane with the
//                      same 4 units of one row as the forward: the cell backward (tb_cell_backward) is in registers, the cell-state gradient
//                      never leaves the lane; dz goes to d_pre (TF column order) and to an LDS tile [16][512 + 8] for the step before
//   tn_partial_kernel  dW = A^T dY over one block of cells: one wave per 64 x 64 output tile and block, 16 accumulator tiles of
//                      v_mfma_f32_16x16x4_f32 whose k dimension is the cell index -- every element is an fma chain over the block's cells in
//                      ascending order, from 0. `shift` reads A one step away inside the sequence (the Wh gradient's h_{t-1}), 0 at its ends
//   colsum_partial_kernel  the bias gradients: tb_colsum_block over the block's cells
//   tn_reduce_kernel   the ordered pass: element = partial 0 + partial 1 + ... (tb_tn_reduce)
// No atomics: the order of every sum depends on the cell count alone (tb_block_cells).
#include "common.h"
#include "tail_grad_dev.h"

namespace ctpn {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BP_ROWS = 16;               // rows per workgroup of bptt_kernel
constexpr int BP_PITCH = TB_GATES + 8;    // floats per dz row in LDS (2080 B: the forward's conflict-free ds_read_b128 pattern, 32 B past a bank row)

__global__ __launch_bounds__(512) void bptt_kernel(const float* __restrict__ d_lstm_out, const float* __restrict__ gates, const float* __restrict__ tail,
                                                   float* __restrict__ d_pre, int rows, int T) {
  __shared__ __attribute__((aligned(16))) float dzb[BP_ROWS][BP_PITCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y;
  const int r = lane & 15, q4 = lane >> 4;
  // Wh = kernel[512:640] of this direction: [128 units][512 gate columns], TF order
  const float* whd = tail + tb_off_kernel(dir) + (size_t)512 * 512;
  // A operand: areg[qq * 4 + e] = Wh[unit 16 wave + r][c = 16 qq + 4 q4 + e]; the B operand below holds dz_next[row r][the same c]
  float areg[128];
  {
    const float* wrow = whd + (size_t)(16 * wave + r) * 512 + 4 * q4;
#pragma unroll
    for (int qq = 0; qq < 32; ++qq) {
      const f32x4 v = *(const f32x4*)(wrow + 16 * qq);
#pragma unroll
      for (int e = 0; e < 4; ++e) areg[qq * 4 + e] = v[e];
    }
  }
  for (int i = tid; i < BP_ROWS * BP_PITCH; i += 512) (&dzb[0][0])[i] = 0.f;

  // this lane's slot, as in the forward: row r of the block, units u0 .. u0 + 3
  const int row_g = blockIdx.x * BP_ROWS + r;
  const bool row_ok = row_g < rows;
  const int row_c = row_ok ? row_g : rows - 1;
  const int u0 = 16 * wave + 4 * q4;
  const size_t cell0 = (size_t)row_c * T;
  f32x4 dc = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  for (int s = T - 1; s >= 0; --s) {      // against the direction's own walk: its last step first
    const int t = dir ? T - 1 - s : s;
    const size_t m = cell0 + t;
    // the saved activations of this step, and c of the step before it in the direction's walk
    const float* g = gates + tb_gate_index(m, dir, 0, u0);
    f32x4 sv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) sv[k] = *(const f32x4*)(g + k * TB_UNITS);
    f32x4 cp = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) cp = *(const f32x4*)(gates + tb_gate_index(dir ? m + 1 : m - 1, dir, 4, u0));
    const f32x4 dlo = *(const f32x4*)(d_lstm_out + m * 256 + dir * TB_UNITS + u0);
    // dz_next . Wh^T: four chains over c, summed ((0 + 1) + (2 + 3)); dz of the step after is zero at the last step
    f32x4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < 32; ++qq) {
      const f32x4 b = *(const f32x4*)(&dzb[r][16 * qq + 4 * q4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[qq & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[qq * 4 + e], b[e], acc[qq & 3], 0, 0, 0);
    }
    __syncthreads();      // every wave has read the tile of the step after
    f32x4 dz[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float rec = (acc[0][e] + acc[1][e]) + (acc[2][e] + acc[3][e]);
      float dce = dc[e], d4[4];
      tb_cell_backward(dlo[e] + rec, dce, sv[0][e], sv[1][e], sv[2][e], sv[3][e], sv[4][e], cp[e], d4);
      dc[e] = dce;
#pragma unroll
      for (int k = 0; k < 4; ++k) dz[k][e] = d4[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      *(f32x4*)(&dzb[r][k * TB_UNITS + u0]) = dz[k];
      if (row_ok) *(f32x4*)(d_pre + m * 1024 + dir * TB_GATES + k * TB_UNITS + u0) = dz[k];
    }
    __syncthreads();
  }
}

int launch_bptt(const float* d_lstm_out, const float* gates, const float* tail, float* d_pre, int rows, int T, hipStream_t s) {
  if (rows <= 0 || T <= 0) return fail(CTPN_ERR_ARG, "bptt: empty problem");
  hipLaunchKernelGGL(bptt_kernel, dim3((rows + BP_ROWS - 1) / BP_ROWS, 2), dim3(512), 0, s, d_lstm_out, gates, tail, d_pre, rows, T);
  return launch_status("bptt");
}

// ---------------------------------------------------------------------------------------------
// dW = A^T dY. A [M][lda] (K columns from a), dY [M][ldy] (N columns from dy), parts [P][K][N]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tn_partial_kernel(const float* __restrict__ a, int lda, int shift, const float* __restrict__ dy, int ldy, long long M, int T,
                                                        long long block, int K, int N, float* __restrict__ parts) {
  const int lane = threadIdx.x, r = lane & 15, q4 = lane >> 4;
  const int tiles_n = (N + 63) / 64;
  const int k0 = (blockIdx.x / tiles_n) * 64, n0 = (blockIdx.x % tiles_n) * 64;
  const long long m_lo = (long long)blockIdx.y * block, m_hi = m_lo + block < M ? m_lo + block : M;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bool col_ok[4];
  int col_c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { col_ok[j] = n0 + 16 * j + r < N; col_c[j] = col_ok[j] ? n0 + 16 * j + r : N - 1; }
  for (long long mb = m_lo; mb < m_hi; mb += 4) {
    const long long m = mb + q4;      // this lane's cell: k = lane >> 4 of both operands
    const bool m_ok = m < m_hi;
    const long long mc = m_ok ? m : m_hi - 1;
    // A row: the cell `shift` steps away inside the same sequence, zero beyond its ends
    const int t = (int)(mc % T) + shift;
    const bool a_ok = m_ok && t >= 0 && t < T;
    const float* arow = a + (size_t)(a_ok ? mc + shift : mc) * lda + k0 + r;
    const float* brow = dy + (size_t)mc * ldy;
    float av[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float v = arow[16 * i]; av[i] = a_ok ? v : 0.f; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float v = brow[col_c[j]]; bv[j] = (m_ok && col_ok[j]) ? v : 0.f; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
  }
  // C/D: column (lane & 15), rows 4 (lane >> 4) + reg
  float* out = parts + (size_t)blockIdx.y * K * N;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (col_ok[j])
#pragma unroll
        for (int e = 0; e < 4; ++e) out[(size_t)(k0 + 16 * i + 4 * q4 + e) * N + n0 + 16 * j + r] = acc[i][j][e];
}

// parts [P][N]: column sums of dY over each block of cells
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ dy, int ldy, long long M, long long block, int N, float* __restrict__ parts) {
  const long long m_lo = (long long)blockIdx.y * block, m_hi = m_lo + block < M ? m_lo + block : M;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  parts[(size_t)blockIdx.y * N + n] = tb_colsum_block(dy + (size_t)m_lo * ldy + n, m_hi - m_lo, (size_t)ldy);
}

// out[k * ldo + n] = the ordered sum of the P partials of element (k, n)
__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ parts, int P, int K, int N, float* __restrict__ out, int ldo) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)K * N;
  if (e >= total) return;
  const int k = (int)(e / N), n = (int)(e - (size_t)k * N);
  out[(size_t)k * ldo + n] = tb_tn_reduce(parts + e, P, total);
}

int launch_tail_tn(const float* a, int lda, int shift, const float* dy, int ldy, long long M, int T, int K, int N, float* parts, float* out, int ldo, hipStream_t s) {
  if (M <= 0 || T <= 0 || K <= 0 || K % 64 || N <= 0 || shift < -1 || shift > 1) return fail(CTPN_ERR_ARG, "tail_tn: K is a multiple of 64, shift is -1, 0 or 1");
  const long long block = tb_block_cells(M);
  const int P = (int)((M + block - 1) / block);
  hipLaunchKernelGGL(tn_partial_kernel, dim3((K / 64) * ((N + 63) / 64), P), dim3(64), 0, s, a, lda, shift, dy, ldy, M, T, block, K, N, parts);
  if (const int rc = launch_status("tail_tn")) return rc;
  hipLaunchKernelGGL(tn_reduce_kernel, dim3((unsigned)(((size_t)K * N + 255) / 256)), dim3(256), 0, s, parts, P, K, N, out, ldo);
  return launch_status("tail_tn_reduce");
}

int launch_tail_colsum(const float* dy, int ldy, long long M, int N, float* parts, float* out, hipStream_t s) {
  if (M <= 0 || N <= 0) return fail(CTPN_ERR_ARG, "tail_colsum: empty problem");
  const long long block = tb_block_cells(M);
  const int P = (int)((M + block - 1) / block);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3((N + 255) / 256, P), dim3(256), 0, s, dy, ldy, M, block, N, parts);
  if (const int rc = launch_status("tail_colsum")) return rc;
  hipLaunchKernelGGL(tn_reduce_kernel, dim3((N + 255) / 256), dim3(256), 0, s, parts, P, 1, N, out, N);
  return launch_status("tail_colsum_reduce");
}

// ---------------------------------------------------------------------------------------------
// the small copies: d_heads with its pad columns cleared; the two head matrices side by side as [512][64] (= the transposed packed heads matrix)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_dheads_kernel(const float* __restrict__ d_heads, float* __restrict__ out, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) out[i] = tb_mask_dheads(d_heads, i);
}
__global__ __launch_bounds__(64) void heads_rows_kernel(const float* __restrict__ tail, float* __restrict__ out) {
  const int j = blockIdx.x, c = threadIdx.x;
  out[j * 64 + c] = c < 40 ? tail[TB_OFF_WBOX + (size_t)j * 40 + c] : (c < 60 ? tail[TB_OFF_WCLS + (size_t)j * 20 + (c - 40)] : 0.f);
}
int launch_mask_dheads(const float* d_heads, float* out, long long M, hipStream_t s) {
  const size_t total = (size_t)M * 64;
  hipLaunchKernelGGL(mask_dheads_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_heads, out, total);
  return launch_status("mask_dheads");
}
int launch_heads_rows(const float* tail, float* out, hipStream_t s) {
  hipLaunchKernelGGL(heads_rows_kernel, dim3(512), dim3(64), 0, s, tail, out);
  return launch_status("heads_rows");
}

}  // namespace ctpn
