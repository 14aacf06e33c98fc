// The backward pass through the recurrent tail (include/ctpn_hip.h, "the recurrent tail: forward with saved activations, backward"): the
// per-thread text of tail_grad.hip's kernels as host + device functions. The kernels call these bodies with their own indices;
// tests/tail_grad_host.cpp compiles this same text with g++ under ASan + UBSan (-ffp-contract=off, as the Makefile gives tail_grad.hip) and
// calls it from loops over whole small problems.
//   tb_cell_backward  one (row, step, unit) of BPTT through the TF-1.3 LSTMCell (bilstm.hip's header: c_t = f c_{t-1} + i j, h_t = o tanh(c_t),
//                     f = sigmoid(z_f + 1.0)) from the SAVED activations: dh and the cell-state gradient carried from the step after ->
//                     the four pre-activation gradients (TF order i, j, f, o) and the carry for the step before
//   tb_cell_forward   the same cell forward, in bilstm.hip's exact-gate forms. The device's saving recurrence is bilstm.hip's own kernel body;
//                     this copy is what the host program builds its saved block with, so that a whole problem runs without a device
//   tb_tn_reduce      one output element of dW = A^T dY: the ordered pass over the partial sums of the cell blocks
//   tb_block_cells    how many cells one partial covers: a function of the cell count alone
//   tb_colsum_block   one column of a bias gradient over one block of cells
//   tb_mask_dheads    one element of d_heads with the pad columns cleared
// The saved block's layout (TB_SAVED_*), the d_tail offsets (TB_OFF_*). Nothing here includes a HIP header.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TB_HD __host__ __device__ inline
#else
#define TB_HD inline
#endif

namespace ctpn {

constexpr int TB_UNITS = 128;                 // hidden units per direction
constexpr int TB_GATES = 4 * TB_UNITS;        // gate columns per direction, TF order i | j | f | o
constexpr int TB_TAIL_FLOATS = 818748;        // CTPN_TAIL_FLOATS
// d_tail / tail: the arena's last ten tensors
TB_HD size_t tb_off_kernel(int d) { return (size_t)d * (640 * 512 + 512); }               // direction d's [640][512]: rows 0..511 Wx, 512..639 Wh
TB_HD size_t tb_off_bias(int d) { return (size_t)d * (640 * 512 + 512) + 640 * 512; }     // [512]
constexpr size_t TB_OFF_WFC = 2 * (640 * 512 + 512);                       // [256][512]
constexpr size_t TB_OFF_BFC = TB_OFF_WFC + 256 * 512;                      // [512]
constexpr size_t TB_OFF_WBOX = TB_OFF_BFC + 512;                           // [512][40]
constexpr size_t TB_OFF_BBOX = TB_OFF_WBOX + 512 * 40;                     // [40]
constexpr size_t TB_OFF_WCLS = TB_OFF_BBOX + 40;                           // [512][20]
constexpr size_t TB_OFF_BCLS = TB_OFF_WCLS + 512 * 20;                     // [20]
static_assert(TB_OFF_BCLS + 20 == TB_TAIL_FLOATS, "the ten tensors are 818748 floats");

// saved block of M = n hf wf cells: lstm_out [M][256] | lstm_o [M][512] | gates [M][2 directions][5: i, j, f, o, c][128], 2048 floats per cell
constexpr int TB_SAVED_PER_CELL = 256 + 512 + 2 * 5 * TB_UNITS;
TB_HD size_t tb_saved_lstm_out(size_t) { return 0; }
TB_HD size_t tb_saved_lstm_o(size_t M) { return M * 256; }
TB_HD size_t tb_saved_gates(size_t M) { return M * (256 + 512); }
// gate g (0..3 = i, j, f, o; 4 = the cell state c) of direction d at cell m, unit u, relative to tb_saved_gates
TB_HD size_t tb_gate_index(size_t m, int d, int g, int u) { return ((m * 2 + (size_t)d) * 5 + (size_t)g) * TB_UNITS + (size_t)u; }

// cells per partial sum of the weight-gradient reductions: 256, doubled until at most 32 partials cover the M cells
constexpr int TB_BLOCK_MIN = 256;
constexpr int TB_MAX_PARTIALS = 32;
TB_HD long long tb_block_cells(long long M) {
  long long b = TB_BLOCK_MIN;
  while ((M + b - 1) / b > TB_MAX_PARTIALS) b *= 2;
  return b;
}

TB_HD float tb_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
TB_HD float tb_tanh(float x) { return 1.f - 2.f / (expf(2.f * x) + 1.f); }

// forward: the four pre-activations -> the activated gates; c: c_{t-1} in, c_t out; returns h_t
TB_HD float tb_cell_forward(float zi, float zj, float zf, float zo, float forget_bias, float& c, float (&gates)[4]) {
  const float ig = tb_sigmoid(zi), jg = tb_tanh(zj), fg = tb_sigmoid(zf + forget_bias), og = tb_sigmoid(zo);
  const float cn = fg * c + ig * jg;
  c = cn;
  gates[0] = ig; gates[1] = jg; gates[2] = fg; gates[3] = og;
  return og * tb_tanh(cn);
}

// backward of one cell. dh: the gradient at h_t (from lstm_out and from the step after through Wh); dc: the gradient at c_t carried from the
// step after, in; the gradient at c_{t-1}, out. ig .. og, c_t, c_prev (0 at the direction's first step): the saved block's values
TB_HD void tb_cell_backward(float dh, float& dc, float ig, float jg, float fg, float og, float c_t, float c_prev, float (&dz)[4]) {
  const float tc = tanhf(c_t);      // the library's tanh: the forward's expf form loses relative accuracy near 0, and nothing here has to match its bits
  const float d_o = dh * tc;
  const float dct = dc + dh * og * (1.f - tc * tc);
  dz[0] = dct * jg * (ig * (1.f - ig));
  dz[1] = dct * ig * (1.f - jg * jg);
  dz[2] = dct * c_prev * (fg * (1.f - fg));
  dz[3] = d_o * (og * (1.f - og));
  dc = dct * fg;
}

// out element = partial[0] + partial[1] + ... + partial[P - 1], left to right; partial p of the element is at parts[p * stride]
TB_HD float tb_tn_reduce(const float* parts, int P, size_t stride) {
  float acc = parts[0];
  for (int p = 1; p < P; ++p) acc = acc + parts[(size_t)p * stride];
  return acc;
}

// a bias gradient over one block of cells: eight interleaved running sums (cell m into sum m & 7, ascending), then ((0 + 1) + (2 + 3)) +
// ((4 + 5) + (6 + 7)); `first` is the block's first cell's value, `stride` floats from one cell to the next
TB_HD float tb_colsum_block(const float* first, long long cells, size_t stride) {
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long m = 0; m < cells; ++m) s[m & 7] = s[m & 7] + first[(size_t)m * stride];
  return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// d_heads row of 64: columns 60..63 are not read
TB_HD float tb_mask_dheads(const float* d_heads, size_t idx) { return (idx & 63) < 60 ? d_heads[idx] : 0.f; }

}  // namespace ctpn
