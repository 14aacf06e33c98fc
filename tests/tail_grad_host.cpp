// Stand-alone host program over csrc/tail_grad_dev.h, the per-thread text of tail_grad.hip's kernels: built by tests/test_tail_grad.py with
// g++ -ffp-contract=off -fsanitize=address,undefined and run as a subprocess. It runs one whole small problem the way the kernels walk it --
// the recurrence forward (tb_cell_forward) filling a saved block, BPTT against each direction (tb_cell_backward), then the weight-gradient
// products as block partials and the ordered pass (tb_tn_reduce, tb_block_cells) -- from heap blocks of exactly the problem's size, so a
// read or write past an array's end stops the program.
//   tail_grad_host IN OUT [MUTANT]
// IN : int32 rows, T; then float32 x [M][512], pre [M][1024] (x Wx + b, fw | bw, TF gate order), wh [2][128][512], d_lstm_out [M][256]; M = rows T
// OUT: float32 gates [M][2][5][128], lstm_out [M][256], d_pre [M][1024], d_wh [2][128][512], d_wx [2][512][512], d_b [2][512]
// MUTANT (the test asserts each one FAILS the comparison): 1 the f and o derivatives swapped, 2 the forget bias dropped, 3 c_t used for
// c_{t-1}, 4 the bw direction walked left to right.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "tail_grad_dev.h"

using namespace ctpn;

static std::unique_ptr<float[]> block(size_t n) { return std::unique_ptr<float[]>(new float[n]()); }

static void read_all(FILE* f, void* p, size_t bytes) {
  if (fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short read\n"); exit(2); }
}

// out [K][N] = A^T dY in the kernels' order: fma chains over each block's cells from 0, then the blocks' partials left to right
static void tn(const float* a, int lda, int shift, const float* dy, int ldy, long long M, int T, int K, int N, float* out) {
  const long long blk = tb_block_cells(M);
  const int P = (int)((M + blk - 1) / blk);
  std::vector<float> parts((size_t)P);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) {
      for (int p = 0; p < P; ++p) {
        const long long lo = p * blk, hi = lo + blk < M ? lo + blk : M;
        float acc = 0.f;
        for (long long m = lo; m < hi; ++m) {
          const int t = (int)(m % T) + shift;
          const float av = (t >= 0 && t < T) ? a[(size_t)(m + shift) * lda + k] : 0.f;
          acc = fmaf(av, dy[(size_t)m * ldy + n], acc);
        }
        parts[p] = acc;
      }
      out[(size_t)k * N + n] = tb_tn_reduce(parts.data(), P, 1);
    }
}

static void colsum(const float* dy, int ldy, long long M, int N, float* out) {
  const long long blk = tb_block_cells(M);
  const int P = (int)((M + blk - 1) / blk);
  std::vector<float> parts((size_t)P);
  for (int n = 0; n < N; ++n) {
    for (int p = 0; p < P; ++p) {
      const long long lo = p * blk, hi = lo + blk < M ? lo + blk : M;
      parts[p] = tb_colsum_block(dy + (size_t)lo * ldy + n, hi - lo, (size_t)ldy);
    }
    out[n] = tb_tn_reduce(parts.data(), P, 1);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: tail_grad_host IN OUT [MUTANT]\n"); return 2; }
  const int mutant = argc > 3 ? atoi(argv[3]) : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[2];
  read_all(f, hdr, sizeof(hdr));
  const int rows = hdr[0], T = hdr[1];
  const size_t M = (size_t)rows * T;
  auto x = block(M * 512), pre = block(M * 1024), wh = block((size_t)2 * 128 * 512), dlo = block(M * 256);
  read_all(f, x.get(), M * 512 * 4);
  read_all(f, pre.get(), M * 1024 * 4);
  read_all(f, wh.get(), (size_t)2 * 128 * 512 * 4);
  read_all(f, dlo.get(), M * 256 * 4);
  fclose(f);
  auto gates = block(M * 2 * 5 * 128), lstm_out = block(M * 256), d_pre = block(M * 1024);
  auto d_wh = block((size_t)2 * 128 * 512), d_wx = block((size_t)2 * 512 * 512), d_b = block(2 * 512);
  const float forget_bias = mutant == 2 ? 0.f : 1.f;

  for (int dir = 0; dir < 2; ++dir) {
    const float* whd = wh.get() + (size_t)dir * 128 * 512;
    const bool right_to_left = dir == 1 && mutant != 4;
    for (int row = 0; row < rows; ++row) {
      // forward: bilstm.hip's walk, one row at a time
      std::vector<float> h(128, 0.f), c(128, 0.f), hn(128);
      for (int s = 0; s < T; ++s) {
        const int t = right_to_left ? T - 1 - s : s;
        const size_t m = (size_t)row * T + t;
        for (int u = 0; u < 128; ++u) {
          float z[4];
          for (int g = 0; g < 4; ++g) {
            float acc = pre[m * 1024 + dir * 512 + g * 128 + u];
            for (int k = 0; k < 128; ++k) acc = fmaf(whd[(size_t)k * 512 + g * 128 + u], h[k], acc);
            z[g] = acc;
          }
          float gt[4];
          hn[u] = tb_cell_forward(z[0], z[1], z[2], z[3], forget_bias, c[u], gt);
          for (int g = 0; g < 4; ++g) gates[tb_gate_index(m, dir, g, u)] = gt[g];
          gates[tb_gate_index(m, dir, 4, u)] = c[u];
          lstm_out[m * 256 + dir * 128 + u] = hn[u];
        }
        h = hn;
      }
      // backward: bptt_kernel's walk, the direction's last step first
      std::vector<float> dz(512, 0.f), dzn(512), dc(128, 0.f);
      for (int s = T - 1; s >= 0; --s) {
        const int t = right_to_left ? T - 1 - s : s;
        const size_t m = (size_t)row * T + t;
        const size_t mp = right_to_left ? m + 1 : m - 1;      // the step before in the walk (s > 0)
        for (int u = 0; u < 128; ++u) {
          float rec = 0.f;
          for (int cc = 0; cc < 512; ++cc) rec = fmaf(whd[(size_t)u * 512 + cc], dz[cc], rec);
          const float c_t = gates[tb_gate_index(m, dir, 4, u)];
          float c_prev = s > 0 ? gates[tb_gate_index(mp, dir, 4, u)] : 0.f;
          if (mutant == 3) c_prev = c_t;
          float d4[4];
          tb_cell_backward(dlo[m * 256 + dir * 128 + u] + rec, dc[u], gates[tb_gate_index(m, dir, 0, u)], gates[tb_gate_index(m, dir, 1, u)],
                           gates[tb_gate_index(m, dir, 2, u)], gates[tb_gate_index(m, dir, 3, u)], c_t, c_prev, d4);
          if (mutant == 1) { const float sw = d4[2]; d4[2] = d4[3]; d4[3] = sw; }
          for (int g = 0; g < 4; ++g) { dzn[g * 128 + u] = d4[g]; d_pre[m * 1024 + dir * 512 + g * 128 + u] = d4[g]; }
        }
        dz = dzn;
      }
    }
    const float* dp = d_pre.get() + dir * 512;
    tn(x.get(), 512, 0, dp, 1024, (long long)M, T, 512, 512, d_wx.get() + (size_t)dir * 512 * 512);
    tn(lstm_out.get() + dir * 128, 256, dir ? 1 : -1, dp, 1024, (long long)M, T, 128, 512, d_wh.get() + (size_t)dir * 128 * 512);
    colsum(dp, 1024, (long long)M, 512, d_b.get() + dir * 512);
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  fwrite(gates.get(), 4, M * 2 * 5 * 128, o);
  fwrite(lstm_out.get(), 4, M * 256, o);
  fwrite(d_pre.get(), 4, M * 1024, o);
  fwrite(d_wh.get(), 4, (size_t)2 * 128 * 512, o);
  fwrite(d_wx.get(), 4, (size_t)2 * 512 * 512, o);
  fwrite(d_b.get(), 4, 2 * 512, o);
  fclose(o);
  return 0;
}
