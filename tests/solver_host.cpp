// Stand-alone host program over csrc/solver_dev.h, the plan, the parameters and the per-element text of solver.hip's kernels: built by
// tests/test_solver.py with g++ -ffp-contract=off -fsanitize=address,undefined and run as a subprocess. It takes one solver step the way the
// kernels walk the vector -- pass 1 block by block, lane by lane (sv_lane_sums), the block's tree (sv_tree_step), the partials left to right;
// sv_params; pass 2 lane by lane with the segment found once and walked (sv_seg_find, sv_seg_walk, sv_update) -- from heap blocks of exactly
// count floats, so a read or write past an array's end stops the program.
//   solver_host IN OUT [MUTANT]
// IN : int64 solver, count, n_seg, t; double hyper[8]; int64 seg_end[n_seg]; float32 seg_decay[n_seg]; float32 w, g, s1, s2 [count]
// OUT: double out2[2]; float32 w, s1, s2 [count]; exit status 3 and out2 alone if out2[0] is not finite
// MUTANT (the test asserts each one FAILS the comparison): 1 the decay added after the clip, 2 epsilon inside Adam's root, 3 RMS's ms started
// at zero, 4 Adam's bias correction dropped, 5 every inner segment boundary one element early.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "solver_dev.h"

using namespace ctpn;

static int mutant = 0;

static void read_all(FILE* f, void* p, size_t bytes) {
  if (bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short read\n"); exit(2); }
}

static void update(const SvParams& p, float d, float g, float& w, float& s1, float& s2) {
  if (mutant == 1) {
    const float gc = (p.clip_on ? g * p.scale : g) + (d == 0.f ? 0.f : d * w);
    SvParams q = p;
    q.clip_on = 0;
    sv_update(q, 0.f, gc, w, s1, s2);
  } else if (mutant == 2 && p.solver == SV_ADAM) {
    const float ge = sv_ge(g, w, d), gc = p.clip_on ? ge * p.scale : ge;
    s1 = s1 + (gc - s1) * p.one_m_a;
    s2 = s2 + (gc * gc - s2) * p.one_m_b;
    w = w - (s1 * p.lr_t) / sqrtf(s2 + p.eps);
  } else {
    sv_update(p, d, g, w, s1, s2);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: solver_host IN OUT [MUTANT]\n"); return 2; }
  if (argc > 3) mutant = atoi(argv[3]);
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int64_t head[4];
  double hyper[8];
  read_all(f, head, sizeof head);
  read_all(f, hyper, sizeof hyper);
  const int solver = (int)head[0], n_seg = (int)head[2];
  const long long count = head[1], t = head[3];
  if (n_seg < 1 || n_seg > SV_MAX_SEGMENTS || count < 1) return 2;
  std::vector<int64_t> seg_end((size_t)n_seg);
  std::vector<float> seg_decay((size_t)n_seg);
  read_all(f, seg_end.data(), (size_t)n_seg * 8);
  read_all(f, seg_decay.data(), (size_t)n_seg * 4);
  const size_t cz = (size_t)count;
  std::unique_ptr<float[]> w(new float[cz]), g(new float[cz]), s1(new float[cz]), s2(new float[cz]);
  read_all(f, w.get(), cz * 4);
  read_all(f, g.get(), cz * 4);
  read_all(f, s1.get(), cz * 4);
  read_all(f, s2.get(), cz * 4);
  fclose(f);
  SvSegments segs{};
  segs.n = n_seg;
  for (int i = 0; i < n_seg; ++i) {
    segs.end[i] = seg_end[(size_t)i] - (mutant == 5 && i < n_seg - 1 ? 1 : 0);
    segs.decay[i] = seg_decay[(size_t)i];
  }
  if (mutant == 3 && solver == SV_RMS && t == 1) for (size_t e = 0; e < cz; ++e) s1[e] = 0.f;

  long long block;
  int blocks;
  sv_plan(count, block, blocks);
  // pass 1
  double out2[2] = {0.0, 0.0};
  std::vector<double> v_sq(SV_LANES), v_reg(SV_LANES);
  for (int b = 0; b < blocks; ++b) {
    const long long lo = b * block, hi = lo + block < count ? lo + block : count;
    for (int lane = 0; lane < SV_LANES; ++lane) sv_lane_sums(w.get(), g.get(), lo, hi, lane, segs, v_sq[(size_t)lane], v_reg[(size_t)lane]);
    for (int stride = SV_LANES / 2; stride >= 1; stride >>= 1)
      for (int lane = 0; lane < stride; ++lane) { sv_tree_step(v_sq.data(), stride, lane); sv_tree_step(v_reg.data(), stride, lane); }
    out2[0] = out2[0] + v_sq[0];
    out2[1] = out2[1] + v_reg[0];
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  fwrite(out2, sizeof out2, 1, o);
  if (!std::isfinite(out2[0])) { fclose(o); return 3; }
  SvParams p = sv_params(solver, hyper, t, std::sqrt(out2[0]));
  if (mutant == 4) p.lr_t = p.lr;
  // pass 2
  for (int b = 0; b < blocks; ++b) {
    const long long lo = b * block, hi = lo + block < count ? lo + block : count;
    for (int lane = 0; lane < SV_LANES; ++lane) {
      long long e0 = lo + 4LL * lane;
      if (e0 >= hi) continue;
      int seg = sv_seg_find(segs, e0);
      for (; e0 < hi; e0 += 4LL * SV_LANES)
        for (long long e = e0; e < (e0 + 4 < hi ? e0 + 4 : hi); ++e) {
          seg = sv_seg_walk(segs, seg, e);
          update(p, segs.decay[seg], g[(size_t)e], w[(size_t)e], s1[(size_t)e], s2[(size_t)e]);
        }
    }
  }
  fwrite(w.get(), 4, cz, o);
  fwrite(s1.get(), 4, cz, o);
  fwrite(s2.get(), 4, cz, o);
  fclose(o);
  return 0;
}
