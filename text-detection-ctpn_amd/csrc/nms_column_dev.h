// The per-column body of the column-decomposed NMS kernels (nms.hip), one copy: the IoU predicate, "is this lane's candidate suppressed by one of
// the column's kept boxes", the in-chunk greedy resolution, and -- the page form's -- one column's whole greedy pass by one wave. A wave's lanes
// run this text side by side; where they talk to each other it says so through four names:
//   NMS_BALLOT(p)        the 64-bit mask of the lanes whose p holds
//   NMS_READLANE(v, i)   lane i's 32-bit v (i wave-uniform)
//   NMS_FIRSTLANE(v)     a wave-uniform v, as a uniform value
//   NMS_CHUNK_END(sp)    the end of a chunk: what the lanes stored to the kept list (sp: some of it to the spill slice) is what they all load next
// Under hipcc these are the wave64 builtins, and the text compiles to what it was when it stood in nms.hip. Any other compiler gets them from the
// file that includes this one, with float4 / make_float4: tests/page_host.cpp runs a wave as 64 threads that meet at every such point, under
// ASan + UBSan. Nothing here includes a HIP header.
#pragma once

#if defined(__HIPCC__)
#define NMS_DEV __device__ __forceinline__
#define NMS_BALLOT(p) __ballot(p)
#define NMS_READLANE(v, i) __builtin_amdgcn_readlane(v, i)
#define NMS_FIRSTLANE(v) __builtin_amdgcn_readfirstlane(v)
// the spill (global) is read back by this wave only, in later chunks: make the stores visible to its own loads
#define NMS_CHUNK_END(spilled) do { if (spilled) __threadfence_block(); } while (0)
#else
#define NMS_DEV static inline
#endif

namespace ctpn {

NMS_DEV bool iou_gt(const float4& a, float sa, const float4& b, float sb, float thr) {
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float width = fmaxf(right - left + 1.f, 0.f), height = fmaxf(bottom - top + 1.f, 0.f);
  const float inter = width * height;
  return inter / (sa + sb - inter) > thr;
}

// Is this lane's candidate suppressed by one of the column's K kept boxes? (wave-uniform loop, LDS broadcast; beyond(k) fetches the kept box at
// position k >= cap, the LDS capacity: from the spill slice, or the sorted boxes by kept rank)
template <typename Beyond>
NMS_DEV bool nms_kept_suppress(const float4* kept, const float* karea, int cap, int K, const float4& bx, float ar, float thr, Beyond beyond) {
  bool supp = false;
  for (int k = 0; k < K; ++k) {
    float4 kb; float ka;
    if (k < cap) { kb = kept[k]; ka = karea[k]; }
    else { kb = beyond(k); ka = (kb.z - kb.x + 1.f) * (kb.w - kb.y + 1.f); }
    supp = supp || iou_gt(kb, ka, bx, ar, thr);
  }
  return supp;
}

// In-chunk greedy resolution over live candidates, ascending: `alive` = the lanes whose candidate passed the kept list; returns the lanes
// that survive each other too. (Round 5 also measured the two-part form -- the suppression rows of every candidate that passed the kept
// list first, lane i parking row i, then a walk that only reads rows: 100 us against 92 for the proposal layer's launch, 15 against 11 for
// the connector's: the rows of candidates that die inside the chunk are wasted work, and they outnumber what the shorter dependent chain saves.)
NMS_DEV unsigned long long nms_resolve_chunk(const float4& bx, float ar, unsigned long long alive, int lane, float thr) {
  unsigned long long rem = alive;
  while (rem) {
    const int i = NMS_FIRSTLANE(__builtin_ctzll(rem));
    auto rl = [&](float v) { return __builtin_bit_cast(float, NMS_READLANE(__builtin_bit_cast(int, v), i)); };
    const float4 bi = make_float4(rl(bx.x), rl(bx.y), rl(bx.z), rl(bx.w));
    const float ai = rl(ar);
    const bool ov = lane > i && ((alive >> lane) & 1ull) && iou_gt(bi, ai, bx, ar, thr);
    alive &= ~NMS_BALLOT(ov);
    rem = alive & ~((2ull << i) - 1ull);
  }
  return alive;
}

// One column's greedy pass by ONE wave (the page form, nms_page_columns_kernel): its m candidates are the boxes of ranks rank_of(0 .. m - 1),
// ascending, taken 64 at a time against the column's kept boxes -- the first `kcap` of them in kept / karea (the wave's LDS), the rest in
// spill[kcap .. m), the column's own slice -- and then against each other. mark(rank) is called once by the lane of every survivor.
template <typename RankOf, typename Mark>
NMS_DEV void nms_column_greedy(const float4* boxes, RankOf rank_of, int m, float4* kept, float* karea, int kcap, float4* spill, float thr, int lane, Mark mark) {
  const unsigned long long lt = (1ull << lane) - 1ull;
  int K = 0;
  for (int cb = 0; cb < m; cb += 64) {
    const int ci = cb + lane;
    const bool valid = ci < m;
    const int rank = valid ? rank_of(ci) : 0;
    const float4 bx = valid ? boxes[rank] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float ar = (bx.z - bx.x + 1.f) * (bx.w - bx.y + 1.f);
    const bool supp = nms_kept_suppress(kept, karea, kcap, K, bx, ar, thr, [&](int k) { return spill[k]; });
    const unsigned long long alive = nms_resolve_chunk(bx, ar, NMS_BALLOT(valid && !supp), lane, thr);
    if ((alive >> lane) & 1ull) {
      const int pos = K + __builtin_popcountll(alive & lt);      // < m: inside the column's slice
      if (pos < kcap) { kept[pos] = bx; karea[pos] = ar; }
      else spill[pos] = bx;
      mark(rank);
    }
    K += __builtin_popcountll(alive);
    NMS_CHUNK_END(K > kcap);
  }
}

}  // namespace ctpn
