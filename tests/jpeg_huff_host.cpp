// TEST INFRASTRUCTURE (never part of the product library): the device Huffman decoder's per-thread source text -- csrc/jpeg_huff_dev.h, what
// the jh_* kernels of jpeg_huff.hip are made of -- compiled for the host with the HIP qualifiers defined away and driven the way the kernels
// and their launcher drive it: every pass a plain loop over thread indices, all threads of a round reading the previous round's states.
// tests/test_jpeg_huff_host.py builds this file with g++ -fsanitize=address,undefined, writes the cases (frame parameters, DHT segments, the
// scan's bytes, the library's host-half result for the same bytes) into a file and runs the program as a child process: on every case,
// damaged ones included, the sanitizers must stay silent and the result must be either a raised flag or the host half's coefficients.
//
// usage: jpeg_huff_host CASEFILE DUMPFILE S [S ...]      exit status 0 = every case held at every S
// DUMPFILE receives, for every case (at the first S), the unstuffed bytes and the segment table, for the Python restatement to compare.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../text-detection-ctpn_amd/csrc/jpeg_huff_dev.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace ctpn;

struct Case {
  int host_status = 0, must_decode = 0;      // the host half's status for these bytes; 1: an undamaged file, the flags must be 0
  int ncomp = 0, mcux = 0, mcuy = 0, dri = 0, hs[3] = {0, 0, 0}, vs[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  struct Dht { int present = 0, nvals = 0; uint8_t counts[16], vals[256]; } dht[2][4];
  std::vector<uint8_t> scan;
  std::vector<int16_t> want;
};

static bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

static bool read_case(FILE* f, Case& c) {
  int32_t hd[18];
  if (!rd(f, hd, sizeof(hd))) return false;
  c.host_status = hd[0]; c.must_decode = hd[1]; c.ncomp = hd[2]; c.mcux = hd[3]; c.mcuy = hd[4]; c.dri = hd[5];
  for (int k = 0; k < 3; ++k) { c.hs[k] = hd[6 + k]; c.vs[k] = hd[9 + k]; c.td[k] = hd[12 + k]; c.ta[k] = hd[15 + k]; }
  for (int cl = 0; cl < 2; ++cl)
    for (int id = 0; id < 4; ++id) {
      int32_t pn[2];
      Case::Dht& d = c.dht[cl][id];
      if (!rd(f, pn, sizeof(pn)) || !rd(f, d.counts, 16) || !rd(f, d.vals, 256)) return false;
      d.present = pn[0]; d.nvals = pn[1];
    }
  int64_t n[2];
  if (!rd(f, n, sizeof(n)) || n[0] < 0 || n[1] < 0 || n[0] > (1 << 28) || n[1] > (1 << 28)) return false;
  c.scan.resize((size_t)n[0]); c.want.resize((size_t)n[1]);
  return rd(f, c.scan.data(), c.scan.size()) && rd(f, c.want.data(), c.want.size() * 2);
}

// the frame in the kernels' form: what jpeg_huff_prepare (jpeg.hip) builds from the parsed frame
static bool make_file(const Case& c, JhFile& F, std::vector<JhTable>& tabs, size_t& ncoef) {
  std::memset(&F, 0, sizeof(F));
  if ((c.ncomp != 1 && c.ncomp != 3) || c.mcux <= 0 || c.mcuy <= 0) return false;
  F.ncomp = c.ncomp; F.mcux = c.mcux; F.mcuy = c.mcuy;
  int slot[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
  long long off = 0;
  for (int k = 0; k < c.ncomp; ++k) {
    F.hs[k] = c.hs[k]; F.vs[k] = c.vs[k]; F.bw[k] = c.mcux * c.hs[k]; F.coef_off[k] = off;
    off += (long long)c.mcuy * c.vs[k] * F.bw[k] * 64;
    for (int q = 0; q < c.hs[k] * c.vs[k]; ++q) { if (F.bpm >= JH_MAX_PATTERN) return false; F.pat_comp[F.bpm++] = (uint8_t)k; }
    for (int cl = 0; cl < 2; ++cl) {
      const int id = cl ? c.ta[k] : c.td[k];
      if (id < 0 || id > 3 || !c.dht[cl][id].present) return false;
      if (slot[cl][id] < 0) {
        tabs.emplace_back();
        if (!jh_build_table(tabs.back(), c.dht[cl][id].counts, c.dht[cl][id].vals, c.dht[cl][id].nvals)) return false;
        slot[cl][id] = (int)tabs.size() - 1;
      }
      (cl ? F.ac_tab : F.dc_tab)[k] = (uint8_t)slot[cl][id];
    }
  }
  ncoef = (size_t)off;
  return true;
}

struct Result { uint32_t flags = 0, rounds = 0, nsub = 0; bool equal = false; };

static Result run_case(const Case& c, uint32_t S, FILE* dump) {
  Result R;
  JhFile F; std::vector<JhTable> tabs; size_t ncoef = 0;
  if (!make_file(c, F, tabs, ncoef)) { R.flags = JH_FLAG_SEGMENTS; return R; }
  tabs.resize(JH_MAX_TABLES);
  const uint32_t total = (uint32_t)c.mcux * (uint32_t)c.mcuy, dri = (uint32_t)c.dri;
  const uint32_t nseg = dri ? (total + dri - 1) / dri : 1u;
  // the host's linear pass, into a block of exactly the size the library stages (ASan guards its ends)
  const size_t raw = c.scan.size(), room = (raw + 3) / 4 * 4 + 8;
  std::vector<uint32_t> words(room / 4, 0u);
  uint8_t* bytes = (uint8_t*)words.data();
  std::vector<JhSeg> segs(nseg);
  uint32_t nb = 0;
  const uint32_t found = (uint32_t)jh_unstuff_segments(c.scan.data(), raw, dri, total, bytes, segs.data(), (int)nseg, &nb);
  if (dump) {
    const uint32_t hd[3] = {nb, found, nseg};
    std::fwrite(hd, 4, 3, dump); std::fwrite(bytes, 1, nb, dump);
    for (uint32_t k = 0; k < found; ++k) { const uint32_t s4[4] = {segs[k].byte0, segs[k].nbits, segs[k].mcu0, segs[k].nmcu}; std::fwrite(s4, 4, 4, dump); }
  }
  if (found < nseg) R.flags |= JH_FLAG_SEGMENTS;
  for (uint32_t k = found; k < nseg; ++k) { JhSeg& s = segs[k]; s.byte0 = nb; s.nbits = 0; s.mcu0 = k * dri; s.nmcu = std::min(dri, total - s.mcu0); }
  F.nwords = (uint32_t)(((nb + 3) / 4 * 4 + 8) / 4);
  uint32_t nsub = 0, cap = 0;
  std::vector<uint32_t> sub_seg;
  for (uint32_t k = 0; k < nseg; ++k) {
    JhSeg& s = segs[k];
    s.file = 0; s.sub0 = nsub; s.nsub = std::max(1u, (s.nbits + S - 1) / S);
    for (uint32_t q = 0; q < s.nsub; ++q) sub_seg.push_back(k);
    nsub += s.nsub; cap = std::max(cap, s.nsub - 1);
  }
  R.nsub = nsub;
  std::vector<JhState> st[2] = {std::vector<JhState>(nsub), std::vector<JhState>(nsub)}, entry(nsub);
  std::vector<uint32_t> begun(nsub, 0), prefix(nsub, 0);
  auto place = [&](uint32_t g, uint32_t& i, uint32_t& start, uint32_t& end) -> const JhSeg& {
    const JhSeg& s = segs[sub_seg[g]];
    i = g - s.sub0;
    const uint64_t a = (uint64_t)i * S, b = a + S;
    start = (uint32_t)std::min<uint64_t>(a, s.nbits); end = (uint32_t)std::min<uint64_t>(b, s.nbits);
    return s;
  };
  // jh_sync_kernel, round 0 .. : one loop iteration per thread
  uint32_t changed = 0, rounds = 0;
  for (uint32_t round = 0; round <= cap; ++round) {
    if (round > 0 && changed + 1 < round) break;            // settled: the launch would return at once (the library stops launching)
    std::vector<JhState>& cur = st[round & 1];
    const std::vector<JhState>& prev = st[(round & 1) ^ 1];
    for (uint32_t g = 0; g < nsub; ++g) {
      uint32_t i, start, end;
      const JhSeg& s = place(g, i, start, end);
      JhState e = jh_fresh(start);
      if (round > 0) {
        if (i > 0) e = prev[g - 1];
        if (jh_same(e, entry[g])) { cur[g] = prev[g]; continue; }
      }
      JhBits bits;
      jh_bits_init(bits, words.data(), F.nwords, s.byte0, s.nbits);
      JhState x = e;
      uint32_t n;
      jh_decode_sub(bits, F, tabs.data(), end, x, n, nullptr, 0);
      entry[g] = e; begun[g] = n; cur[g] = x;
      if (round > 0 && !jh_same(x, prev[g])) changed = round;
    }
    rounds = round;
  }
  R.rounds = rounds;
  const std::vector<JhState>& fin = st[rounds & 1];
  // jh_scan_kernel
  for (uint32_t k = 0; k < nseg; ++k) {
    const JhSeg& s = segs[k];
    uint64_t carry = 0;
    for (uint32_t q = 0; q < s.nsub; ++q) { prefix[s.sub0 + q] = (uint32_t)carry; carry += begun[s.sub0 + q]; }
    const uint64_t need = (uint64_t)s.nmcu * (uint32_t)F.bpm;
    if (carry < need) R.flags |= JH_FLAG_COUNT;
    else if (carry == need && (fin[s.sub0 + s.nsub - 1].bk & 0xffu) != 0) R.flags |= JH_FLAG_OVERRUN;
  }
  // jh_write_kernel: into a block of exactly the frame's size
  std::vector<int16_t> coef(ncoef, 0);
  const uint8_t zz[64] = JH_ZIGZAG_INIT;
  for (uint32_t g = 0; g < nsub; ++g) {
    uint32_t i, start, end;
    const JhSeg& s = place(g, i, start, end);
    JhState x = i > 0 ? fin[g - 1] : jh_fresh(0);
    JhBits bits;
    jh_bits_init(bits, words.data(), F.nwords, s.byte0, s.nbits);
    JhWrite W;
    W.coef = coef.data(); W.zz = zz; W.f = &F; W.mcu0 = s.mcu0; W.seg_blocks = (long long)s.nmcu * F.bpm; W.blk = -1; W.dst = nullptr; W.flags = 0;
    uint32_t n;
    jh_decode_sub(bits, F, tabs.data(), end, x, n, &W, (long long)prefix[g]);
    R.flags |= W.flags;
  }
  // jh_dc_kernel
  for (uint32_t k = 0; k < nseg; ++k)
    for (int cc = 0; cc < F.ncomp; ++cc) {
      const JhSeg& s = segs[k];
      const int hv = F.hs[cc] * F.vs[cc];
      int acc = 0;
      for (uint64_t e = 0; e < (uint64_t)s.nmcu * (uint32_t)hv; ++e) {
        const uint32_t mcu = s.mcu0 + (uint32_t)(e / (uint32_t)hv);
        if (mcu >= total) continue;
        const int j = (int)(e % (uint32_t)hv), by = j / F.hs[cc], bx = j - by * F.hs[cc];
        const int my = (int)(mcu / (uint32_t)F.mcux), mx = (int)(mcu % (uint32_t)F.mcux);
        int16_t* blk = coef.data() + F.coef_off[cc] + ((long long)(my * F.vs[cc] + by) * F.bw[cc] + (mx * F.hs[cc] + bx)) * 64;
        acc += (int)blk[0];
        blk[0] = (int16_t)acc;
      }
    }
  R.equal = c.host_status == 0 && c.want.size() == ncoef && std::memcmp(c.want.data(), coef.data(), ncoef * 2) == 0;
  return R;
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s CASEFILE DUMPFILE S [S ...]\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  FILE* dump = std::fopen(argv[2], "wb");
  if (!f || !dump) { std::fprintf(stderr, "cannot open the case / dump file\n"); return 2; }
  int bad = 0, idx = 0;
  long long decoded = 0, flagged = 0, max_rounds = 0, max_sub = 0;
  for (Case c; read_case(f, c); ++idx) {
    for (int a = 3; a < argc; ++a) {
      const int S = std::atoi(argv[a]);
      if (S < JH_SUBSEQ_MIN || S > JH_SUBSEQ_MAX || S % 32) { std::fprintf(stderr, "bad S %d\n", S); return 2; }
      const Result r = run_case(c, (uint32_t)S, a == 3 ? dump : nullptr);
      const bool ok = c.must_decode ? (r.flags == 0 && r.equal) : (r.flags != 0 || r.equal);
      if (!ok) { ++bad; std::printf("FAIL case %d S %d: flags 0x%x equal %d host status %d rounds %u subsequences %u\n", idx, S, r.flags, (int)r.equal, c.host_status, r.rounds, r.nsub); }
      if (r.flags) ++flagged; else ++decoded;
      max_rounds = std::max<long long>(max_rounds, r.rounds); max_sub = std::max<long long>(max_sub, r.nsub);
    }
  }
  std::fclose(f); std::fclose(dump);
  std::printf("cases %d decoded %lld flagged %lld max_rounds %lld max_subsequences %lld bad %d\n", idx, decoded, flagged, max_rounds, max_sub, bad);
  return bad ? 1 : 0;
}
