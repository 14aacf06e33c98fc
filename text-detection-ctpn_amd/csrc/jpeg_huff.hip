// JPEG Huffman streams -> quantised DCT coefficients on the device: the kernels around jpeg_huff_dev.h's per-thread decode (the algorithm
// is described there). One thread per subsequence, JH_WG subsequences of ONE file per workgroup (the host pads every file's subsequences to a
// multiple of JH_WG), so that a workgroup keeps its file's Huffman tables in LDS: 6 x 1336 bytes, read at a random index per code, which
// LDS serves per lane and the vector cache would serve per line. Order between workgroups comes from kernel boundaries alone: no kernel here
// waits on a flag another workgroup sets. Every loop is bounded before it starts (bits of a subsequence, subsequences / blocks of a segment).
// What bounds the kernels: the decode is a chain of dependent LDS lookups and shifts per code with every lane of a wave at its own place in
// its own loop -- latency- and divergence-bound, not bandwidth-bound; the rate comes from the number of subsequences in flight.
#include "common.h"
#include "wg_scan.h"

namespace ctpn {

enum { JH_WG = 256 };

struct JhShared {
  JhTable tabs[JH_MAX_TABLES];
  JhFile file;
  uint8_t zz[64];
  uint32_t go;
};

__constant__ uint8_t jh_zz_const[64] = JH_ZIGZAG_INIT;

// the workgroup's file and its tables into LDS; false (for the whole workgroup) if the workgroup has no file
static __device__ __forceinline__ void jh_load_shared(const JhBatchDev& B, JhShared& sh, uint32_t fi) {
  const uint32_t tid = threadIdx.x;
  const JhFile* gf = B.files + fi;
  const uint32_t* src = (const uint32_t*)gf;
  uint32_t* dst = (uint32_t*)&sh.file;
  for (uint32_t i = tid; i < sizeof(JhFile) / 4; i += JH_WG) dst[i] = src[i];
  if (tid < 64) sh.zz[tid] = jh_zz_const[tid];
  const uint32_t ntab = min(gf->ntab, (uint32_t)JH_MAX_TABLES);
  const uint32_t* ts = (const uint32_t*)(B.tabs + gf->tab0);
  uint32_t* td = (uint32_t*)sh.tabs;
  for (uint32_t i = tid; i < ntab * (uint32_t)(sizeof(JhTable) / 4); i += JH_WG) td[i] = ts[i];
}

// a subsequence's place: its segment, index inside it, first and last bit
struct JhPlace { const JhSeg* seg; uint32_t i, start, end; };
static __device__ __forceinline__ bool jh_place(const JhBatchDev& B, uint32_t g, JhPlace& pl) {
  if (g >= B.nsub) return false;
  const uint32_t si = B.sub_seg[g];
  if (si >= B.nseg) return false;                       // padding behind a file's last subsequence
  pl.seg = B.segs + si;
  if (g < pl.seg->sub0 || g - pl.seg->sub0 >= pl.seg->nsub) return false;
  pl.i = g - pl.seg->sub0;
  const uint64_t s = (uint64_t)pl.i * B.S, e = s + B.S;
  pl.start = (uint32_t)min(s, (uint64_t)pl.seg->nbits);
  pl.end = (uint32_t)min(e, (uint64_t)pl.seg->nbits);
  return true;
}

// round 0: pass 1, every subsequence from its first bit with a fresh state. round r >= 1: subsequence i from the exit state round r - 1
// stored for i - 1 (the other buffer: all threads of a round read the previous round's states). A file none of whose states changed in
// round r - 1 is settled: its workgroups return at once (changed[file] = the last round that changed a state, read here, written for the
// NEXT launch to read). A thread whose entry state is the one it decoded from last time copies its exit state instead of decoding again.
__global__ __launch_bounds__(JH_WG) void jh_sync_kernel(JhBatchDev B, int round) {
  __shared__ JhShared sh;
  const uint32_t fi = B.wg_file[blockIdx.x];
  if (fi >= B.nfiles) return;
  if (threadIdx.x == 0) sh.go = round == 0 || B.changed[fi] + 1u >= (uint32_t)round;
  __syncthreads();
  if (!sh.go) return;
  jh_load_shared(B, sh, fi);
  __syncthreads();
  const uint32_t g = blockIdx.x * JH_WG + threadIdx.x;
  JhPlace pl;
  if (!jh_place(B, g, pl)) return;
  JhState* cur = B.st[round & 1];
  const JhState* prev = B.st[(round & 1) ^ 1];
  JhState e = jh_fresh(pl.start);
  if (round > 0) {
    if (pl.i > 0) e = prev[g - 1];
    if (jh_same(e, B.entry[g])) { cur[g] = prev[g]; return; }
  }
  JhBits bits;
  jh_bits_init(bits, (const uint32_t*)(B.bytes + sh.file.bytes_off), sh.file.nwords, pl.seg->byte0, pl.seg->nbits);
  JhState x = e;
  uint32_t begun;
  jh_decode_sub(bits, sh.file, sh.tabs, pl.end, x, begun, nullptr, 0);
  B.entry[g] = e;
  B.begun[g] = begun;
  cur[g] = x;
  if (round > 0 && !jh_same(x, prev[g])) B.changed[fi] = (uint32_t)round;      // every writer of a round stores the same value
}

static_assert(JH_WG == 256, "wg_scan256 scans a workgroup of 256");

// one workgroup per segment: exclusive scan of the blocks begun per subsequence, JH_WG at a time with a carry; then the segment's checks
__global__ __launch_bounds__(JH_WG) void jh_scan_kernel(JhBatchDev B, int fin) {
  const JhSeg seg = B.segs[blockIdx.x];
  if (seg.file >= B.nfiles) return;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < seg.nsub; base += JH_WG) {
    const uint32_t i = base + threadIdx.x;
    const bool in = i < seg.nsub && seg.sub0 + i < B.nsub;
    const uint32_t v = in ? B.begun[seg.sub0 + i] : 0u;
    uint32_t total;
    const uint32_t incl = wg_scan256(v, total);
    if (in) B.prefix[seg.sub0 + i] = carry + (incl - v);
    carry += total;
    __syncthreads();      // wg_scan256's second barrier
  }
  if (threadIdx.x == 0 && seg.nsub > 0 && seg.sub0 + seg.nsub <= B.nsub) {
    const uint64_t need = (uint64_t)seg.nmcu * (uint32_t)B.files[seg.file].bpm;
    const JhState last = B.st[fin][seg.sub0 + seg.nsub - 1];
    uint32_t fl = 0;
    if (carry < need) fl = JH_FLAG_COUNT;
    else if (carry == need && (last.bk & 0xffu) != 0) fl = JH_FLAG_OVERRUN;      // the last block is still open at the segment's end
    if (fl) atomicOr(&B.flags[seg.file], fl);
  }
}

// every subsequence once more from its settled entry state, storing the coefficients of the codes that start in it
__global__ __launch_bounds__(JH_WG) void jh_write_kernel(JhBatchDev B, int fin) {
  __shared__ JhShared sh;
  const uint32_t fi = B.wg_file[blockIdx.x];
  if (fi >= B.nfiles) return;
  jh_load_shared(B, sh, fi);
  __syncthreads();
  const uint32_t g = blockIdx.x * JH_WG + threadIdx.x;
  JhPlace pl;
  if (!jh_place(B, g, pl)) return;
  JhState x = pl.i > 0 ? B.st[fin][g - 1] : jh_fresh(0);
  JhBits bits;
  jh_bits_init(bits, (const uint32_t*)(B.bytes + sh.file.bytes_off), sh.file.nwords, pl.seg->byte0, pl.seg->nbits);
  JhWrite W;
  W.coef = B.coef + sh.file.coef_base; W.zz = sh.zz; W.f = &sh.file; W.mcu0 = pl.seg->mcu0;
  W.seg_blocks = (long long)pl.seg->nmcu * sh.file.bpm; W.blk = -1; W.dst = nullptr; W.flags = 0;
  uint32_t begun;
  jh_decode_sub(bits, sh.file, sh.tabs, pl.end, x, begun, &W, (long long)B.prefix[g]);
  if (W.flags) atomicOr(&B.flags[fi], W.flags);
}

// one workgroup per (segment, component): the DC differences of the component's blocks, in scan order, summed in 32 bits and truncated to
// int16 at the store, as pred[c] is on the host; JH_WG blocks at a time with a carry
__global__ __launch_bounds__(JH_WG) void jh_dc_kernel(JhBatchDev B) {
  const JhSeg seg = B.segs[blockIdx.x / 3];
  const int c = blockIdx.x % 3;
  if (seg.file >= B.nfiles) return;
  const JhFile& f = B.files[seg.file];
  if (c >= f.ncomp) return;
  const int hs = f.hs[c], vs = f.vs[c], hv = hs * vs, bw = f.bw[c], mcux = f.mcux;
  const uint32_t mcus = (uint32_t)f.mcux * (uint32_t)f.mcuy;
  const uint64_t n = (uint64_t)seg.nmcu * (uint32_t)hv;
  int16_t* comp = B.coef + f.coef_base + f.coef_off[c];
  int carry = 0;
  for (uint64_t base = 0; base < n; base += JH_WG) {
    const uint64_t e = base + threadIdx.x;
    int16_t* blk = nullptr;
    if (e < n) {
      const uint32_t mcu = seg.mcu0 + (uint32_t)(e / (uint32_t)hv);
      const int j = (int)(e % (uint32_t)hv), by = j / hs, bx = j - by * hs;
      if (mcu < mcus) {
        const int my = (int)(mcu / (uint32_t)mcux), mx = (int)(mcu - (uint32_t)my * (uint32_t)mcux);
        blk = comp + ((long long)(my * vs + by) * bw + (mx * hs + bx)) * 64;
      }
    }
    const int v = blk ? (int)blk[0] : 0;
    uint32_t total;      // (two's complement: the unsigned scan is exact for the differences)
    const int incl = (int)wg_scan256((uint32_t)v, total);
    if (blk) blk[0] = (int16_t)(carry + incl);
    carry += (int)total;
    __syncthreads();      // wg_scan256's second barrier
  }
}

static int jh_grid_ok(const JhBatchDev& B) {
  if (B.nsub == 0 || B.nsub % JH_WG || B.nseg == 0 || B.nseg > 0x2fffffffu || B.nfiles == 0) return fail(CTPN_ERR_ARG, "jpeg_huff: bad batch descriptor");
  return CTPN_OK;
}

int jpeg_huff_workgroup() { return JH_WG; }

int launch_jpeg_huff_round(const JhBatchDev& B, int round, hipStream_t s) {
  if (jh_grid_ok(B) || round < 0) return fail(CTPN_ERR_ARG, "jpeg_huff: bad batch descriptor");
  hipLaunchKernelGGL(jh_sync_kernel, dim3(B.nsub / JH_WG), dim3(JH_WG), 0, s, B, round);
  return launch_status("jpeg_huff");
}

// after `rounds` sync rounds: scan, write pass, DC pass. The coefficient block must be zero (the caller clears it on the same queue)
int launch_jpeg_huff_write(const JhBatchDev& B, int rounds, hipStream_t s) {
  if (jh_grid_ok(B) || rounds < 0) return fail(CTPN_ERR_ARG, "jpeg_huff: bad batch descriptor");
  const int fin = rounds & 1;
  hipLaunchKernelGGL(jh_scan_kernel, dim3(B.nseg), dim3(JH_WG), 0, s, B, fin);
  hipLaunchKernelGGL(jh_write_kernel, dim3(B.nsub / JH_WG), dim3(JH_WG), 0, s, B, fin);
  hipLaunchKernelGGL(jh_dc_kernel, dim3(B.nseg * 3u), dim3(JH_WG), 0, s, B);
  return launch_status("jpeg_huff");
}

}  // namespace ctpn
