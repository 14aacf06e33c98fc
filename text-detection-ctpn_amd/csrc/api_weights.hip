// C ABI of libctpn_hip.so, weights unit: the manifest of the flat fp32 arena, packing into the kernels' layouts, the RCCL broadcast.
#include "ctx.h"

namespace ctpn {

struct ManifestEntry { std::string name; int rank; int shape[4]; size_t offset; size_t count; };
static std::vector<ManifestEntry> build_manifest() {
  std::vector<ManifestEntry> m;
  size_t off = 0;
  auto add = [&](const std::string& name, int rank, int a, int b, int c, int d) {
    ManifestEntry e; e.name = name; e.rank = rank; e.shape[0] = a; e.shape[1] = b; e.shape[2] = c; e.shape[3] = d;
    e.offset = off; e.count = (size_t)a * (rank > 1 ? b : 1) * (rank > 2 ? c : 1) * (rank > 3 ? d : 1);
    off += e.count; m.push_back(e);
  };
  for (const auto& c : kConvs) {
    add(std::string(c.name) + "/weights", 4, 3, 3, c.ci, c.co);
    add(std::string(c.name) + "/biases", 1, c.co, 1, 1, 1);
  }
  add("lstm_o/bidirectional_rnn/fw/lstm_cell/kernel", 2, 640, 512, 1, 1);
  add("lstm_o/bidirectional_rnn/fw/lstm_cell/bias", 1, 512, 1, 1, 1);
  add("lstm_o/bidirectional_rnn/bw/lstm_cell/kernel", 2, 640, 512, 1, 1);
  add("lstm_o/bidirectional_rnn/bw/lstm_cell/bias", 1, 512, 1, 1, 1);
  add("lstm_o/weights", 2, 256, 512, 1, 1);
  add("lstm_o/biases", 1, 512, 1, 1, 1);
  add("rpn_bbox_pred/weights", 2, 512, 40, 1, 1);
  add("rpn_bbox_pred/biases", 1, 40, 1, 1, 1);
  add("rpn_cls_score/weights", 2, 512, 20, 1, 1);
  add("rpn_cls_score/biases", 1, 20, 1, 1, 1);
  return m;
}
static const std::vector<ManifestEntry>& manifest() {
  static const std::vector<ManifestEntry> m = build_manifest();
  return m;
}
static const ManifestEntry* find_entry(const std::string& name) {
  for (const auto& e : manifest()) if (e.name == name) return &e;
  return nullptr;
}

// ---------------------------------------------------------------------------------------------
int pack_lstm_projection(const float* const kx[2], long long kx_ld, const float* const bias[2], DType prec, void* wt_x, size_t row_bytes, float* b_x,
                         void* wt_xf, hipStream_t s) {
  int rc;
  for (int d = 0; d < 2; ++d) {
    // kernel[:512] ([512 in][512 gates]) -> wt_x rows d*512.. ([gate][in]; split precision: [gate][hi | hi | lo] against [hi | lo | hi] pixels)
    char* dst = (char*)wt_x + (size_t)d * 512 * row_bytes;
    if (prec == DType::SPLIT) { if ((rc = launch_pack_transpose_split(kx[d], kx_ld, dst, 1, 512, 512, s))) return rc; }
    else if ((rc = launch_pack_transpose(kx[d], kx_ld, dst, 512, prec, 512, 512, s))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(b_x + d * 512, bias[d], 512 * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  // gate columns of lstm_pre in the recurrence kernel's order (bilstm.hip: a lane's 4 gates x 4 units = one 64-byte run): permute
  // the rows of the packed [1024][512] input-projection matrix and its bias once, here
  const size_t wbytes = (size_t)1024 * row_bytes;
  DevBuf tmp_buf;      // released on every way out (the release waits for what s still does with it)
  if ((rc = tmp_buf.alloc(wbytes))) return rc;
  void* tmp = tmp_buf.get();
  CTPN_HIP_TRY(hipMemcpyAsync(tmp, wt_x, wbytes, hipMemcpyDeviceToDevice, s));
  if ((rc = launch_lstm_permute_rows(tmp, wt_x, (int)row_bytes, s))) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(tmp, b_x, 1024 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if ((rc = launch_lstm_permute_rows(tmp, b_x, 4, s))) return rc;
  if (wt_xf && (rc = launch_lstm_pre_pack(wt_x, wt_xf, s))) return rc;
  CTPN_HIP_TRY(hipStreamSynchronize(s));
  return CTPN_OK;
}

static int pack_weights(ctpn_ctx* c) {
  hipStream_t s = c->stream;
  const float* A = c->arena;
  int rc;
  for (int i = 0; i < 14; ++i) {
    const ManifestEntry* we = find_entry(std::string(kConvs[i].name) + "/weights");
    const ManifestEntry* be = find_entry(std::string(kConvs[i].name) + "/biases");
    CTPN_HIP_TRY(hipMemcpyAsync(c->b_conv[i], A + be->offset, be->count * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (i == 0) {
      CTPN_HIP_TRY(hipMemcpyAsync(c->w_first, A + we->offset, we->count * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else {
      const int K = 9 * kConvs[i].ci, Co = kConvs[i].co;
      // HWIO [K][Co] -> [Co][K] (split precision: [Co][9][hi(Ci) | hi(Ci) | lo(Ci)])
      if (c->prec == DType::SPLIT) { if ((rc = launch_pack_transpose_split(A + we->offset, Co, c->wt_conv[i], 9, kConvs[i].ci, Co, s))) return rc; }
      else if ((rc = launch_pack_transpose(A + we->offset, Co, c->wt_conv[i], K, c->prec, K, Co, s))) return rc;
    }
  }
  {
    const ManifestEntry* kf = find_entry("lstm_o/bidirectional_rnn/fw/lstm_cell/kernel");
    const ManifestEntry* kb = find_entry("lstm_o/bidirectional_rnn/bw/lstm_cell/kernel");
    const ManifestEntry* bf = find_entry("lstm_o/bidirectional_rnn/fw/lstm_cell/bias");
    const ManifestEntry* bb = find_entry("lstm_o/bidirectional_rnn/bw/lstm_cell/bias");
    const float* const kx[2] = {A + kf->offset, A + kb->offset};      // kernel[:512]: the first 512 of the 640 rows
    const float* const bx[2] = {A + bf->offset, A + bb->offset};
    for (int d = 0; d < 2; ++d)      // kernel[512:] = Wh, fp32 as it is
      CTPN_HIP_TRY(hipMemcpyAsync(c->wh + (size_t)d * 128 * 512, kx[d] + (size_t)512 * 512, (size_t)128 * 512 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = pack_lstm_projection(kx, 512, bx, c->prec, c->wt_x, c->wx_row_bytes, c->b_x, c->wt_xf, s))) return rc;
  }
  {
    const ManifestEntry* we = find_entry("lstm_o/weights");
    const ManifestEntry* be = find_entry("lstm_o/biases");
    if ((rc = launch_pack_transpose(A + we->offset, 512, c->wt_fc, 256, DType::F32, 256, 512, s))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(c->b_fc, A + be->offset, 512 * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  {
    const ManifestEntry* wb = find_entry("rpn_bbox_pred/weights");
    const ManifestEntry* bb = find_entry("rpn_bbox_pred/biases");
    const ManifestEntry* wc = find_entry("rpn_cls_score/weights");
    const ManifestEntry* bc = find_entry("rpn_cls_score/biases");
    CTPN_HIP_TRY(hipMemsetAsync(c->wt_h, 0, (size_t)64 * 512 * sizeof(float), s));
    CTPN_HIP_TRY(hipMemsetAsync(c->b_h, 0, 64 * sizeof(float), s));
    if ((rc = launch_pack_transpose(A + wb->offset, 40, c->wt_h, 512, DType::F32, 512, 40, s))) return rc;
    if ((rc = launch_pack_transpose(A + wc->offset, 20, c->wt_h + (size_t)40 * 512, 512, DType::F32, 512, 20, s))) return rc;
    CTPN_HIP_TRY(hipMemcpyAsync(c->b_h, A + bb->offset, 40 * sizeof(float), hipMemcpyDeviceToDevice, s));
    CTPN_HIP_TRY(hipMemcpyAsync(c->b_h + 40, A + bc->offset, 20 * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  CTPN_HIP_TRY(hipStreamSynchronize(s));
  if ((rc = pack_conv1_frags(c->w_first, c->b_conv[0], (uint4*)c->w_first_frags))) return rc;
  {
    // lstm_o has no activation after its FC (reference network.py:110-113), so FC (256 -> 512) and the two heads
    // (512 -> 40 | 20) compose into one 256 -> 60 map: W' = W_fc W_h, b' = b_fc W_h + b_h, folded here in double.
    // Used by the bf16 throughput mode only; the fp32 gate keeps the reference's two-GEMM op order.
    const ManifestEntry* wf = find_entry("lstm_o/weights");
    const ManifestEntry* bf = find_entry("lstm_o/biases");
    const ManifestEntry* wb = find_entry("rpn_bbox_pred/weights");
    const ManifestEntry* bb = find_entry("rpn_bbox_pred/biases");
    const ManifestEntry* wc = find_entry("rpn_cls_score/weights");
    const ManifestEntry* bc = find_entry("rpn_cls_score/biases");
    std::vector<float> hfc(256 * 512), hbf(512), hwb(512 * 40), hbb(40), hwc(512 * 20), hbc(20);
    CTPN_HIP_TRY(hipMemcpy(hfc.data(), A + wf->offset, hfc.size() * 4, hipMemcpyDeviceToHost));
    CTPN_HIP_TRY(hipMemcpy(hbf.data(), A + bf->offset, hbf.size() * 4, hipMemcpyDeviceToHost));
    CTPN_HIP_TRY(hipMemcpy(hwb.data(), A + wb->offset, hwb.size() * 4, hipMemcpyDeviceToHost));
    CTPN_HIP_TRY(hipMemcpy(hbb.data(), A + bb->offset, hbb.size() * 4, hipMemcpyDeviceToHost));
    CTPN_HIP_TRY(hipMemcpy(hwc.data(), A + wc->offset, hwc.size() * 4, hipMemcpyDeviceToHost));
    CTPN_HIP_TRY(hipMemcpy(hbc.data(), A + bc->offset, hbc.size() * 4, hipMemcpyDeviceToHost));
    std::vector<float> fold((size_t)64 * 256, 0.f), bfold(64, 0.f);
    for (int o = 0; o < 60; ++o) {
      auto wh = [&](int j) -> double { return o < 40 ? hwb[(size_t)j * 40 + o] : hwc[(size_t)j * 20 + (o - 40)]; };
      for (int k = 0; k < 256; ++k) {
        double acc = 0;
        for (int j = 0; j < 512; ++j) acc += (double)hfc[(size_t)k * 512 + j] * wh(j);
        fold[(size_t)o * 256 + k] = (float)acc;
      }
      double accb = o < 40 ? hbb[o] : hbc[o - 40];
      for (int j = 0; j < 512; ++j) accb += (double)hbf[j] * wh(j);
      bfold[o] = (float)accb;
    }
    CTPN_HIP_TRY(hipMemcpy(c->wt_fold, fold.data(), fold.size() * 4, hipMemcpyHostToDevice));
    CTPN_HIP_TRY(hipMemcpy(c->b_fold, bfold.data(), bfold.size() * 4, hipMemcpyHostToDevice));
  }
  c->weights_loaded = true;
  return CTPN_OK;
}

// ctpn_set_option's contract in front of everything that rewrites the arena and its packed copies: both forward streams and the proposal stream
// read them (a submit beside a batch in flight runs on set 1's stream, the recurrence and the heads on stream_p with tail_overlap), the pack runs
// on c->stream alone. Drain, refuse while a slot is busy, forget the cross-stream hand-over: the ctx is idle when the first byte is copied.
static int weights_quiesce(ctpn_ctx* c, const char* who) {
  CTPN_HIP_TRY(hipSetDevice(c->device));
  CTPN_HIP_TRY(sync_forwards(c));
  CTPN_HIP_TRY(hipStreamSynchronize(c->stream_p));
  for (auto& sl : c->slot) if (sl.busy) return fail(CTPN_ERR_STATE, std::string(who) + ": a submitted batch has not been collected");
  for (auto& f : c->fs) f.tail_pending = false;
  return CTPN_OK;
}

}  // namespace ctpn

// ---------------------------------------------------------------------------------------------
// Weight broadcast over RCCL: the ONLY collective on the path -- 71.57 MB of fp32 once at start-up, nothing per
// batch. librccl is dlopen'ed by soname on first use (no link-time dependency; a process that has imported torch gets torch's copy,
// exactly like libamdhip64), the types below restate the five entry points of rccl.h that are used.
// ---------------------------------------------------------------------------------------------
namespace {
typedef struct rcclComm* rccl_comm_t;
struct rccl_unique_id { char internal[128]; };
struct RcclApi {
  int (*get_unique_id)(rccl_unique_id*) = nullptr;
  int (*comm_init_rank)(rccl_comm_t*, int, rccl_unique_id, int) = nullptr;
  int (*comm_init_all)(rccl_comm_t*, int, const int*) = nullptr;
  int (*comm_destroy)(rccl_comm_t) = nullptr;
  int (*bcast)(const void*, void*, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
  const char* (*err_string)(int) = nullptr;
  bool ok = false;
};
constexpr int kRcclFloat = 7;      // ncclFloat32 (rccl.h ncclDataType_t)
const RcclApi& rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
    void* h = nullptr;
    const char* override_path = std::getenv("CTPN_RCCL_LIB");
    if (override_path && *override_path) h = dlopen(override_path, RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      const char* rp = std::getenv("ROCM_PATH");
      const std::string p = std::string(rp && *rp ? rp : "/opt/rocm") + "/lib/librccl.so";
      h = dlopen(p.c_str(), RTLD_NOW | RTLD_GLOBAL);
    }
    if (!h) return a;
    a.get_unique_id = (decltype(a.get_unique_id))dlsym(h, "ncclGetUniqueId");
    a.comm_init_rank = (decltype(a.comm_init_rank))dlsym(h, "ncclCommInitRank");
    a.comm_init_all = (decltype(a.comm_init_all))dlsym(h, "ncclCommInitAll");
    a.comm_destroy = (decltype(a.comm_destroy))dlsym(h, "ncclCommDestroy");
    a.bcast = (decltype(a.bcast))dlsym(h, "ncclBroadcast");
    a.group_start = (decltype(a.group_start))dlsym(h, "ncclGroupStart");
    a.group_end = (decltype(a.group_end))dlsym(h, "ncclGroupEnd");
    a.err_string = (decltype(a.err_string))dlsym(h, "ncclGetErrorString");
    a.ok = a.get_unique_id && a.comm_init_rank && a.comm_init_all && a.comm_destroy && a.bcast && a.group_start && a.group_end;
    return a;
  }();
  return api;
}
int rccl_fail(const char* what, int code) {
  const RcclApi& r = rccl_api();
  return fail(CTPN_ERR_HIP, std::string(what) + ": RCCL error " + std::to_string(code) + (r.err_string ? std::string(" (") + r.err_string(code) + ")" : std::string()));
}
}  // namespace

extern "C" {

int ctpn_weight_count(void) { return (int)manifest().size(); }
int ctpn_weight_manifest(int index, const char** name, int* rank, int shape4[4], size_t* offset_floats) {
  const auto& m = manifest();
  if (index < 0 || index >= (int)m.size()) return fail(CTPN_ERR_ARG, "manifest index out of range");
  if (name) *name = m[index].name.c_str();
  if (rank) *rank = m[index].rank;
  if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = m[index].shape[i];
  if (offset_floats) *offset_floats = m[index].offset;
  return CTPN_OK;
}

int ctpn_load_weights_host(ctpn_ctx* c, const float* arena_host) {
  if (!c || !arena_host) return fail(CTPN_ERR_ARG, "null pointer");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_load_weights_host: post-processing-only ctx (ctpn_create_postproc) has no network");
  if (const int rc = weights_quiesce(c, "ctpn_load_weights_host")) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(c->arena, arena_host, (size_t)CTPN_WEIGHT_FLOATS * sizeof(float), hipMemcpyHostToDevice, c->stream));
  return pack_weights(c);
}
int ctpn_load_weights_device(ctpn_ctx* c, const void* arena_dev) {
  if (!c || !arena_dev) return fail(CTPN_ERR_ARG, "null pointer");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_load_weights_device: post-processing-only ctx (ctpn_create_postproc) has no network");
  if (const int rc = weights_quiesce(c, "ctpn_load_weights_device")) return rc;
  CTPN_HIP_TRY(hipMemcpyAsync(c->arena, arena_dev, (size_t)CTPN_WEIGHT_FLOATS * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return pack_weights(c);
}

int ctpn_comm_unique_id(char* id_out, size_t capacity) {
  if (!id_out || capacity < CTPN_COMM_ID_BYTES) return fail(CTPN_ERR_ARG, "ctpn_comm_unique_id: buffer of at least CTPN_COMM_ID_BYTES required");
  const RcclApi& r = rccl_api();
  if (!r.ok) return fail(CTPN_ERR_NODEVICE, "ctpn_comm_unique_id: librccl.so could not be loaded (set CTPN_RCCL_LIB or ROCM_PATH)");
  rccl_unique_id id;
  const int e = r.get_unique_id(&id);
  if (e) return rccl_fail("ncclGetUniqueId", e);
  std::memcpy(id_out, id.internal, CTPN_COMM_ID_BYTES);
  return CTPN_OK;
}

int ctpn_broadcast_weights_rank(ctpn_ctx* c, const char* unique_id, int rank, int world, int root) {
  if (!c || !unique_id) return fail(CTPN_ERR_ARG, "null pointer");
  if (world < 1 || rank < 0 || rank >= world || root < 0 || root >= world) return fail(CTPN_ERR_ARG, "ctpn_broadcast_weights_rank: rank / root outside [0, world)");
  if (c->postproc_only) return fail(CTPN_ERR_STATE, "ctpn_broadcast_weights_rank: post-processing-only ctx has no network");
  if (rank == root && !c->weights_loaded) return fail(CTPN_ERR_STATE, "ctpn_broadcast_weights_rank: the root's weights are not loaded");
  // a local pre-check like the others: in front of the communicator, so that a rank with a batch in flight leaves before it joins
  if (const int rc = weights_quiesce(c, "ctpn_broadcast_weights_rank")) return rc;
  const RcclApi& r = rccl_api();
  if (!r.ok) return fail(CTPN_ERR_NODEVICE, "ctpn_broadcast_weights_rank: librccl.so could not be loaded (set CTPN_RCCL_LIB or ROCM_PATH)");
  rccl_unique_id id;
  std::memcpy(id.internal, unique_id, CTPN_COMM_ID_BYTES);
  rccl_comm_t comm = nullptr;
  int e = r.comm_init_rank(&comm, world, id, rank);
  if (e) return rccl_fail("ncclCommInitRank", e);
  e = r.bcast(c->arena, c->arena, (size_t)CTPN_WEIGHT_FLOATS, kRcclFloat, root, comm, c->stream);
  const hipError_t he = hipStreamSynchronize(c->stream);
  (void)r.comm_destroy(comm);
  if (e) return rccl_fail("ncclBroadcast", e);
  if (he != hipSuccess) return fail(CTPN_ERR_HIP, std::string("ctpn_broadcast_weights_rank: ") + hipGetErrorString(he));
  return rank == root ? CTPN_OK : pack_weights(c);
}

int ctpn_broadcast_weights(ctpn_ctx** handles, int n) {
  if (!handles || n < 1) return fail(CTPN_ERR_ARG, "ctpn_broadcast_weights: handles / n");
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) {
    if (!handles[i] || handles[i]->postproc_only) return fail(CTPN_ERR_ARG, "ctpn_broadcast_weights: null or post-processing-only ctx");
    devs[i] = handles[i]->device;
    for (int j = 0; j < i; ++j) if (devs[j] == devs[i]) return fail(CTPN_ERR_ARG, "ctpn_broadcast_weights: two ctxs on the same device (RCCL needs one rank per GPU)");
  }
  if (!handles[0]->weights_loaded) return fail(CTPN_ERR_STATE, "ctpn_broadcast_weights: handles[0] has no weights loaded");
  for (int i = 0; i < n; ++i)      // every handle, the sender included: its arena is read while the others' are written
    if (const int rc = weights_quiesce(handles[i], "ctpn_broadcast_weights")) return rc;
  if (n == 1) return CTPN_OK;
  const RcclApi& r = rccl_api();
  if (!r.ok) return fail(CTPN_ERR_NODEVICE, "ctpn_broadcast_weights: librccl.so could not be loaded (set CTPN_RCCL_LIB or ROCM_PATH)");
  std::vector<rccl_comm_t> comms(n, nullptr);
  int e = r.comm_init_all(comms.data(), n, devs.data());
  if (e) return rccl_fail("ncclCommInitAll", e);
  int rc = CTPN_OK;
  e = r.group_start();
  for (int i = 0; i < n && !e; ++i) {
    if (hipSetDevice(devs[i]) != hipSuccess) { rc = fail(CTPN_ERR_HIP, "ctpn_broadcast_weights: hipSetDevice"); break; }
    e = r.bcast(handles[i]->arena, handles[i]->arena, (size_t)CTPN_WEIGHT_FLOATS, kRcclFloat, 0, comms[i], handles[i]->stream);
  }
  const int e2 = r.group_end();
  if (!e) e = e2;
  for (int i = 0; i < n; ++i) {
    (void)hipSetDevice(devs[i]);
    if (hipStreamSynchronize(handles[i]->stream) != hipSuccess && rc == CTPN_OK) rc = fail(CTPN_ERR_HIP, "ctpn_broadcast_weights: stream sync");
  }
  for (int i = 0; i < n; ++i) (void)r.comm_destroy(comms[i]);
  if (e) return rccl_fail("ncclBroadcast", e);
  if (rc) return rc;
  for (int i = 1; i < n; ++i) {
    CTPN_HIP_TRY(hipSetDevice(devs[i]));
    if ((rc = pack_weights(handles[i]))) return rc;
  }
  return CTPN_OK;
}

}  // extern "C"
