/*
 * ctpn_hip.h -- C ABI of libctpn_hip.so, the MI355X (gfx950) CTPN inference hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, returns an int status
 * (0 = CTPN_OK, negative = error; ctpn_last_error() gives the text) and never throws.
 * A ctx owns its HIP streams and its HBM arena. Threads: any number of ctxs per device; each ctx is used by one host thread at a time;
 * distinct ctxs, and the calls that take no ctx, may run concurrently from different host threads (what they share per device is
 * guarded inside the library: INTEGRATION.md, "Threads"). One ctx used from two threads at once is outside the contract.
 *
 * Each declaration cites the reference interface (paths relative to the upstream tree of
 * eragonruan/text-detection-ctpn) that it replaces; INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add to bind it.
 */
#ifndef CTPN_HIP_H
#define CTPN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTPN_ABI_VERSION 10

/* status codes */
#define CTPN_OK            0
#define CTPN_ERR_ARG      -1   /* bad argument (null pointer, size out of range, K not tile-aligned ...) */
#define CTPN_ERR_HIP      -2   /* a HIP runtime call failed; text has hipGetErrorString */
#define CTPN_ERR_STATE    -3   /* call order violated (e.g. forward before weights are loaded) */
#define CTPN_ERR_CAPACITY -4   /* caller buffer or ctx arena too small for the request */
#define CTPN_ERR_NODEVICE -5   /* no usable gfx950 device: the product path never falls back to CPU */
#define CTPN_ERR_UNSUPPORTED -6 /* a well-formed input of a kind this entry point does not handle (ctpn_decode_jpeg_batch: CMYK / 4:1:1 / arithmetic-coded / incomplete files) */

/* arithmetic of the conv stack / LSTM input projection (BiLSTM recurrence and heads are fp32 in all of them) */
#define CTPN_PREC_FP32  0      /* exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): correctness gate, config 2 */
#define CTPN_PREC_BF16  1      /* bf16 MFMA, fp32 accumulate (v_mfma_f32_32x32x16_bf16): configs 3-5 (BASELINE.json's dtype) */
#define CTPN_PREC_FP16  2      /* IEEE fp16 MFMA, fp32 accumulate (v_mfma_f32_32x32x16_f16): the bf16 mode's rate, three more mantissa bits
                                  (activations of this network stay far below 65504) */
#define CTPN_PREC_SPLIT 3      /* parity-grade at the matrix cores' 16-bit rate / 3: every activation and weight is a (hi, lo) pair of bf16 and
                                  a product is three bf16 MFMAs (x_hi w_hi + x_lo w_hi + x_hi w_lo, fp32 accumulate; the dropped term is
                                  ~2^-17 of the product): holds north_star's 1e-3 / +-1 px against the fp32 path like CTPN_PREC_FP32 does */
/* (value 4 was CTPN_PREC_FP16W, ABI versions 6 - 7: fp16 with three layers through a 1-D Winograd transform. +2 % images/s for a fifth
 * arithmetic; removed in ABI version 8, ctpn_create answers CTPN_ERR_ARG for it. Measurements: profiles/r04_layers_fp16w.txt.) */

/* text-line connector mode: cfg.TEST.DETECT_MODE, lib/fast_rcnn/config.py:150 */
#define CTPN_MODE_H 0
#define CTPN_MODE_O 1

/* fixed geometry of the path (lib/rpn_msr/generate_anchors.py:24-32, lib/fast_rcnn/config.py:175-183) */
#define CTPN_NUM_ANCHORS      10
#define CTPN_FEAT_STRIDE      16
#define CTPN_WEIGHT_FLOATS    17893244  /* fp32 scalars in the flat weight arena, see ctpn_weight_manifest */

typedef struct ctpn_ctx ctpn_ctx;

/* ---- library ---------------------------------------------------------------------------- */

int         ctpn_abi_version(void);
/* thread-local text of the last error raised on this thread ("" if none) */
const char* ctpn_last_error(void);
/* number of visible HIP devices (0 if none); never fails */
int         ctpn_device_count(void);

/* ---- context ------------------------------------------------------------------------------
 * Replaces: tf.Session + get_network("VGGnet_test") (ctpn/demo.py:79-82,
 * lib/networks/VGGnet_test.py:7-55) and _set_device (lib/utils/nms_kernel.cu:80-89).
 * Allocates every activation buffer for up to max_batch images of max_h x max_w once; no
 * allocation happens on the forward path afterwards. */
int ctpn_create(ctpn_ctx** out, int device_id, int max_batch, int max_h, int max_w, int precision);
/* Post-processing-only ctx: the proposal layer (ctpn_proposals_from_host, ctpn_proposal_anchors) for up to max_batch feature
 * maps of max_hf x max_wf cells, WITHOUT the VGG activation arena and the weights (what lib/rpn_msr/proposal_layer_tf.py
 * needs when the network ran elsewhere, ctpn/demo_pb.py:91-92). ctpn_forward / ctpn_load_weights_* fail with CTPN_ERR_STATE. */
int ctpn_create_postproc(ctpn_ctx** out, int device_id, int max_batch, int max_hf, int max_wf);
int ctpn_destroy(ctpn_ctx* ctx);
/* Behaviour switches of ONE ctx (ABI 5; they were process-wide environment variables before): integer options by name, settable between
 * calls (the ctx drains its streams first; CTPN_ERR_STATE while a submitted batch is uncollected). ctpn_option_count / ctpn_option_name
 * enumerate them. None has a counterpart in the reference, whose only knobs are cfg.TEST.* (lib/fast_rcnn/config.py:147-183).
 *   keep_acts       0 | 1  also store the full-resolution output of pool-fused convs and lstm_o (layer-wise parity via ctpn_get_tensor)
 *   conv1_kernel    0..2   16-bit modes: conv1_1 as 2 = exact integer pixels x 16-bit weights, one MFMA term, from the q-image (8-byte pixels
 *                          (q_B, q_G, q_R, 1.0), q = p - round(mean); uint8 feed; default), 1 = split-bf16 operands, three terms (fp32-class; the
 *                          float-blob feed always), 0 = fp32 VALU
 *   conv1_fuse      0 | 1  with conv1_kernel = 2 and keep_acts = 0: conv1_1 is computed inside conv1_2's window stage and never stored
 *                          (default); 0 = stored by a stand-alone kernel and read back -- the same bytes downstream either way
 *   lstm_split      0 | 1  BiLSTM recurrent product h Wh on split-bf16 MFMAs (three bf16 terms per product, fp32 state / gates / accumulation:
 *                          |d| < 3e-5 vs the exact-fp32 MFMA kernel, 2 x faster). Default 1 in CTPN_PREC_BF16 / FP16 / SPLIT (split precision: since
 *                          ABI 9 -- it is that mode's own arithmetic), 0 in FP32, which never uses it
 *   nms_columns     0 .. 3 proposal-layer NMS: 1 (default) the column decomposition -- one workgroup per image, and for batches of up to four
 *                          images one COLUMN per wave over a quarter as many workgroups per image (a lone image's tail used one CU of 256);
 *                          0 the generic kernel; 2 / 3 pin the one-workgroup / the multi-workgroup form. Identical keep lists in all four
 *   nms_check       0 | 1  debug: run both and fail with CTPN_ERR_STATE on a mismatch (synchronises)
 *   connect_device  0 | 1  text-line connector of ctpn_detect_*: host C++ worker pool (default) or connect_kernel on the GPU: identical lines
 *   tail_overlap    0 | 1  ctpn_detect_submit: BiLSTM + heads of batch k on the proposal stream next to conv1_1 of batch k + 1
 *   conv_p64        0 | 1  CTPN_PREC_SPLIT: conv1_2 (Co = 64) through the persistent kernel's 64-channel form (default 1; 0 = the non-persistent
 *                          kernel of ABI 8). Other last bits than ABI 8 (kx-major K order), same tolerance class
 *   split_edge      0 | 1  CTPN_PREC_SPLIT: ragged tile columns (W mod 16 = 1, 2; pooled layers: 2, 4) through conv3x3_edge_kernel's split form, as in
 *                          the 16-bit modes (default 1; 0 = a padded tile column as in ABI 9: other last bits in those columns, same tolerance class)
 *   tail_confine    0 | 1  ctpn_detect_submit: the forward of batch k + 1 waits, behind its conv1_1, for the proposal tail of batch k (default 0).
 *                          Round 6 shipped 1 for CTPN_PREC_SPLIT while a cross-batch race of the conv kernels was open; the race is fixed in the
 *                          kernels (ABI 10), the switch stays for A/B runs
 *   nms_prefix      0 | 1  proposal-layer column NMS: look at the 4096 best-scored candidates first and at all of them only if those hold fewer
 *                          than post_nms_topn survivors (default 1). Identical keep lists
 *   debug_hog       0 .. 200000  diagnostic: microseconds a kernel with the one-workgroup NMS's footprint (1024 threads, 84 KB of LDS, one
 *                          workgroup per image) spins, without memory traffic, in front of the proposal NMS (default 0: not launched); values
 *                          above 50000: it also keeps writing its LDS, for (value - 50000) microseconds; above 100000: twice the workgroups gather random 16-byte
 *                          pieces of the largest activation buffer for (value - 100000) microseconds (memory-system load beside EVERY layer of
 *                          the next batch). It delays the NMS of batch k into later
 *                          layers of batch k + 1: the stress under which tests/test_gpu_round6.py checks that batches in flight do not
 *                          change each other's bits
 *   debug_nms       0 .. 15  diagnostic, WRONG proposals: parts of the one-workgroup proposal NMS switched off (1 no greedy pass, 2 no output
 *                          stores, 4 no box loads in the greedy pass, 8 return after the column lists); tools/r6_nms_parts.sh */
int         ctpn_set_option(ctpn_ctx* ctx, const char* key, int value);
int         ctpn_get_option(ctpn_ctx* ctx, const char* key, int* value_out);
int         ctpn_option_count(void);
const char* ctpn_option_name(int index);
/* Parameters of ONE ctx's detection tail (additive in ABI 10): what the reference reads at run time from cfg.TEST.RPN_* (ctpn/text.yml,
 * lib/fast_rcnn/config.py:175-183) and from TextLineCfg (lib/text_connector/text_connect_cfg.py:4-12), as doubles by the reference's
 * names. ctpn_detect, ctpn_detect_submit / ctpn_detect_collect and ctpn_debug_text_lines read them -- the proposal layer's arguments,
 * lines_prep_kernel, the connector's NMS, connect_kernel and the collect's host connector alike; ctpn_proposals and
 * ctpn_proposals_from_host keep taking their four values as arguments. A fresh ctx holds the defaults, with which every entry point
 * computes bit for bit what it did while the values were compiled in.
 *   name                       default  accepted
 *   RPN_PRE_NMS_TOP_N          12000    integral, 1 .. 12000 (the ctx's buffers are sized for the default)
 *   RPN_POST_NMS_TOP_N         1000     integral, 1 .. capacity (ctpn_reserve_proposals; 1000 on a fresh ctx)
 *   RPN_NMS_THRESH             0.7      0 .. 1 (below 0.1 the generic NMS kernel runs instead of the column decomposition: same keep lists)
 *   RPN_MIN_SIZE               8        >= 0
 *   TEXT_PROPOSALS_MIN_SCORE   0.7      finite
 *   TEXT_PROPOSALS_NMS_THRESH  0.2      0 .. 1 (below 0.15 the generic NMS kernel runs: same keep lists)
 *   MAX_HORIZONTAL_GAP         50       integral, 0 .. 4096
 *   MIN_V_OVERLAPS             0.7      finite
 *   MIN_SIZE_SIM               0.7      finite
 *   MIN_RATIO                  0.5      finite
 *   LINE_MIN_SCORE             0.9      finite
 *   MIN_LINE_WIDTH             32       finite; TEXT_PROPOSALS_WIDTH * MIN_NUM_PROPOSALS -- the reference only ever uses the product
 * A value is used in the precision of the reference's comparison: RPN_NMS_THRESH, RPN_MIN_SIZE, TEXT_PROPOSALS_MIN_SCORE,
 * TEXT_PROPOSALS_NMS_THRESH, MIN_V_OVERLAPS, MIN_SIZE_SIM and the gap are rounded to fp32 ONCE, when set (they must stay finite in fp32:
 * |value| <= 3e38); MIN_RATIO, LINE_MIN_SCORE and MIN_LINE_WIDTH are compared in fp64 (filter_boxes). No kernel bounds a value more tightly
 * than the table says. ctpn_set_param follows ctpn_set_option's contract: the ctx drains its streams first, CTPN_ERR_STATE while a submitted
 * batch is uncollected, CTPN_ERR_ARG for an unknown name, a NaN or a value outside its range. ctpn_get_param returns the value as set.
 * With RPN_POST_NMS_TOP_N below the capacity, rois_out / keep_out of ctpn_detect*, ctpn_debug_text_lines still hold capacity rows per image
 * (fewer of them valid). ctpn_param_count / ctpn_param_name enumerate the names; ctpn_param_default needs no ctx and no device. */
int         ctpn_set_param(ctpn_ctx* ctx, const char* name, double value);
int         ctpn_get_param(ctpn_ctx* ctx, const char* name, double* value_out);
int         ctpn_param_count(void);
const char* ctpn_param_name(int index);
int         ctpn_param_default(const char* name, double* value_out);
/* The proposal capacity of ONE ctx (additive in ABI 10): the rows per image of rois_out, keep_out and anchors_out towards the caller, and the
 * upper bound of RPN_POST_NMS_TOP_N and of every post_nms_topn argument. The reference reads cfg.TEST.RPN_POST_NMS_TOP_N at run time and
 * takes any value (lib/rpn_msr/proposal_layer_tf.py:55; lib/fast_rcnn/config.py:180 sets 1000); a proposal is a 16-pixel slice of a line, so
 * 1000 of them cover about 17 full-width lines of a 600 x 900 page, and a dense page needs more. A fresh ctx has capacity 1000 and refuses
 * 1001 everywhere, as ever. ctpn_reserve_proposals(ctx, post_capacity), 1000 .. CTPN_POST_NMS_CAPACITY_MAX, replaces every buffer of the
 * tail that is laid out by the capacity (the slots' page-locked blocks among them); results of earlier ctpn_proposals* calls are no longer
 * readable afterwards (ctpn_proposal_anchors, ctpn_debug_proposal_fetch: CTPN_ERR_STATE). ctpn_set_option's contract: the ctx drains its streams
 * first, CTPN_ERR_STATE while a submitted batch is uncollected; CTPN_ERR_ARG outside the range or below the ctx's current
 * RPN_POST_NMS_TOP_N; a failed allocation (CTPN_ERR_HIP) leaves the ctx as it was. Works on a ctpn_create_postproc ctx too. Above 1024 rows
 * per image (RPN_POST_NMS_TOP_N, not the capacity) the text-line tail takes other kernel forms (ctpn_debug_text_line_plan); the device
 * connector returns up to capacity / 2 lines per image and mode. ctpn_proposal_capacity reports the capacity. */
#define CTPN_POST_NMS_CAPACITY_MAX 4096
int         ctpn_reserve_proposals(ctpn_ctx* ctx, int post_capacity);
int         ctpn_proposal_capacity(ctpn_ctx* ctx, int* rows_out);
/* Host worker threads of a ctx (per-image connector work of ctpn_detect_collect, staging copies of pageable images): one
 * persistent pool per ctx, created in ctpn_create. Size = ctpn_host_thread_budget(hardware cores, LOCAL_WORLD_SIZE of the
 * launcher (torchrun), CTPN_HOST_THREADS): `requested` if > 0, else cores / ranks-on-this-node clamped to [1, 32].
 * CTPN_AFFINITY=1 pins the pool to the cores [LOCAL_RANK * budget, (LOCAL_RANK + 1) * budget). Pure function, needs no GPU.
 * (The reference runs its connector on the one Python thread of ctpn/demo.py:63-64.) */
int ctpn_host_thread_budget(int cpu_count, int local_world_size, int requested);
int ctpn_host_threads(ctpn_ctx* ctx, int* threads_out);
/* block until everything queued on the ctx stream has finished */
int ctpn_sync(ctpn_ctx* ctx);
/* the hipStream_t the ctx launches on (as void*), for callers that bracket it with events */
int ctpn_stream(ctpn_ctx* ctx, void** stream_out);

/* ---- weights ------------------------------------------------------------------------------
 * Replaces: tf.train.Saver().restore (ctpn/demo.py:85-93) / Network.load (lib/networks/network.py:40-53).
 * The arena is CTPN_WEIGHT_FLOATS fp32 values: the reference's TF variables, each in its TF
 * layout (conv HWIO [3,3,Ci,Co], LSTMCell kernel [640,512] gate order i,j,f,o, matmul [in,out]),
 * concatenated in the order ctpn_weight_manifest() reports. */
int ctpn_weight_manifest(int index, const char** name, int* rank, int shape4[4], size_t* offset_floats);
int ctpn_weight_count(void);
/* A ctx's weights are the LAST arena loaded: every load rewrites the ctx's copy of the arena and every layout packed from it, on a live ctx as
 * on a fresh one (a server that swaps checkpoints), and changes nothing else -- options, parameters, the proposal capacity and the stored
 * activations of the last forward stay. When a load is allowed: ctpn_load_weights_host, ctpn_load_weights_device, ctpn_broadcast_weights_rank
 * and ctpn_broadcast_weights follow ctpn_set_option's contract -- the ctx drains its forward streams and the proposal stream first, and the call
 * is refused with CTPN_ERR_STATE ("... a submitted batch has not been collected") while a ctpn_detect_submit* is uncollected in either slot,
 * whatever the arena holds: a batch in flight reads the packed weights on streams the pack does not run on. Collect, then load. */
int ctpn_load_weights_host(ctpn_ctx* ctx, const float* arena_host);
/* arena already in this device's HBM (e.g. a torch tensor filled by an RCCL broadcast, or another ctx's arena): copied into the ctx's own arena
 * and packed from there. The copy runs on the ctx's stream, which knows nothing of the stream that filled arena_dev: the caller synchronises
 * the producer first (torch.cuda.synchronize(), hipStreamSynchronize). The call returns after the pack; arena_dev may be released then. */
int ctpn_load_weights_device(ctpn_ctx* ctx, const void* arena_dev);

/* ---- weight broadcast (RCCL over xGMI) ----------------------------------------------------------
 * The reference has no collective at all (no NCCL / MPI anywhere; batch asserted to 1). This build shards
 * images over GPUs with ONE collective: the fp32 arena is broadcast once at start-up (north_star: "RCCL broadcast of weights over
 * xGMI only"), nothing per batch. librccl.so is loaded on first use (dlopen by soname; CTPN_RCCL_LIB overrides the path).
 *
 * ctpn_broadcast_weights: one process, n ctxs on n DIFFERENT devices (SURVEY section 8b export list): handles[0] must have its weights
 * loaded; every other ctx receives the arena over RCCL (ncclCommInitAll + grouped ncclBroadcast on each ctx's stream) and packs it. EVERY
 * handle is drained and checked first (the weights block above): one uncollected batch on any of them is CTPN_ERR_STATE and nothing is sent.
 *
 * One process per GPU (torchrun; bench.py): the root calls ctpn_comm_unique_id and hands the CTPN_COMM_ID_BYTES bytes to the other
 * ranks by any side channel (bench.py: the torch.distributed store), then EVERY rank calls ctpn_broadcast_weights_rank, which
 * joins the communicator (collective call), receives / sends the arena on the ctx stream and packs. The root loads its weights first. */
#define CTPN_COMM_ID_BYTES 128
int ctpn_broadcast_weights(ctpn_ctx** handles, int n);
int ctpn_comm_unique_id(char* id_out, size_t capacity);
int ctpn_broadcast_weights_rank(ctpn_ctx* ctx, const char* unique_id, int rank, int world, int root);
/* ctpn_broadcast_weights_rank is a COLLECTIVE with no timeout of its own: a rank whose local pre-checks fail (librccl not loadable, a
 * post-processing-only ctx, a root without weights, a submitted batch that has not been collected) returns an error BEFORE joining the
 * communicator, and every other rank then blocks in ncclCommInitRank. The caller must either make sure all ranks pass the same pre-checks
 * (same library, same kind of ctx, root loaded, both slots collected) or
 * run the call under its own watchdog -- bench.py does both (180 s timer, and the ranks agree on success over the side channel before
 * anyone proceeds; on failure all of them fall back to a host broadcast). */

/* ---- network forward ----------------------------------------------------------------------
 * Replaces: _get_image_blob + sess.run of conv1_1 .. rpn_cls_prob_reshape / rpn_bbox_pred
 * (lib/fast_rcnn/test.py:7-51, lib/networks/VGGnet_test.py:20-52, lib/networks/network.py:88-196,
 * 269-277, 332-337). images: n x h x w x 3 uint8, BGR, already at network resolution (the two
 * reference resizes are identity there); PIXEL_MEANS (lib/fast_rcnn/config.py:200) are subtracted
 * on device. images_on_device != 0 means the pointer is HBM, else host (copied on the ctx stream).
 * Asynchronous: returns after enqueueing. */
int ctpn_forward(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w);
/* Same, fed with the reference's own `net.data` blob (lib/fast_rcnn/test.py:47-49): n x h x w x 3 float32,
 * BGR, PIXEL_MEANS already subtracted (what _get_image_blob returns after its cv2.resize).
 * Feed dtype and conv1_1 (CTPN_PREC_BF16 / CTPN_PREC_FP16; CTPN_PREC_FP32 and CTPN_PREC_SPLIT compute both feeds identically): the uint8 feed runs
 * conv1_1 as EXACT integer pixels x bf16-rounded weights (one MFMA term), the float feed -- arbitrary floats -- as split-bf16
 * operands (three terms, fp32-class). The same image through the two feeds therefore differs by the bf16 rounding of conv1_1's 27
 * weights per channel, the same class of error every other layer of the bf16 path carries: rpn_cls_prob within 3e-2 max / 2e-3
 * mean of each other at 600x900 (tests/test_gpu_round3.py::test_float_blob_feed_tracks_uint8_feed_in_bf16_mode). In bf16 mode the
 * BiLSTM gates use v_exp_f32 / v_rcp_f32 (|diff| < 2e-5 on lstm_out against the exact path, same file). */
int ctpn_forward_blob(ctpn_ctx* ctx, const float* blob, int blob_on_device, int n, int h, int w);
/* ---- ragged batches: images of one WIDTH and different heights in one call --------------------
 * (The reference's notion of such a batch is lib/utils/blob.py im_list_to_blob, which zero-pads a list of images to the largest shape; it
 * asserts batch size 1 in front of it, lib/rpn_msr/proposal_layer_tf.py:51-52.)
 * A ragged batch is a canvas n x hc x w x 3 (BGR uint8) plus heights[n], 16 <= heights[i] <= hc. Image i is rows [0, heights[i]) of slot i;
 * the rows below it may hold anything and are never read as pixels. Its valid rows at pooling level L are heights[i] >> L (every VALID
 * pool drops an odd last row): ctpn_ragged_valid_rows, a pure function (no ctx, no device; -1 for height < 0 or a level outside 0 .. 4).
 * The forward runs the uniform forward's kernels on the canvas geometry (n, hc, w) and clears rows >= heights[i] >> L of every STORED
 * activation of image i before the next layer reads it -- the input, every stored conv output, every stored pool output, rpn_conv/3x3 -- so
 * that to the image above them those rows are the zero padding it would have had alone. The result is defined as, and tested to be, bit
 * for bit what ctpn_forward / ctpn_detect give for image i alone (an n x heights[i] x w call of one image).
 *  - conv1_1 is computed stand-alone from the q-image (the form option conv1_fuse = 0 selects: the same bytes); CTPN_PREC_FP32, CTPN_PREC_SPLIT
 *    and conv1_kernel < 2 go through a ctx-owned float feed (pixel - PIXEL_MEANS inside an image, 0.0f below it; n * hc * w * 12 bytes,
 *    allocated on the first ragged call and grown on demand).
 *  - The BiLSTM, its projection and the heads run on all n * (hc >> 4) feature rows; the proposal layer gives the cells below an image no
 *    candidates. Anchor indices (y * wf + x) * 10 + a are the lone image's, since wf is shared.
 *  - im_info row i is [heights[i], w, scales[i]] in the detect forms. ctpn_proposals after a ragged forward uses that forward's valid rows
 *    (its im_info is the caller's, as always); a uniform ctpn_forward forgets them.
 *  - ctpn_get_tensor after a ragged forward returns canvas-shaped tensors (n, hc >> L, w >> L, C): conv and pool maps are zero below an
 *    image, lstm_*, heads and rpn_* are undefined there.
 *  - A call whose heights all equal hc IS the uniform call and takes its path (fused conv1_1, no clearing).
 *  - A caller's device canvas is not modified. Mixed widths are not supported: group by width first.
 * Errors: CTPN_ERR_ARG for a null pointer or a height outside 16 .. hc; CTPN_ERR_CAPACITY for the canvas as ctpn_forward; CTPN_ERR_STATE
 * on a post-processing-only ctx or without weights. Asynchronous like ctpn_forward. */
int ctpn_ragged_valid_rows(int height, int level);
int ctpn_forward_ragged(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights);
/* feature-map geometry of the last forward: hf = h/16 (VALID pools), wf = w/16 */
int ctpn_feat_shape(ctpn_ctx* ctx, int* n, int* hf, int* wf);
/* copy a named activation of the last forward to the host as dense fp32 NHWC (layer-wise parity).
 * names: conv1_1 .. conv5_3, pool1..pool4, rpn_conv/3x3, lstm_pre, lstm_out, lstm_o, heads,
 * rpn_cls_prob_reshape (n,hf,wf,20), rpn_bbox_pred (n,hf,wf,40). Synchronises the stream. */
int ctpn_get_tensor(ctpn_ctx* ctx, const char* name, float* out_host, size_t capacity_floats, int shape4[4]);
/* The same tensor left in HBM, unpacked by a kernel: the training-side companion header, ctpn_hip_train.h. */

/* ---- proposal layer -----------------------------------------------------------------------
 * Replaces: Network.proposal_layer / proposal_layer (lib/networks/network.py:207-222,
 * lib/rpn_msr/proposal_layer_tf.py:14-157) incl. bbox_transform_inv, clip_boxes, _filter_boxes
 * (lib/fast_rcnn/bbox_transform.py:36-80) and the nms call at :144. Runs on the activations of
 * the last ctpn_forward. im_info: n x 3 floats [H, W, scale] (lib/fast_rcnn/test.py:44-46).
 * rois_out: n x post_nms_topn x 5 floats [score,x1,y1,x2,y2] (column 0 is the score, as in the
 * reference, proposal_layer_tf.py:155), counts_out: n ints. Tie order: descending score, equal
 * scores by ascending anchor index (h, w, a) -- documented deviation from numpy's unstable sort.
 * Synchronous (returns after the D2H copy). */
int ctpn_proposals(ctpn_ctx* ctx, const float* im_info, int pre_nms_topn, int post_nms_topn,
                   float nms_thresh, float min_size, float* rois_out, int* counts_out);
/* same computation from caller-supplied head outputs (the demo_pb.py seam, ctpn/demo_pb.py:91-92):
 * cls_prob n x hf x wf x 20, bbox_pred n x hf x wf x 40, fp32 host arrays */
int ctpn_proposals_from_host(ctpn_ctx* ctx, const float* cls_prob, const float* bbox_pred,
                             int n, int hf, int wf, const float* im_info, int pre_nms_topn,
                             int post_nms_topn, float nms_thresh, float min_size,
                             float* rois_out, int* counts_out);

/* Second return value of proposal_layer (lib/rpn_msr/proposal_layer_tf.py:133-157: bbox_deltas[order][keep]): for every roi row of
 * the LAST ctpn_proposals / ctpn_proposals_from_host call, the index of the anchor that produced it, (y * wf + x) * 10 + a --
 * i.e. the row of rpn_bbox_pred.reshape(-1, 4). anchors_out: n x post_nms_topn ints (rows >= counts_out[i] are undefined);
 * post_nms_topn must equal that call's. */
int ctpn_proposal_anchors(ctpn_ctx* ctx, int* anchors_out, int post_nms_topn);

/* ---- input pipeline ------------------------------------------------------
 * Replaces: cv2.resize(im, None, None, fx=f, fy=f, interpolation=cv2.INTER_LINEAR) as called by
 * resize_im (ctpn/demo.py:21-25, uint8 BGR image) and by _get_image_blob (lib/fast_rcnn/test.py:17-27,
 * float32 image after the PIXEL_MEANS subtraction). OpenCV itself (opencv_python==3.4.0.12) is a
 * third-party dependency outside the reference tree: the kernel follows its published algorithm
 * (dsize = round-half-even(src * f); sample at (d + 0.5) / f - 0.5; uint8 in 11-bit fixed point,
 * float32 in fp32) -- parity with the real cv2 is UNPINNED, parity with oracle/resize_ref.py is
 * bit-exact. src: n x h x w x 3, dst: n x out_h x out_w x 3 (capacity in elements); either side may
 * be a device pointer (src_on_device / dst_on_device), e.g. to feed ctpn_forward without a round
 * trip. out_h / out_w are always written (call with dst == NULL to size the output). */
int ctpn_resize_dims(int h, int w, double fx, double fy, int* out_h, int* out_w);
int ctpn_resize(int device_id, const void* src, int src_is_f32, int src_on_device, int n, int h, int w,
                double fx, double fy, void* dst, int dst_on_device, long long dst_capacity,
                int* out_h, int* out_w);

/* ---- NMS ----------------------------------------------------------------------------------
 * Replaces: void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num,
 *                     int boxes_dim, float nms_overlap_thresh, int device_id)
 * (lib/utils/gpu_nms.hpp:1-2, lib/utils/nms_kernel.cu:91-143). Same argument order and meaning:
 * boxes_host is boxes_num x boxes_dim (>= 4) fp32 rows [x1,y1,x2,y2,...] already sorted by
 * descending score; keep_out (capacity boxes_num) receives positions into that array in
 * ascending order. Suppress iff fp32 IoU("+1" areas) > fp32(thresh) (nms_kernel.cu:24-32,71).
 * Differences: returns a status instead of printing CUDA errors; device buffers are cached per
 * device instead of malloc/free per call; only keep[] leaves the GPU (no 18 MB mask D2H). */
int ctpn_nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
             float nms_overlap_thresh, int device_id);

/* ---- text-line connector ------------------------------------------------------------------
 * Replaces: TextDetector.detect (lib/text_connector/detectors.py:19-49) with the graph builder
 * (text_proposal_graph_builder.py:6-78), Graph.sub_graphs_connected (other.py:20-29) and
 * get_text_lines H (text_proposal_connector.py:21-64) / O (text_proposal_connector_oriented.py:24-105).
 * boxes: r x 4 fp32 [x1,y1,x2,y2], scores: r fp32, (im_h, im_w) = `size`. recs_out: capacity x 9
 * float64 [x1,y1,x2,y2,x3,y3,x4,y4,score]; count_out = number of lines (may exceed capacity ->
 * CTPN_ERR_CAPACITY with count_out set). The NMS(0.2) inside runs on device_id when
 * device_id >= 0 (reference: nms_wrapper.nms -> gpu_nms, detectors.py:29). Host C++ otherwise. */
int ctpn_text_lines(const float* boxes, const float* scores, int r, int im_h, int im_w, int mode,
                    int device_id, double* recs_out, int capacity, int* count_out);
/* The same with a configuration of the caller's (the reference's TextLineCfg, which it reads at run time): cfg8 in the order
 * ctpn_connector_constants reports, NULL = the defaults (ctpn_text_lines is that case). Ranges and precisions as for ctpn_set_param's
 * parameters of the same names (cfg8[0] is MIN_LINE_WIDTH); a value outside them is CTPN_ERR_ARG. Stateless: no ctx is read. */
int ctpn_text_lines_cfg(const float* boxes, const float* scores, int r, int im_h, int im_w, int mode,
                        int device_id, const double* cfg8, double* recs_out, int capacity, int* count_out);
/* The connector's DEFAULTS (the reference's TextLineCfg, lib/text_connector/text_connect_cfg.py:4-12):
 * out8 = {TEXT_PROPOSALS_WIDTH * MIN_NUM_PROPOSALS, MIN_RATIO, LINE_MIN_SCORE, MAX_HORIZONTAL_GAP, TEXT_PROPOSALS_MIN_SCORE,
 * TEXT_PROPOSALS_NMS_THRESH, MIN_V_OVERLAPS, MIN_SIZE_SIM}, the fp32 ones as their fp32 values. The Python mirror's TextDetector() compares the
 * module-level Config with them and raises if a caller has edited one (an edit that would silently do nothing is worse than an error);
 * TextDetector(config=...) is the way to run another configuration. Needs no device. */
int ctpn_connector_constants(double* out8);

/* ---- pages in tiles ---------------------------------------------------------------------------
 * No counterpart in the reference, whose resize_im (ctpn/demo.py:21-25) shrinks every image to 600 px on its short side. A page larger than a
 * ctx's max_h x max_w is detected at its own resolution as overlapping tiles: CTPN's proposals are 16-px columns on a 16-px grid, x is never
 * regressed and the connector sees proposals only, so with tile origins on multiples of 16 every tile's anchor grid is the page's, each page
 * cell is owned by exactly one tile, and a text line across a seam is one chain of columns to the ordinary connector. The five functions are
 * stateless (no ctx; plan and merge need no device); the forward on the tiles is ctpn_detect_submit / ctpn_detect_collect at scale 1.
 *
 * ctpn_page_plan. tile_h, tile_w: multiples of 16; overlap: a multiple of 32 in 0 .. min(tile_h, tile_w) / 2; page sides 16 .. 16384; anything
 * else is CTPN_ERR_ARG. Per axis of length L with tile T and overlap V: L <= T is one tile at origin 0; otherwise the stride is S = T - V and
 * k = ceil((L - T) / S) + 1 tiles sit at j S (the last tile's valid part is wider than V). valid = min(T, L - origin). Tile j owns the
 * half-open range from origin_j + V / 2 (0 for the first tile) to origin_{j+1} + V / 2 (L for the last). Tiles are numbered row-major;
 * tiles8: one record {oy, ox, valid_h, valid_w, own_y0, own_y1, own_x0, own_x1} of eight ints per tile, page coordinates. The owned rectangles
 * partition the page; origins and own bounds other than the page's end are multiples of 16. count_out = tiles (written even when capacity
 * is too small: CTPN_ERR_CAPACITY; tiles8 == NULL only counts), grid2 (nullable) = {tile rows, tile columns}.
 *
 * ctpn_page_cut. Tiles first .. first + n - 1 of tiles8 out of the page (page_h x page_w x 3 BGR uint8, rows pitch_bytes >= 3 page_w apart;
 * neither the pointer nor the pitch needs any alignment; host or device memory) into out: n x tile_h x tile_w x 3 bytes, host or device memory
 * (a device buffer 4-byte aligned), ready for ctpn_detect_submit(images_on_device = 1). Bytes outside the page are round(PIXEL_MEANS) =
 * {103, 116, 123}: what the 16-bit modes' feed turns into exactly zero, the nearest thing to im_list_to_blob's zero padding that a uint8 feed
 * allows. Every byte of out's n tiles is written, none beyond. Synchronous, on a stream of its own.
 *
 * ctpn_page_merge. rois: n_tiles x roi_capacity x 5 rows [score, x1, y1, x2, y2] as ctpn_detect_collect returns them at scale 1, roi_counts
 * their numbers. A roi of tile t is kept iff its column is owned -- with c = int(x1) >> 4, own_x0 <= 16 c + ox < own_x1 -- and its centre row
 * is: cy = (y1 + y2) * 0.5f in fp32, tile coordinates, (float)(own_y0 - oy) <= cy < (float)(own_y1 - oy). A kept roi is translated by fp32
 * adds of (ox, oy), clipped to x2 <= page_w - 1 and y2 <= page_h - 1, and dropped if x2 - x1 + 1 or y2 - y1 + 1 is below min_size (the
 * proposal layer's filter, again after the page clip). Output in tile order, then roi order: boxes_out capacity x 4, scores_out, src_out =
 * tile * roi_capacity + row. count_out may exceed capacity -> CTPN_ERR_CAPACITY with count_out set.
 *
 * ctpn_page_nms. ctpn_nms's contract and signature, by the page form of the column-decomposed kernels: up to 2^20 boxes in up to 1024 columns
 * int(x1) >> 4, partitioned over many workgroups, one wave per column over the whole chip. The keep list equals ctpn_nms's on every input of
 * its domain: thresh >= 0.1; every box's x-extent inside [16 c, 16 c + 16] of its column c < 1024 (x1 <= x2); of two neighbouring columns
 * at least one without a box narrower than 10 px (neighbours share one pixel column, which is then below a tenth of the wider box). Checked
 * on the host; outside the domain: CTPN_ERR_ARG (ctpn_nms takes anything). Device buffers are cached per device, like ctpn_nms's.
 *
 * ctpn_page_text_lines. ctpn_text_lines_cfg's contract and its records bit for bit -- the same score filter, stable sort and connector --
 * with the NMS in between chosen by nms_form: 0 = ctpn_nms, 1 = ctpn_page_nms (then its domain applies). device_id < 0: host C++, either form.
 *
 * Known limit: a tile clips its proposals to the tile, so a box taller than the overlap whose centre is owned near a seam is cut at the
 * tile's edge: choose the overlap >= the tallest text expected. */
int ctpn_page_plan(int page_h, int page_w, int tile_h, int tile_w, int overlap, int* tiles8, int capacity, int* count_out, int* grid2);
int ctpn_page_cut(int device_id, const uint8_t* page, int page_on_device, int page_h, int page_w, long long pitch_bytes, const int* tiles8,
                  int first, int n, int tile_h, int tile_w, uint8_t* out, int out_on_device, long long capacity_bytes);
int ctpn_page_merge(const int* tiles8, int n_tiles, const float* rois, int roi_capacity, const int* roi_counts, int page_h, int page_w,
                    float min_size, float* boxes_out, float* scores_out, int* src_out, int capacity, int* count_out);
int ctpn_page_nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim, float nms_overlap_thresh, int device_id);
int ctpn_page_text_lines(const float* boxes, const float* scores, int r, int page_h, int page_w, int mode, int device_id, const double* cfg8,
                         int nms_form, double* recs_out, int capacity, int* count_out);

/* ---- result files ---------------------------------------------------------------------------
 * Replaces draw_boxes (ctpn/demo.py:28-52), host C++: the text of data/results/res_<stem>.txt -- one "min_x,min_y,max_x,max_y\r\n" line
 * per text line, coordinates int(coord / scale) (truncation, :43-46), lines skipped where |box[0] - box[1]| < 5 or |box[3] - box[0]| < 5
 * (the reference's scalar comparison, :32) -- and the outline rendering into the BGR image (cv2.line(..., 2): green for score >= 0.9).
 * recs: n_lines x 9 float64 as returned by ctpn_text_lines / ctpn_detect. ctpn_result_text with out == NULL only sizes the text. */
int ctpn_result_text(const double* recs, int n_lines, double scale, char* out, size_t capacity, size_t* bytes_out, int* lines_out);
int ctpn_write_result_file(const char* path, const double* recs, int n_lines, double scale, int* lines_out);
int ctpn_draw_boxes(uint8_t* img_bgr, int h, int w, const double* recs, int n_lines);

/* ---- whole path, batched ------------------------------------------------------------------
 * Replaces the body of ctpn() in ctpn/demo.py:55-68 between imread/resize and draw_boxes for a
 * batch: forward -> proposals -> (boxes / scale) -> text lines. scales: n floats (im_scales[0] of
 * lib/fast_rcnn/test.py:57, 1.0 when the image is already at network resolution).
 * recs_out: n x line_capacity x 9 float64, line_counts: n ints; rois_out (n x capacity x 5, ctpn_proposal_capacity) / roi_counts may be NULL.
 * The proposal layer's four values and the connector's thresholds are the ctx's parameters (ctpn_set_param). */
int ctpn_detect(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w,
                const float* scales, int mode, double* recs_out, int line_capacity, int* line_counts,
                float* rois_out, int* roi_counts);

/* Asynchronous form of ctpn_detect for throughput: submit enqueues the whole device part of a batch (forward on the
 * ctx stream; proposal layer + connector front end + D2H on a second stream) into slot 0 or 1 and returns at once;
 * collect waits for that slot, runs the host part of the connector and fills the outputs. With two slots the host
 * part of batch k and the latency-bound sort / NMS kernels overlap the convolutions of batch k+1. A submit that finds the
 * other slot in flight runs its forward on a second stream and a second set of forward buffers, allocated then (not with
 * keep_acts = 1 or per-stage profiling; without the memory the ctx stays on one set): its first layers run beside the other
 * batch's recurrent tail. Results do not depend on what runs beside what. A slot must be
 * collected before it is submitted to again; images must stay valid until the forward of that submit has run
 * (device pointers: until ctpn_sync or the matching collect).
 * Between a submit and its collect (tests/inflight_cases.py classifies every function that takes a ctx; tests/test_gpu_inflight.py holds it):
 *  - MAY be called, changes neither batch in flight and gives what it gives on an idle ctx: a submit to the other slot and the collects;
 *    ctpn_forward / ctpn_forward_blob / ctpn_forward_ragged, ctpn_get_tensor, ctpn_feat_shape, ctpn_proposals, ctpn_proposals_from_host,
 *    ctpn_proposal_anchors (the "last forward" they read is then the most recent submit's, or the ctpn_forward* called since); ctpn_detect /
 *    ctpn_detect_ragged, which take the free slot (with both slots busy: ctpn_detect_submit's CTPN_ERR_STATE); ctpn_sync, ctpn_stream,
 *    ctpn_host_threads, ctpn_get_option, ctpn_get_param, ctpn_proposal_capacity, ctpn_profile_enable / _reset / _read,
 *    ctpn_debug_forward_sets; the image I/O units, which run on the copy stream and their own buffers: ctpn_decode_jpeg_batch[_device],
 *    ctpn_jpeg_batch_fetch, ctpn_pack_canvas, ctpn_crop_lines, ctpn_encode_jpeg_batch[_device], ctpn_encode_png_batch.
 *  - REFUSED with CTPN_ERR_STATE ("<function>: a submitted batch has not been collected") while either slot is busy, after the ctx has drained
 *    its streams, and harmless to the batches: ctpn_set_option, ctpn_set_param, ctpn_reserve_proposals, ctpn_debug_text_lines, and the weight
 *    loads ctpn_load_weights_host, ctpn_load_weights_device, ctpn_broadcast_weights_rank, ctpn_broadcast_weights (see the weights block).
 *  - ctpn_destroy drains the streams and drops what was in flight. */
int ctpn_detect_submit(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w,
                       const float* scales, int slot);
int ctpn_detect_collect(ctpn_ctx* ctx, int slot, int mode, double* recs_out, int line_capacity, int* line_counts,
                        float* rois_out, int* roi_counts);

/* ctpn_detect / ctpn_detect_submit for a ragged batch (see ctpn_forward_ragged): per image the rois, roi counts, anchors, lines and line
 * counts of that image through ctpn_detect alone. Slots, outputs and ctpn_detect_collect as for the uniform forms. */
int ctpn_detect_ragged(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights,
                       const float* scales, int mode, double* recs_out, int line_capacity, int* line_counts,
                       float* rois_out, int* roi_counts);
int ctpn_detect_submit_ragged(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights,
                              const float* scales, int slot);

/* ---- measurement --------------------------------------------------------------------------
 * When enabled, every kernel launch on the ctx stream is bracketed by hipEvents; ctpn_profile_read
 * returns, per kernel kind, the accumulated milliseconds, launch count and algorithmic work
 * (flops for MFMA kernels, bytes for HBM-bound kernels) since the last reset. Used by bench.py for
 * the roofline object; costs two hipEventRecord per launch. */
#define CTPN_KIND_CONV_FIRST  0   /* preprocess + conv1_1 (direct, VALU)        */
#define CTPN_KIND_CONV_GEMM   1   /* implicit-GEMM conv3x3 (MFMA)               */
#define CTPN_KIND_POOL        2   /* 2x2/2 VALID max-pool                       */
#define CTPN_KIND_GEMM        3   /* LSTM input projection, lstm_o FC, heads    */
#define CTPN_KIND_BILSTM      4   /* persistent recurrent kernel                */
#define CTPN_KIND_DECODE      5   /* softmax + anchor decode + clip + filter    */
#define CTPN_KIND_SORT        6   /* per-image key sort + gather                */
#define CTPN_KIND_NMS         7   /* greedy NMS                                 */
#define CTPN_KIND_COUNT       8
/* on = 1: a hipEvent pair around every stage (CTPN_KIND_*); on = 2: ONE pair around the 13 conv3x3 launches of a forward and
 * nothing else (42 event records per step cost ~0.2 ms of bubbles at 11 ms / step); on = 0: off. */
int ctpn_profile_enable(ctpn_ctx* ctx, int on);
int ctpn_profile_reset(ctpn_ctx* ctx);
int ctpn_profile_read(ctpn_ctx* ctx, int kind, double* ms, long long* launches, double* work);

/* ---- diagnostics ---------------------------------------------------------------------------
 * One conv3x3 + bias + ReLU (+ 2x2/2 VALID max-pool when fuse_pool) on dense fp32 host tensors, through the same
 * kernels the forward uses (impl 1 = tap-reuse conv3x3.hip, 0 = im2col igemm.hip + pool kernel). in: n x h x w x ci,
 * w_hwio: 3 x 3 x ci x co (TF layout), out_full: n x h x w x co or NULL, out_pool: n x h/2 x w/2 x co or NULL.
 * ci must be a multiple of 32 (fp32) / 64 (bf16, fp16, split), co of 8 (split: <= 64 or a multiple of 128). precision: CTPN_PREC_*.
 * impl 1 = the product kernels (conv3x3), impl 0 = the im2col GEMM as an independent reference (its pool taken on the host).
 * Unit-test hook for shapes VGG never produces. */
/* fp32 -> bf16 exactly as the kernels' epilogues do it: use_hw_instruction 1 = v_cvt_pk_bf16_f32, 0 = integer
 * round-to-nearest-even formula (the two must agree bit for bit on finite inputs). */
int ctpn_debug_cvt_bf16(int device_id, const float* in, uint16_t* out, int n, int use_hw_instruction);
/* The kernels' two LDS-DMA helper forms (conv3x3_base.h: c3_glds16_saddr declares m0 clobbered, c3_glds16_asm saves and restores it around
 * global_load_lds_dwordx4) on the same `bytes` (a multiple of 1024) of src: both outputs must equal src. Guards the clobber form's
 * contract against a compiler that starts to keep state in m0. */
int ctpn_debug_lds_dma(int device_id, const uint8_t* src, size_t bytes, uint8_t* out_clobber, uint8_t* out_keep);
int ctpn_debug_conv3x3(int device_id, const float* in_nhwc, const float* w_hwio, const float* bias, int n, int h, int w,
                       int ci, int co, int precision, int impl, int fuse_pool, float* out_full, float* out_pool);
/* impl 3 (split precision, no pool, out_full given): impl 1 with the dup_hi layout of the layer that feeds the LSTM projection -- the stored
 * pixel is [hi | lo | hi]; out_full is hi + lo as always, and a third plane that is not bit-equal to the hi plane is CTPN_ERR_STATE.
 *
 * Which kernels one conv3x3 layer runs -- the plan launch_conv3x3 computes from the layer's shape and then follows (csrc/conv3x3_plan.h), so
 * what this reports is what ctpn_debug_conv3x3 and the forward launch for that shape. Pure host arithmetic: no device is touched when
 * cu_count > 0; cu_count 0 = the current device's CU count (CTPN_ERR_NODEVICE without one). One call covers the widths w_first ..
 * w_first + w_count - 1 of an n x h x w map with ci -> co channels (the layer's channel counts in every precision): fuse_pool / keep_full as
 * ctpn_debug_conv3x3's fuse_pool / out_full != NULL (without a pool the full map is always kept), dup_hi as the forward passes it for
 * rpn_conv in split precision, conv_p64 / split_edge the ctx options of those names (split precision only; defaults 1, 1). Bias and ReLU are
 * taken as present, as on every layer of the network. plans: w_count x CTPN_CONV_PLAN_INTS ints per width:
 *   [0] main form   0 wr  1 p64  2 t64  3 p_flat  4 p_flat64  5 p_16x16  6 p_8x32  7 p_8x32_half  8 t_flat  9 t_16x16  10 t_8x32
 *   [1] strip kind  0 none  1 edge  2 edge_pool  3 im2col     (the ragged right-hand columns of a 2D tiling)
 *   [2] strip columns (0 without a strip)     [3] w_cover: columns [0, w_cover) are the main launch's, 0 = all
 *   [4] 1 = edge strip in its deep form in the layer's own stream, 0 = forked onto the helper stream (the im2col strip always is)
 *   [5] K split of an edge strip in waves (split precision: 3 or 6 by Ci; the 16-bit modes: 1); 0 without an edge strip
 * ctpn_debug_conv3x3_form_name(kind, id): the short name above of main form (kind 0) / strip kind (kind 1) id, NULL out of range. */
#define CTPN_CONV_PLAN_INTS 6
int ctpn_debug_conv3x3_plan(int precision, int n, int h, int w_first, int w_count, int ci, int co, int fuse_pool, int keep_full, int dup_hi,
                            int conv_p64, int split_edge, int cu_count, int* plans);
const char* ctpn_debug_conv3x3_form_name(int kind, int id);
/* The tile walk of the layer's main launch (csrc/conv3x3_plan.h c3_walk: the struct the persistent and the weights-in-registers launchers
 * copy into their kernel argument, so what this reports is the launch). Arguments as ctpn_debug_conv3x3_plan; out: w_count x
 * CTPN_CONV_WALK_INTS ints per width. p = a persistent form (p64, p_flat, p_flat64, p_16x16, p_8x32, p_8x32_half), wr = the
 * weights-in-registers kernel; a form without a walk (t64, t_*) reports [1] .. [11], [13] as 0.
 *   [0] main form (as above)   [1] tiles_x   [2] tiles_y (per image; stacked: of the whole bordered batch; flat windows: 0)
 *   [3] tiles_n: channel slices   [4] stacked (p, 2D patches without a pool: tile rows run over the bordered batch)
 *   [5] work items of whole tiles (p: pixel tiles x tiles_n; wr: pixel tiles, walked by every slice)
 *   [6] workers (p: the grid; wr: workgroups per group and channel slice)
 *   [7] ht_full: items [0, ht_full) are whole tiles   [8] ht_r: the tiles behind them run as two halves each (p forms that split, [13])
 *   [9] groups (wr: tile ranges, one per XCD)   [10] per_group (wr: tiles per range; the last may be shorter or empty)
 *   [11] workgroups of the launch   [12] 128-byte K chunks per tap (p: window refills per tile)   [13] 1 = the form splits tail tiles
 * ctpn_debug_conv3x3_walk: ctpn_debug_conv3x3 through the product kernels (impl 1, 3) with the main launch planned and walked as on a device of
 * cu_count CUs (1 .. the device's own, else CTPN_ERR_ARG; 0 = the device's). Both output maps and 64 guard rows behind each hold 0xC3 bytes
 * before the launch; a border pixel or guard row that changed is CTPN_ERR_STATE naming image and bordered row. At most 2^22 bordered pixels.
 * No product caller passes a CU count: this hook and ctpn_debug_conv1_fused_walk are the only ones. */
#define CTPN_CONV_WALK_INTS 14
int ctpn_debug_conv3x3_walk_plan(int precision, int n, int h, int w_first, int w_count, int ci, int co, int fuse_pool, int keep_full, int dup_hi,
                                 int conv_p64, int split_edge, int cu_count, int* out);
int ctpn_debug_conv3x3_walk(int device_id, const float* in_nhwc, const float* w_hwio, const float* bias, int n, int h, int w,
                            int ci, int co, int precision, int impl, int fuse_pool, int cu_count, float* out_full, float* out_pool);
/* The kernels behind the conv stack, one at a time on caller data (test hooks; null stream, buffers allocated and freed inside). Every output
 * buffer is followed by 64 guard rows and pre-filled with one byte value; a guard byte that changed is CTPN_ERR_STATE.
 *
 * ctpn_debug_lstm_pre_plan: the launch shape launch_lstm_pre computes for `cells` feature-map cells and then follows (csrc/lstm_pre.hip). Pure
 *   host arithmetic; cu_count 0 = the current device's CU count (CTPN_ERR_NODEVICE without one). plan_out[4]:
 *   [0] form 0 small (one wave per 32 cells x four column tiles) / 1 resident (lstm_pre_kernel)   [1] waves per workgroup (small: 1)
 *   [2] workgroups   [3] whole waves of the last workgroup that lie beyond the last cell
 * ctpn_debug_lstm_pre: lstm_pre = x @ wx + bias of an n x hf x wf map. x [cells][512], wx [512][1024], bias [1024], out [cells][1024], gate columns
 *   in TF's order (fw i | j | f | o, then bw) on both sides: the weights go through the chain ctpn_load_weights_* uses, the result's columns are
 *   put back on the host. x is rounded to the mode's operand type and laid out as the bordered map the forward reads, the border filled with 3e4
 *   instead of zeros. CTPN_PREC_BF16 / FP16: launch_lstm_pre with cu_count (0 = the device's; another value plans the launch for that many
 *   CUs), fp16 results; CTPN_PREC_FP32 / SPLIT: the im2col GEMM as the forward sets it up, fp32 results.
 * ctpn_debug_bilstm: the recurrence alone. pre [rows][T][1024] in TF's order (permuted inside; rounded to and stored as fp16 when pre_f16), wh
 *   [2][128][512] = kernel[512:] of fw, bw; out [rows][T][256]. split / fast_gates / pre_f16 as the forward passes them; the two pairs it never
 *   passes (no split: exact gates on fp16 pre, fast gates on fp32 pre) are CTPN_ERR_ARG. *form_out (nullable; set before a device is asked for):
 *   the form launch_bilstm chooses: 0 exact, 1 exact with v_exp / v_rcp gates, 2 split-bf16 16 rows per workgroup, 3 split-bf16 4 rows.
 * ctpn_debug_gemm: out[m][0 .. Co) = a[m] @ w + bias through launch_pack_transpose + launch_igemm (plain A, no ReLU, fp32 out). a [M][K] (rounded to
 *   in_precision: CTPN_PREC_FP32 / BF16 / FP16), w [K][Co], out [M][ldc]: columns Co .. ldc - 1 come back holding the fill (bytes 0xC3), and a
 *   pad column that changed is CTPN_ERR_STATE. K a multiple of 32 (fp32) / 64, Co and ldc of 4. */
int ctpn_debug_lstm_pre_plan(long long cells, int cu_count, int* plan_out);
/* The forward sets of a ctx (test hook; pure host read). A ctx owns one set of forward buffers and one forward stream from ctpn_create; the
 * first ctpn_detect_submit* that finds the other slot in flight adds a second (see ctpn_detect_submit), unless keep_acts is set, per-stage
 * profiling is on or the memory is not there. out4: [0] sets allocated (1 or 2)  [1] the set of the most recent forward (0 or 1)
 * [2] device bytes of set 1 (0 without it)  [3] the set the batch in flight in slot 0 runs on | that of slot 1 << 8 (-1 for an idle slot, as 255). */
int ctpn_debug_forward_sets(ctpn_ctx* ctx, long long* out4);
/* What the library's host side holds in this process right now (test hook; pure host read, no ctx, no device). Every device block, page-locked
 * block, event and stream the host units create is owned by a handle type (csrc/owned.h) that counts it in and out. out4: [0] device bytes
 * [1] page-locked bytes  [2] events  [3] streams. A ctx adds to all four while it lives and ctpn_destroy takes exactly that off again; a
 * stateless entry point (ctpn_resize, ctpn_debug_*) leaves them as it found them, on success and on failure. What stays for the life of the
 * process: ctpn_nms's and ctpn_page_nms's per-device caches, once used. The kernel launchers' few process-wide scratch blocks are not counted. */
int ctpn_debug_live_resources(long long* out4);
int ctpn_debug_lstm_pre(int device_id, const float* x, const float* wx, const float* bias, int n, int hf, int wf, int precision, int cu_count,
                        float* out);
int ctpn_debug_bilstm(int device_id, const float* pre, const float* wh, int rows, int T, int split, int fast_gates, int pre_f16, float* out,
                      int* form_out);
int ctpn_debug_gemm(int device_id, const float* a, const float* w, const float* bias, int M, int K, int Co, int ldc, int in_precision, float* out);
/* The proposal layer's kernels alone (test hooks): decode_kernel -> radix_sort_kernel (+ merge_rank_kernel) -> gather_kernel -> one of three NMS forms.
 * Key order: ascending key = descending score, equal scores by ascending anchor index; the key orders the score's BITS, so -0.0 ranks below
 *   +0.0 where a float comparison calls the two a tie (softmax never produces -0.0; only ctpn_proposals_from_host can hand one in).
 * ctpn_debug_proposal_plan: what a ctpn_proposals* call launches -- the function the call itself computes once and follows (csrc/api_proposals.hip).
 *   Pure host arithmetic, no device. For options nms_columns / nms_prefix, a ctx with (mw_scratch = 1) or without the multi-workgroup NMS's
 *   scratch, n images and every map hf_first .. + hf_count - 1 x wf_first .. + wf_count - 1; im_widths: the n im_info widths (NULL: no image is
 *   narrower than its map). plans[hf_count][wf_count][CTPN_PROPOSAL_PLAN_INTS]:
 *   [0] npad, keys per image in the key buffers   [1] 1 = fill_keys_kernel pads the keys behind the image's anchors
 *   [2] sort: 0 one workgroup per image, 1 segmented (eight workgroups + merge_rank_kernel)   [3] keys per sort workgroup   [4] keys of the last one
 *   [5] merge_rank_kernel workgroups per image (0: none)   [6] NMS: 0 generic (nms_kernel), 1 column form on one workgroup per image, 2 column groups
 *   [7] column-group workgroups per image (0 in the other forms)   [8] prefix pass: 0 none, 1 inside the kernel, 2 a prefix and a full launch
 *       (none above post_nms_topn = 1024: the 4096 best-scored ranks would rarely hold that many survivors, and the pass would run twice)
 * ctpn_debug_proposal_fetch: one intermediate of the ctx's LAST ctpn_proposals / ctpn_proposals_from_host call (n images, per_img = hf x wf x 10
 *   anchors, pre / post its top-N), copied to the host; synchronises the ctx's streams and reads only. CTPN_ERR_CAPACITY below the size given here:
 *   CTPN_PF_BOXES4 n x per_img x 4 fp32 | SORTED_KEYS n x npad uint64, the buffer the gather read | SORTED_BOXES n x pre x 4 fp32 | SORTED_SCORES
 *   n x pre fp32 | SORTED_ANCHOR n x pre int32 (rows of the three at and behind VALID_COUNTS[i] are stale) | VALID_COUNTS n int32 | COLID n x pre
 *   bytes (CTPN_ERR_STATE unless plan [6] was 2) | KEEP_IDX n x post int32 | KEEP_COUNTS n int32 | MW_SCRATCH n x 2048 bytes, zero between calls |
 *   IM_INFO n x 3 fp32, the im_info rows on the device for the kernels behind decode_kernel (up to four images: decode_kernel publishes them).
 * ctpn_debug_proposals_from_heads: ctpn_proposals on caller-supplied heads instead of a forward's -- decode_kernel's production branch (the
 *   pair softmax inside the kernel, rows of 64 floats, the ragged filter), which ctpn_proposals_from_host enters behind. Any ctx, a
 *   ctpn_create_postproc one included. heads: n x hf x wf rows of 64 fp32 as the heads GEMM stores them: [0, 40) ten anchors' (dx, dy, dw, dh),
 *   [40, 60) their (bg, fg) logit pairs, [60, 64) unused (never read). valid_rows: NULL, or n ints -- feature rows of every image of a ragged
 *   batch; the anchors of the rows at and below valid_rows[i] get invalid keys. Shape and pointer checks as ctpn_proposals_from_host. rois_out
 *   n x post x 5, counts_out n; cls_prob_out (n x hf x wf x 20) and bbox_pred_out (n x hf x wf x 40): NULL or what the kernel stored for
 *   rpn_cls_prob_reshape / rpn_bbox_pred. Afterwards ctpn_debug_proposal_fetch and ctpn_proposal_anchors read this call. On a ctx with a
 *   network, ctpn_get_tensor's two proposal tensors are this call's until the next forward.
 * ctpn_debug_sort_keys: launch_sort_keys alone. keys: n_img x per_img; out: n_img x npad (npad = per_img rounded up to a power of two), the buffer
 *   that holds the result. Both device buffers are CTPN_SORT_POISON (a key that reads as valid) wherever the caller's keys are not, and followed
 *   by a guard row (a changed guard byte: CTPN_ERR_STATE). The one-workgroup form leaves [per_img, npad) alone (poison comes back); the segmented
 *   form (segmented = 1; outside up to 4 images of 4097 .. 32768 keys: CTPN_ERR_ARG) pads it with invalid keys (all ones). */
#define CTPN_PROPOSAL_PLAN_INTS 9
#define CTPN_SORT_POISON 0x00000000C3C3C3C3ull
enum { CTPN_PF_BOXES4 = 0, CTPN_PF_SORTED_KEYS, CTPN_PF_SORTED_BOXES, CTPN_PF_SORTED_SCORES, CTPN_PF_SORTED_ANCHOR, CTPN_PF_VALID_COUNTS, CTPN_PF_COLID,
       CTPN_PF_KEEP_IDX, CTPN_PF_KEEP_COUNTS, CTPN_PF_MW_SCRATCH, CTPN_PF_IM_INFO };
int ctpn_debug_proposal_plan(int nms_columns, int nms_prefix, int mw_scratch, int n, int hf_first, int hf_count, int wf_first, int wf_count,
                             int pre_nms_topn, int post_nms_topn, float nms_thresh, const float* im_widths, int* plans);
int ctpn_debug_proposal_fetch(ctpn_ctx* ctx, int what, void* out, size_t capacity_bytes);
int ctpn_debug_sort_keys(int device_id, const unsigned long long* keys, int n_img, int per_img, int segmented, unsigned long long* out);
int ctpn_debug_proposals_from_heads(ctpn_ctx* ctx, const float* heads, int n, int hf, int wf, const float* im_info, const int* valid_rows,
                                    int pre_nms_topn, int post_nms_topn, float nms_thresh, float min_size, float* rois_out, int* counts_out,
                                    float* cls_prob_out, float* bbox_pred_out);
/* The first layer's kernels alone (test hooks; null stream, buffers allocated and freed inside). The weights go through the chain
 * ctpn_load_weights_* uses (w_hwio 3 x 3 x 3 x 64 as the [27][64] block, bias[64], pack_conv1_frags). The image, n x h x w x 3 (h, w >= 16 as in
 * ctpn_forward; at most 64 images and 2^20 pixels), is copied to byte 64 + byte_offset of a device block whose every other byte -- 64 in front
 * of the image, at least 64 behind it -- is the poison value 0x47 (pixel 71; as a float 5.1e4): the image pointer the kernels get is
 * byte_offset mod 4, no dword they may fetch leaves the block, and a byte outside the image used as a pixel shows in the result. Bordered output
 * maps are pre-filled with bytes 0xC3 and followed by 64 guard rows; a border pixel or guard byte that changed is CTPN_ERR_STATE.
 * ctpn_debug_conv1: one conv1_1 kernel. image: uint8, or float32 (image_is_f32; the mean-subtracted blob, byte_offset 0 only). form:
 *     0 conv_first_kernel                          fp32, bf16, fp16             both feeds
 *     1 conv_first_mfma_kernel                     bf16, fp16, split            both feeds
 *     2 image_to_q_kernel + conv_first_p_kernel    bf16, fp16                   uint8 feed
 *   anything else: CTPN_ERR_ARG. out: n x h x w x 64 fp32 (split precision: hi + lo). out_bits (nullable; not fp32): the stored 16-bit values,
 *   n x h x w x 64, split precision n x h x w x [hi(64) | lo(64)]. q_out (nullable; form 2): the whole q-image, n x Hq x Wq x 4 uint16 with
 *   Hq = 8 ceil(h / 8) + 4, Wq = 64 ceil(w / 64) + 8, built into a buffer of 0xC3 bytes -- image pixel (y, x) is q pixel (y + 2, x + 2), the frame
 *   comes back as the fill, and a frame pixel that changed is CTPN_ERR_STATE; the conv reads a second q-image built into zeros, as in the product.
 * ctpn_debug_conv1_fused: the production chain of the 16-bit modes' uint8 feed: launch_image_to_q, then conv1_2 (w2_hwio 3 x 3 x 64 x 64, bias2[64])
 *   with conv1_1 computed inside its window stage and the 2x2 pool fused (conv3x3_wr_kernel<FUSE>). precision bf16 or fp16. out_pool:
 *   n x h/2 x w/2 x 64 fp32, out_bits (nullable) its stored 16-bit values. A shape whose plan has a strip is refused by the launcher: its error. */
int ctpn_debug_conv1(int device_id, const void* image, int image_is_f32, int byte_offset, const float* w_hwio, const float* bias, int n, int h, int w,
                     int precision, int form, float* out, uint16_t* out_bits, uint16_t* q_out);
int ctpn_debug_conv1_fused(int device_id, const uint8_t* image, int byte_offset, const float* w_hwio, const float* bias, const float* w2_hwio,
                           const float* bias2, int n, int h, int w, int precision, float* out_pool, uint16_t* out_bits);
/* ... with conv1_2's launch laid out for cu_count CUs (as ctpn_debug_conv3x3_walk; 0 = the device's own: ctpn_debug_conv1_fused) */
int ctpn_debug_conv1_fused_walk(int device_id, const uint8_t* image, int byte_offset, const float* w_hwio, const float* bias, const float* w2_hwio,
                                const float* bias2, int n, int h, int w, int precision, int cu_count, float* out_pool, uint16_t* out_bits);
/* TextDetector.detect (lib/text_connector/detectors.py:19-49) for ONE image with every step on the device -- score > 0.7 prefix and
 * boxes / scale (lines_prep_kernel), NMS 0.2 (nms_kernel), graph build / chains / line fit / filter_boxes (connect_kernel) -- i.e.
 * the device-connector form of the asynchronous detect path (option connect_device = 1). rois: r x 5 fp32 [score,x1,y1,x2,y2] in
 * descending score order (what proposal_layer returns), r <= 1000. Test hook for the connector kernel. */
int ctpn_debug_connect(int device_id, const float* rois, int r, int im_h, int im_w, float scale, int mode, double* recs_out,
                       int capacity, int* count_out);
/* The text-line tail of ctpn_detect_submit / ctpn_detect_collect on caller-supplied rois: the SAME enqueue function the submit calls
 * (lines_prep_kernel, the connector's NMS 0.2 in the form options nms_columns and the batch size select, connect_kernel with option
 * connect_device = 1) on the ctx's proposal stream, then what the collect does (device records, or connect_lines on the host with
 * connect_device = 0). Works on any ctx, a ctpn_create_postproc one included. rois: n x capacity x 5 fp32 [score,x1,y1,x2,y2] per image in
 * descending score order, roi_counts[n] rows of each are valid (0 .. RPN_POST_NMS_TOP_N); n <= max_batch; im_h x im_w is every image's network size
 * (im_w / 16 columns of the anchor grid), scales[n] (NULL: 1.0) the im_info scale the boxes are divided by. recs_out: n x line_capacity
 * x 9, line_counts[n] as ctpn_detect_collect returns them (the true count also where CTPN_ERR_CAPACITY is returned). keep_out
 * (nullable): n x capacity indices into the image's rois that survived the connector's NMS, keep_counts[n] of them. With option nms_check
 * = 1 a column-decomposed NMS is followed by the generic kernel on the same boxes and a difference is CTPN_ERR_STATE. Test hook.
 * ctpn_debug_text_line_plan: what that tail launches -- the function enqueue_text_lines itself computes once and follows. Pure host arithmetic,
 * no device. For options nms_columns / connect_device, a ctx with (mw_scratch = 1) or without the multi-workgroup NMS's scratch, n images of
 * `rows` rows each (RPN_POST_NMS_TOP_N, 1 .. CTPN_POST_NMS_CAPACITY_MAX) on a map wf columns wide, TEXT_PROPOSALS_NMS_THRESH and the largest
 * im_info scale of the batch. plan[CTPN_TEXT_LINE_PLAN_INTS]:
 *   [0] NMS: 0 generic (nms_kernel), 1 column form on one workgroup of 4 waves per image, 2 column groups, 3 column form on one workgroup of 16
 *       waves per image (more than 1024 rows)
 *   [1] connector: 0 host (connect_lines at collect), 1 connect_kernel (all pairs, up to 1024 rows), 2 connect_large_kernel (anchor-column buckets)
 *   [2] column-group workgroups per image (0 in the other forms) */
#define CTPN_TEXT_LINE_PLAN_INTS 3
int ctpn_debug_text_line_plan(int nms_columns, int connect_device, int mw_scratch, int n, int wf, int rows, float nms_thresh, float max_scale, int* plan);
int ctpn_debug_text_lines(ctpn_ctx* ctx, const float* rois, const int* roi_counts, int n, int im_h, int im_w, const float* scales, int mode,
                          double* recs_out, int line_capacity, int* line_counts, int* keep_out, int* keep_counts);

/* ---- cv2.imread for JPEG files (reference ctpn/demo.py:59), split where the work splits: marker parsing and Huffman decoding on the host
 * (the ctx's worker pool, one image per thread), dequantisation + inverse DCT + chroma upsampling + YCbCr -> BGR on the device. The pixel
 * arithmetic is libjpeg's integer arithmetic (islow IDCT, h2v2 / h2v1 / h1v2 "fancy" upsampling, 16-bit fixed-point colour conversion): the
 * images equal what cv2 / Pillow (libjpeg-turbo) return, bit for bit. The IDCT restates libjpeg-turbo's x86 SIMD islow code (16-bit lanes:
 * coef x q keeps its low 16 bits, four sums per pass wrap, each pass saturates to int16, a block whose rows 1 .. 7 are zero takes row 0 << 2
 * wrapped), which equals jidctint.c on every coefficient an encoder writes from 8-bit pixels and is the pin beyond that (scaled or 16-bit
 * tables, hand-made coefficients); a libjpeg-turbo running WITHOUT SIMD follows jidctint.c's masked range-limit table there and differs. Supported: 8-bit Huffman-coded files, sequential (SOF0 / SOF1) and
 * progressive (SOF2: it differs in the host half only), 1 component or YCbCr 4:4:4 / 4:4:0 / 4:2:2 / 4:2:0, restart intervals, and the
 * eight EXIF orientations, applied the way cv2.imread applies them (an index map in the colour kernel: every size below is the TURNED
 * image's) -- i.e. every JPEG file of the reference's own data/demo. Anything else (CMYK, 4:1:1, arithmetic coding, 12-bit, three components
 * that store RGB by libjpeg's marker rule) and every INCOMPLETE file (entropy data that ends early, a progressive file without its last
 * scans: libjpeg smooths / zero-fills those by rules of its own) is CTPN_ERR_UNSUPPORTED and the caller decodes that file another way
 * (lib/utils/image.py).
 *   ctpn_jpeg_probe            size (as cv2.imread returns it), components and layout of one file: layout & 0xff = luma sampling (1: 4:4:4 /
 *                              gray, 2: 4:2:0, 0x21: 4:2:2 = 2 horizontally, 1 vertically, 0x12: 4:4:0), layout >> 8 = EXIF orientation - 1.
 *                              Host only.
 *   ctpn_jpeg_coef_capacity    int16 elements one h x w image can need in ctpn_jpeg_entropy_decode's coefficient buffer
 *   ctpn_jpeg_entropy_decode   the host half alone (no device needed: the seam the CPU tests use): quantised DCT blocks, natural order,
 *                              component after component, [block rows][block columns][64] each; qt = 3 x 64 quantisation values (natural
 *                              order); layout8 = {STORED h, w, ncomp, horizontal luma sampling | (EXIF orientation - 1) << 8, block columns
 *                              of component 0, 1, block rows of component 0, 1} (vertical luma sampling = block rows of component 0 / 1)
 *   ctpn_decode_jpeg_batch     resize_im(cv2.imread(f)) (reference ctpn/demo.py:59-60) for n files of one size h x w (turned), one layout and
 *                              one orientation: decode,
 *                              then -- unless fx = fy = 1 (or <= 0) -- cv2.resize(fx, fy, INTER_LINEAR) in the same queue. Result: n x
 *                              out_h x out_w x 3 BGR uint8 in device memory owned by the ctx; *images_dev_out is valid for ctpn_forward /
 *                              ctpn_detect_submit(images_on_device = 1) until the second-next call of this function (two buffer sets; the
 *                              ctx orders the decode, the forward that reads it and the buffer's reuse by events: no host wait). The call
 *                              returns when the host half is done and the device half is queued. The buffers grow with the largest
 *                              n x h x w seen; h x w is the FILE size and is not bound by the ctx's max_h x max_w (the output is, once it
 *                              is passed to ctpn_forward).
 *   ctpn_decode_jpeg_files     the same from n PATHS (the reference's cv2.imread(im_name) takes a path): the files are read inside the worker
 *                              threads, right before their entropy decoding.
 *   ctpn_jpeg_probe_files      header scan of n paths on `threads` host threads (<= 0: up to 16): info4[i] = {h, w, components, layout}
 *                              as ctpn_jpeg_probe returns them; h = 0 marks a file ctpn_decode_jpeg_files does not take (unreadable, not a JPEG, or a kind
 *                              that is CTPN_ERR_UNSUPPORTED) -- per-file outcomes are data here, not errors: the caller routes those
 *                              files to its other decoder. Host only, needs no device.
 *   ctpn_jpeg_batch_fetch      copy a batch returned by ctpn_decode_jpeg_batch (still live) to the host, n x out_h x out_w x 3 bytes: for
 *                              callers that also draw on the image (reference ctpn/demo.py:28-52). Waits for that batch's decode. */
int    ctpn_jpeg_probe(const uint8_t* data, size_t len, int* h, int* w, int* ncomp, int* luma_sampling);
size_t ctpn_jpeg_coef_capacity(int h, int w);
int    ctpn_jpeg_entropy_decode(const uint8_t* data, size_t len, int16_t* coef, size_t coef_capacity, uint16_t* qt, int* layout8);
int    ctpn_decode_jpeg_batch(ctpn_ctx* ctx, const uint8_t* const* files, const size_t* sizes, int n, int h, int w, double fx, double fy,
                              const uint8_t** images_dev_out, int* out_h, int* out_w);
int    ctpn_decode_jpeg_files(ctpn_ctx* ctx, const char* const* paths, int n, int h, int w, double fx, double fy,
                              const uint8_t** images_dev_out, int* out_h, int* out_w);
int    ctpn_jpeg_probe_files(const char* const* paths, int n, int* info4, int threads);
int    ctpn_jpeg_batch_fetch(ctpn_ctx* ctx, const uint8_t* images_dev, uint8_t* host_out, size_t capacity);

/* ---- the same with the Huffman decode on the device too (jpeg_huff.hip): additive to ABI 10, no option and no default changes. For
 * SEQUENTIAL files (SOF0 / SOF1: one interleaved scan, what the host half's sequential decoder takes) the host only parses the markers and
 * makes one linear pass over the scan's bytes (byte stuffing removed, cut at the RSTn markers); bytes, Huffman tables and segment table
 * cross in one copy (a tenth of the coefficients' bytes) and the self-synchronising parallel decode writes the coefficients where
 * the IDCT kernel reads them: restart segments cut into subsequences of S bits, one thread each; pass 1 from every subsequence's first
 * bit, sync rounds from the predecessor's exit state until no state changes (at most `subsequences of the longest segment - 1` rounds),
 * a scan of the blocks per subsequence, a write pass, a prefix sum of the DC differences. Every file has a flag word: 0 = its coefficients
 * are the host half's, bit for bit; anything else (an invalid code, a DC category above 11, an AC run past 63, data that ends early, a
 * block or segment count that does not come out) and the library runs the HOST half on that file alone -- status and message are the
 * host's, the two paths cannot disagree about a file. A progressive file is CTPN_ERR_UNSUPPORTED here: route it to the calls above.
 *   ctpn_decode_jpeg_batch_device    ctpn_decode_jpeg_batch's contract, buffers (the same two sets), events and one-layout-per-batch rule;
 *   ctpn_decode_jpeg_files_device    the images are byte-equal to that call's. The call returns when the flag words are back (it waits for
 *                                    the entropy kernels, as the host form waits for its worker threads) and the pixel half is queued.
 *   ctpn_jpeg_entropy_decode_device  the seam the tests use, synchronous: n files of any mix of sizes and layouts; subseq_bits = S, 0 for the
 *                                    default (1024), else a multiple of 32 in 128 .. 4096. coef_out: host memory, n x coef_capacity_per_file
 *                                    int16, file i's part filled exactly as ctpn_jpeg_entropy_decode fills it; qt_out n x 192; layout8_out
 *                                    n x 8; status_out[i] = the status that call returns for file i (per-file outcomes are data: the call
 *                                    itself fails on bad arguments and HIP errors only), except that a progressive file is
 *                                    CTPN_ERR_UNSUPPORTED. ctpn_last_error() holds the message of the last file that failed.
 *   ctpn_jpeg_entropy_device_stats   of the ctx's last device-entropy call: out4 = {files decoded on the device, files handed to the host
 *                                    half because of a flag, subsequences in total, sync rounds run}.
 * A post-processing-only ctx is CTPN_ERR_STATE. */
int    ctpn_decode_jpeg_batch_device(ctpn_ctx* ctx, const uint8_t* const* files, const size_t* sizes, int n, int h, int w, double fx, double fy,
                                     const uint8_t** images_dev_out, int* out_h, int* out_w);
int    ctpn_decode_jpeg_files_device(ctpn_ctx* ctx, const char* const* paths, int n, int h, int w, double fx, double fy,
                                     const uint8_t** images_dev_out, int* out_h, int* out_w);
int    ctpn_jpeg_entropy_decode_device(ctpn_ctx* ctx, const uint8_t* const* files, const size_t* sizes, int n, int subseq_bits, int16_t* coef_out,
                                       size_t coef_capacity_per_file, uint16_t* qt_out, int* layout8_out, int* status_out);
int    ctpn_jpeg_entropy_device_stats(ctpn_ctx* ctx, long long* out4);

/* ---- JPEG files of MIXED sizes into one ragged device batch (jpeg_ragged.hip): additive to ABI 10, no option and no default changes. The
 * calls above take n files of one size, one layout and one orientation; a folder of photographs and scans has many file sizes that resize_im
 * maps to one or two widths, and ctpn_forward_ragged / ctpn_detect_submit_ragged batch images of one width and different heights. These two
 * calls join them: the files of one call may differ in size, component layout (gray, 4:4:4, 4:4:0, 4:2:2, 4:2:0), EXIF orientation and
 * restart interval.
 *   ctpn_decode_jpeg_batch_ragged   file_h[i] x file_w[i]: file i's size as ctpn_jpeg_probe reports it (turned), checked after the parse;
 *                                   factors[i]: its resize_im factor, used as fx = fy (<= 0 or 1: no resize). Every file's width must map to
 *                                   the canvas's -- round-half-even(file_w[i] * factors[i]) == wc -- and its height to 16 .. hc; otherwise
 *                                   CTPN_ERR_ARG naming the file, before any work. Result: a canvas n x hc x wc x 3 BGR uint8 in device memory
 *                                   owned by the ctx; slot i holds cv2.resize(cv2.imread(file i), factors[i]) in rows [0, heights_out[i]) and
 *                                   ZEROS below (lib/utils/blob.py im_list_to_canvas's canvas, byte for byte: image i's rows are what
 *                                   ctpn_decode_jpeg_batch(n = 1, fx = fy = factors[i]) returns for it). entropy_on_device: 0 = Huffman
 *                                   decoding on the ctx's host pool (progressive files included), 1 = on the device (a progressive file is
 *                                   CTPN_ERR_UNSUPPORTED; a raised flag word sends that file alone to the host half). Per-file errors carry
 *                                   the file's index. Buffers and events are ctpn_decode_jpeg_batch's -- the same two sets, in turn with
 *                                   that call: *canvas_dev_out is valid for ctpn_forward_ragged / ctpn_detect_submit_ragged(canvas_on_device
 *                                   = 1) and ctpn_jpeg_batch_fetch (n x hc x wc x 3 bytes) until the second-next decode call of either
 *                                   kind. Coefficients and planes are packed per file (each file's own ctpn_jpeg_coef_capacity at a
 *                                   prefix-summed base), not n x the largest. The file-size BGR image is never stored: colour conversion
 *                                   and resize are one kernel over the canvas.
 *   ctpn_decode_jpeg_files_ragged   the same from n PATHS.
 * A post-processing-only ctx is CTPN_ERR_STATE. */
int    ctpn_decode_jpeg_batch_ragged(ctpn_ctx* ctx, const uint8_t* const* files, const size_t* sizes, int n, const int* file_h, const int* file_w,
                                     const double* factors, int hc, int wc, int entropy_on_device, const uint8_t** canvas_dev_out, int* heights_out);
int    ctpn_decode_jpeg_files_ragged(ctpn_ctx* ctx, const char* const* paths, int n, const int* file_h, const int* file_w, const double* factors,
                                     int hc, int wc, int entropy_on_device, const uint8_t** canvas_dev_out, int* heights_out);

/* ---- Decoded images and PNG files of MIXED sizes into one ragged device batch (canvas_pack.hip): additive to ABI 10, no option and no
 * default changes. The two calls above build a ragged canvas from JPEG files; these two build it from every other source the library takes:
 * BGR uint8 images already decoded, on the host or on the device, and PNG files. One kernel resizes every image by its own factor into its
 * slot and writes the zeros below it: no per-image resize call, no canvas built on the host, no memset.
 *   ctpn_pack_canvas               images[i]: img_h[i] x img_w[i] x 3 BGR uint8, rows pitches[i] bytes apart (pitches NULL: 3 x img_w[i]; a
 *                                  pitch below that is CTPN_ERR_ARG); no alignment of pointer or pitch is required. factors[i]: the image's
 *                                  resize_im factor, used as fx = fy (<= 0 or 1: no resize). Every width must map to the canvas's --
 *                                  ctpn_resize_dims(img_h[i], img_w[i], factors[i], factors[i]) gives wc -- and every height to 16 .. hc;
 *                                  otherwise CTPN_ERR_ARG naming the image, before any work, as is a NULL image. n above the ctx's max_batch
 *                                  or a canvas above max_h x max_w is CTPN_ERR_ARG. Result: a canvas n x hc x wc x 3 BGR uint8 in device
 *                                  memory owned by the ctx; slot i holds cv2.resize(image i, factors[i]) in rows [0, heights_out[i]) and
 *                                  ZEROS below (lib/utils/blob.py im_list_to_canvas's canvas, byte for byte: image i's rows are what
 *                                  ctpn_resize returns for it alone).
 *                                  images_on_device = 0: the images are copied into a page-locked block of the ctx at prefix-summed
 *                                  offsets (rows at pitch 3 w, on the ctx's host pool) and cross in ONE copy together with their
 *                                  descriptors; they may be reused when the call returns. The zero-padded canvas never crosses.
 *                                  images_on_device = 1: device pointers, read in place and never written; a pointer that is a live
 *                                  batch of a decode call is waited for in the copy queue, any other memory must be complete when the
 *                                  call is made and stay unchanged until work that reads the canvas has been waited for.
 *                                  Buffers and events are ctpn_decode_jpeg_batch's -- the same two sets, in turn with the JPEG calls:
 *                                  *canvas_dev_out is valid for ctpn_forward_ragged / ctpn_detect_submit_ragged(canvas_on_device = 1) --
 *                                  which wait for it by pointer match, as for the JPEG canvas --, the ragged writers and crops and
 *                                  ctpn_jpeg_batch_fetch (n x hc x wc x 3 bytes) until the second-next decode or pack call of any
 *                                  kind. Everything runs on the ctx's copy queue; the call returns when the work is queued.
 *   ctpn_decode_png_files_ragged   n PNG files of file_h[i] x file_w[i] (ctpn_png_probe_files) through the same path: the ctx's host pool
 *                                  runs ctpn_png_decode's decoder, one file per worker, straight into the page-locked block at the file's
 *                                  offset (gray, palette and RGBA files are expanded to BGR there). A file of another size than announced
 *                                  is CTPN_ERR_ARG; a decoder error (bad CRC, a missing file, CTPN_ERR_UNSUPPORTED for 16-bit samples)
 *                                  fails the call with that file's code; ctpn_last_error() names the file's index and path.
 * A post-processing-only ctx is CTPN_ERR_STATE; a NULL ctx in a process without a device CTPN_ERR_NODEVICE (there is no host form).
 * Rate (tools/canvas_pack_throughput.py, profiles/canvas_pack_throughput.json): on a folder of PNG files of 16 sizes, files to text lines,
 * 2.5 - 3.2 x the size-grouped path and 11 - 14 x a canvas built on the host. The kernel alone has not been timed. */
int    ctpn_pack_canvas(ctpn_ctx* ctx, const uint8_t* const* images, const int* img_h, const int* img_w, const long long* pitches /* NULL: 3 w */,
                        int images_on_device, int n, const double* factors, int hc, int wc, const uint8_t** canvas_dev_out, int* heights_out);
int    ctpn_decode_png_files_ragged(ctpn_ctx* ctx, const char* const* paths, int n, const int* file_h, const int* file_w, const double* factors,
                                    int hc, int wc, const uint8_t** canvas_dev_out, int* heights_out);

/* ---- cv2.imwrite for the annotated result images (reference ctpn/demo.py:28-52: draw_boxes, cv2.resize by 1 / scale, cv2.imwrite), the mirror
 * image of the JPEG reader above, split where the work splits: BGR -> YCbCr, 2 x 2 chroma downsampling, the 8 x 8 forward DCT and the
 * quantiser on the device (one launch; the outlines and the resize before it, so annotated pixels never visit the host), baseline Huffman
 * coding and the file writing on the ctx's worker pool, one image per thread. The arithmetic is libjpeg's, integer for integer (jccolor.c,
 * jcsample.c h2v2_downsample, jfdctint.c islow, jcdctmgr.c's quantiser, jccoefct.c's dummy blocks, jchuff.c with the standard tables K.3 - K.6),
 * the marker sequence libjpeg's (SOI, JFIF APP0, DQT 0, DQT 1, SOF0, four DHT, SOS, data, EOI): the files are byte-equal to Pillow's
 * save(quality = q, subsampling = 2) (libjpeg-turbo), which is what cv2.imwrite writes with its defaults at q = 95. Parity with a real
 * cv2.imwrite is UNPINNED (cv2 is not installed). Always 4:2:0, three components; no optimised tables, restart markers or EXIF.
 *   ctpn_jpeg_encode_capacity   upper bound of the bytes one h x w file can need (0 for a bad size): header + 416 bytes per block (a block
 *                               codes into at most 1660 bits, every byte of which may need a stuffed zero) + padding + EOI
 *   ctpn_jpeg_entropy_encode    the host half alone (needs no device): coefficients, layout8 and qt EXACTLY as ctpn_jpeg_entropy_decode returns
 *                               them -- NATURAL order (the device half writes zig-zag order; the library converts where the two meet) -- so
 *                               decode followed by encode reproduces a baseline 3-component file written with the standard tables byte for
 *                               byte. *bytes_out is the file size, also when it exceeds capacity (CTPN_ERR_CAPACITY; out == NULL with
 *                               capacity 0 sizes the file). CTPN_ERR_UNSUPPORTED: other than 3 components, an EXIF orientation, quantisation
 *                               values above 255, different tables for Cb and Cr
 *   ctpn_encode_jpeg_batch      n images of h x w x 3 BGR uint8, in HBM (images_on_device) or on the host (copied in the ctx's copy queue) ->
 *                               n files in caller memory: out[i] holds capacities[i] bytes, bytes_out[i] receives the size (also of a file
 *                               that did not fit: CTPN_ERR_CAPACITY). quality 1 .. 100 (else CTPN_ERR_ARG)
 *   ctpn_write_annotated_files  one batch of the demo: the outlines of recs (n x line_capacity x 9 float64, line_counts[i] lines each, as
 *                               ctpn_detect_collect returns them) drawn exactly as ctpn_draw_boxes draws them, cv2.resize by 1 / scale
 *                               (nothing for scale 1), and paths[i] written at `quality`. images_dev: n x h x w x 3 in HBM -- a live batch of
 *                               ctpn_decode_jpeg_batch, or any device buffer whose contents are complete; it is not modified (the drawing
 *                               goes onto a copy owned by the ctx: the decoder's buffer may still feed a forward). A path that cannot be
 *                               written is CTPN_ERR_ARG, its name in ctpn_last_error().
 * The two ctx calls run their device half in the ctx's copy queue, behind the decode that produced the batch and in front of the next one,
 * and return when the files are coded; their buffers grow to the largest batch seen and are then reused (no allocation per call). */
size_t ctpn_jpeg_encode_capacity(int h, int w);
int    ctpn_jpeg_entropy_encode(const int16_t* coef, const int* layout8, const uint16_t* qt, uint8_t* out, size_t capacity, size_t* bytes_out);
int    ctpn_encode_jpeg_batch(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w, int quality, uint8_t* const* out,
                              const size_t* capacities, size_t* bytes_out);
int    ctpn_write_annotated_files(ctpn_ctx* ctx, const uint8_t* images_dev, int n, int h, int w, const double* recs, int line_capacity,
                                  const int* line_counts, double scale, const char* const* paths, int quality);

/* ---- the same with the Huffman coding on the device too (jpeg_huff_enc.hip): additive to ABI 10, no option and no default changes. A block's
 * code depends only on its own coefficients and on the previous block's DC, which lies in the coefficient array, so there is nothing to
 * synchronise: a length pass (one thread per block), a prefix sum per image, a write pass that runs the length pass's text once more into
 * the unstuffed stream, then the 0xFF count per 64-byte chunk, its prefix sum and the stuffed scan body. The host writes header and EOI.
 * Only the result words (16 bytes per image) and the files' own scan bytes cross to the host -- sizes first, then what they say -- instead
 * of every coefficient. An image whose flag is raised (a DC difference above 11 bits, an AC coefficient above 10, a count that does not
 * come out) or that has more than 2^20 blocks is coded by the HOST half alone, so status and message are the host's: the two forms cannot
 * disagree about an image.
 *   ctpn_encode_jpeg_batch_device          arguments, contract, queue, events and error codes of ctpn_encode_jpeg_batch /
 *   ctpn_write_annotated_files_device      ctpn_write_annotated_files; the files are byte-equal to theirs
 *   ctpn_jpeg_entropy_encode_device        the seam the tests use, synchronous: n coefficient sets of any mix of sizes and of the layouts
 *                                          ctpn_jpeg_entropy_encode takes, in host memory in NATURAL order: coef[i], layout8 + 8 i and
 *                                          qt + 192 i are that call's arguments, out[i] / capacities[i] / bytes_out[i] are filled as it fills
 *                                          them (CTPN_ERR_CAPACITY with the size set for a file that does not fit; out[i] == NULL with
 *                                          capacity 0 sizes it), status_out[i] is its status. Per-file outcomes are data: the call itself
 *                                          fails on bad arguments and HIP errors only; ctpn_last_error() holds the last failed file's message
 *   ctpn_jpeg_entropy_encode_device_stats  of the ctx's last device-entropy encode: out4 = {files coded on the device, files handed to the
 *                                          host half, blocks coded on the device, bytes copied device to host} */
int    ctpn_encode_jpeg_batch_device(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w, int quality, uint8_t* const* out,
                                     const size_t* capacities, size_t* bytes_out);
int    ctpn_write_annotated_files_device(ctpn_ctx* ctx, const uint8_t* images_dev, int n, int h, int w, const double* recs, int line_capacity,
                                         const int* line_counts, double scale, const char* const* paths, int quality);
int    ctpn_jpeg_entropy_encode_device(ctpn_ctx* ctx, const int16_t* const* coef, const int* layout8, const uint16_t* qt, int n, uint8_t* const* out,
                                       const size_t* capacities, size_t* bytes_out, int* status_out);
int    ctpn_jpeg_entropy_encode_device_stats(ctpn_ctx* ctx, long long* out4);

/* ---- Rectified crops of the detected text lines, cut out on the device: one image of fixed height per line, what a recogniser behind the
 * detector reads. Not part of the reference (its demo stops at the outlines); additive to ABI 10. The batch's pixels are in HBM already
 * (ctpn_decode_jpeg_batch) and stay there: only the crops cross to the host, if at all. The rate of the kernel is unmeasured.
 * A line is a record [x0,y0,x1,y1,x2,y2,x3,y3,score] as ctpn_text_lines / ctpn_detect_collect return it, in the coordinates of the image
 * that was fed: P0 top-left, P1 top-right, P2 bottom-left, P3 bottom-right (the order ctpn_draw_boxes connects them).
 *   width   top = |P1-P0|, bottom = |P3-P2|, left = |P2-P0|, right = |P3-P1| (sqrt(dx*dx + dy*dy), double, no contraction), wlen = (top +
 *           bottom) / 2, hlen = max((left + right) / 2, 1); Wc = nearbyint(crop_h * wlen / hlen) (half to even) clamped to [1, max_w]: a
 *           longer line is squeezed to max_w, not cut
 *   pixel   output pixel (u, v), 0 <= u < Wc, 0 <= v < crop_h: s = (u + 0.5) / Wc, t = (v + 0.5) / crop_h, tx = x0 + s*(x1-x0), bx = x2 +
 *           s*(x3-x2), X = tx + t*(bx-tx) - 0.5 (Y likewise), in double in this order; then ctpn_resize's uint8 arithmetic at (X, Y): float
 *           position, 11-bit weights, the same integer formula -- with the image's border replicated on BOTH axes, so a line that hangs
 *           over the border reads border pixels (an affine box whose size equals its crop's is an exact copy)
 *   layout  image 0's lines, then image 1's, ...: total x crop_h x max_w x 3 BGR uint8; columns >= Wc hold pad_value. EVERY line gets a
 *           crop (ctpn_draw_boxes skips thin ones; filtering is the caller's business)
 *   ctpn_line_crop_width   Wc of one record. Pure: no ctx, no device.
 *   ctpn_crop_lines        images: n x h x w x 3 BGR uint8 in HBM (images_on_device: a live batch of ctpn_decode_jpeg_batch -- its decode
 *                          is waited for in the queue --, or any device buffer whose contents are complete) or on the host (copied into a
 *                          ctx-owned buffer). recs / line_capacity / line_counts as in ctpn_write_annotated_files. crops_out: capacity_bytes
 *                          bytes on the host, or (crops_on_device) in HBM, 4-byte aligned; widths_out (nullable): total ints. *total_out
 *                          is always written. crops_out == NULL with capacity_bytes == 0 SIZES the call: widths and total, no launch.
 *                          Runs in the ctx's copy queue and returns when crops_out is complete (host output: after the copy back; device
 *                          output: after the kernel). CTPN_ERR_CAPACITY: capacity_bytes < total * crop_h * max_w * 3; CTPN_ERR_STATE: a
 *                          post-processing-only ctx; CTPN_ERR_ARG: crop_h outside 1 .. 256, max_w < 4, not a multiple of 4 (a thread
 *                          stores four pixels as three dwords) or > 65535, pad_value outside 0 .. 255, a coordinate that is not finite.
 *                          No lines at all is CTPN_OK. The buffers grow to the largest call seen and are then reused. */
int    ctpn_line_crop_width(const double* rec9, int crop_h, int max_w, int* width_out);
int    ctpn_crop_lines(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs, int line_capacity,
                       const int* line_counts, int crop_h, int max_w, int pad_value, uint8_t* crops_out, int crops_on_device,
                       size_t capacity_bytes, int* widths_out, int* total_out);

/* ---- JPEG files of images of MIXED sizes in one call, and the text-line crops written as files where they are cut: additive to ABI 10.
 * The writer's pixel half over a table of images (jpeg_enc.hip, jpeg_fdct_mixed_kernel): one descriptor per image -- size, row pitch,
 * place in the source, block grid, place of its coefficients -- and a one-dimensional grid over the call's work items (one MCU row by 8
 * MCUs each), whose workgroups find their image by a binary search of the items' prefix sums. The arithmetic is the uniform kernel's own
 * text, so every file is byte-equal to ctpn_encode_jpeg_batch's of that image alone (and to Pillow's). Always 4:2:0, standard tables.
 * Both entropy forms: the plain names code on the ctx's host pool, the _device names on the device (an image whose flag is raised goes to
 * the host half, as in ctpn_encode_jpeg_batch_device; ctpn_jpeg_entropy_encode_device_stats counts the call's files). Measured end to end only: docs/decode_pipeline.md, "Crops out".
 *   ctpn_encode_jpeg_mixed         n BGR uint8 images in ONE source buffer: image i is heights[i] x widths[i] (1 .. 65535 each), its first
 *   ctpn_encode_jpeg_mixed_device  pixel offsets[i] bytes into `source`, its rows pitches[i] >= 3 widths[i] bytes apart; the bytes between a
 *                                  row's end and the next row never enter a file. source on the host: source_bytes is its size, every image
 *                                  must lie inside it, and it is copied in the ctx's copy queue (with slack behind it). source in HBM
 *                                  (source_on_device; source_bytes is not read): a live batch of ctpn_decode_jpeg_batch is waited for in
 *                                  the queue, any other buffer must be complete. The pixel read takes whole aligned dwords: a device
 *                                  source must be READABLE over the aligned dwords its pixels touch -- at most three bytes past an image's
 *                                  last pixel and three in front of its first (nothing outside the pixels where rows start 4-byte
 *                                  aligned). This is ctpn_encode_jpeg_batch's contract for device images too. out / capacities /
 *                                  bytes_out: as in ctpn_encode_jpeg_batch -- out[i] holds capacities[i] bytes, bytes_out[i] receives the
 *                                  size, also of a file that did not fit (CTPN_ERR_CAPACITY; out[i] == NULL with capacity 0 sizes it);
 *                                  ctpn_jpeg_encode_capacity(heights[i], widths[i]) always fits. CTPN_ERR_ARG: n <= 0, a null pointer, a
 *                                  size outside 1 .. 65535, a pitch below 3 widths[i], a pitch or offset of 2^40 bytes or more, an image outside
 *                                  source_bytes (host source),
 *                                  quality outside 1 .. 100, more than 2^31 - 1 work items; CTPN_ERR_STATE: a post-processing-only ctx
 *   ctpn_write_line_crops          ctpn_crop_lines' arguments without the output buffer, plus quality and paths[total] (image 0's lines,
 *   ctpn_write_line_crops_device   then image 1's, ...): the crops are cut into a buffer the ctx owns (the same kernel, the same pixels)
 *                                  and coded there, crop k as a crop_h x Wc_k image at pitch 3 max_w -- the pad columns never enter a
 *                                  file, no crop visits the host. The ctx's pool writes the files; the call returns when they are
 *                                  written. widths_out (nullable): total ints; *total_out is always written. paths == NULL SIZES the
 *                                  call: widths and total, no launch. No lines at all is CTPN_OK. A path that cannot be written (or is
 *                                  NULL) is CTPN_ERR_ARG, its name in ctpn_last_error(); quality outside 1 .. 100 is CTPN_ERR_ARG; the
 *                                  remaining errors are ctpn_crop_lines' and the writer's.
 * All four run in the ctx's copy queue, behind the decode that produced the batch and in front of the next one; their buffers (the
 * descriptor table and its page-locked copy among them) grow to the largest call seen and are then reused. */
int    ctpn_encode_jpeg_mixed(ctpn_ctx* ctx, const uint8_t* source, int source_on_device, size_t source_bytes, int n, const int* heights,
                              const int* widths, const size_t* pitches, const size_t* offsets, int quality, uint8_t* const* out,
                              const size_t* capacities, size_t* bytes_out);
int    ctpn_encode_jpeg_mixed_device(ctpn_ctx* ctx, const uint8_t* source, int source_on_device, size_t source_bytes, int n, const int* heights,
                                     const int* widths, const size_t* pitches, const size_t* offsets, int quality, uint8_t* const* out,
                                     const size_t* capacities, size_t* bytes_out);
int    ctpn_write_line_crops(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs, int line_capacity,
                             const int* line_counts, int crop_h, int max_w, int pad_value, int quality, const char* const* paths,
                             int* widths_out, int* total_out);
int    ctpn_write_line_crops_device(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs,
                                    int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value, int quality,
                                    const char* const* paths, int* widths_out, int* total_out);

/* ---- Ragged batches OUT: the annotated writer and the crops over a ragged canvas: additive to ABI 10, no option and no default changes.
 * A ragged batch is what ctpn_forward_ragged defines: a canvas n x hc x w x 3 BGR uint8 plus heights[n], 16 <= heights[i] <= hc; image i
 * is rows [0, heights[i]) of slot i; the rows below it may hold anything and are never read as pixels. Each call's result for image i
 * is, byte for byte, what the uniform call of the same name gives for that image ALONE -- rows [0, heights[i]) of slot i passed as n = 1,
 * h = heights[i], w, with that image's lines and (the annotated writer) that image's scale. Nothing about JPEG coding, drawing, resizing
 * or crop arithmetic is redefined: one copy of each body serves both forms (draw_boxes_kernel's body, resize_pixel.h, crop_pixel.h,
 * encode_mixed_dev).
 *   ctpn_write_annotated_files_ragged          the outlines of recs drawn per slot, bounded by the image's own height; every image resized
 *   ctpn_write_annotated_files_ragged_device   by its OWN 1 / scales[i] into an output of its own size (dh_i = round-half-even(heights[i] /
 *                                              scales[i]), dw_i likewise from w), all images of the call in one launch over a descriptor
 *                                              table (resize_mixed.hip: ctpn_resize's uint8 arithmetic); an image at scale 1 is coded where
 *                                              it lies. Then paths[i] written at `quality` by the mixed-size encoder. scales: n doubles.
 *                                              _device: the Huffman coding on the device too; the files are byte-equal.
 *   ctpn_crop_lines_ragged                     ctpn_crop_lines / ctpn_write_line_crops[_device] with a line's image taken from slot
 *   ctpn_write_line_crops_ragged               `img` of the canvas and the row axis clamped at heights[img] - 1: a line that hangs below
 *   ctpn_write_line_crops_ragged_device        its image reads the image's last row, never a canvas row. Everything else -- layout of recs /
 *                                              line_capacity / line_counts, lines in image order, the sizing forms (crops_out == NULL with
 *                                              capacity 0; paths == NULL), *total_out always written, no lines at all is CTPN_OK, geometry
 *                                              limits -- is the uniform call's.
 * canvas: in HBM (canvas_on_device: a live canvas of ctpn_decode_jpeg_*_ragged is waited for in the copy queue; any other buffer must be
 * complete) or on the host (copied into a ctx-owned buffer in the copy queue). A caller's canvas is never modified: the outlines go onto
 * the ctx's copy. Everything runs in the ctx's copy queue, behind the decode that produced the canvas and in front of the next one; the
 * calls return when their files are written or their output is complete; buffers grow to the largest call seen and are then reused.
 * CTPN_ERR_ARG, before any device work and naming the image: a null pointer, n <= 0, a height outside 16 .. hc, a scale that is not finite
 * and positive, a resized size outside 1 .. 65535, quality outside 1 .. 100; a path that cannot be written (its name in
 * ctpn_last_error()). CTPN_ERR_STATE: a post-processing-only ctx. Measured end to end: docs/decode_pipeline.md, "Ragged batches out". */
int    ctpn_write_annotated_files_ragged(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights,
                                         const double* recs, int line_capacity, const int* line_counts, const double* scales,
                                         const char* const* paths, int quality);
int    ctpn_write_annotated_files_ragged_device(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights,
                                                const double* recs, int line_capacity, const int* line_counts, const double* scales,
                                                const char* const* paths, int quality);
int    ctpn_crop_lines_ragged(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights, const double* recs,
                              int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value, uint8_t* crops_out,
                              int crops_on_device, size_t capacity_bytes, int* widths_out, int* total_out);
int    ctpn_write_line_crops_ragged(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights,
                                    const double* recs, int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value, int quality,
                                    const char* const* paths, int* widths_out, int* total_out);
int    ctpn_write_line_crops_ragged_device(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights,
                                           const double* recs, int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value,
                                           int quality, const char* const* paths, int* widths_out, int* total_out);

/* ---- cv2.imread for PNG files (reference ctpn/demo.py:59; data/demo holds .jpg and .png). HOST ONLY, by the nature of READING the format: one
 * DEFLATE stream (zlib's inflate, the library libpng itself sits on) and row filters that chain from row to row -- nothing a GPU is for. One
 * file per host thread, straight into the caller's batch buffer, which ctpn_detect_submit / ctpn_forward take as host images (one
 * host-to-device copy per batch). libpng's IMREAD_COLOR transforms restated: RGB / RGBA -> BGR with the alpha dropped, gray 1 / 2 / 4 / 8
 * bit and gray + alpha -> B = G = R, palette images through PLTE (tRNS ignored), Adam7 interlacing; critical-chunk CRCs and the zlib
 * checksum are verified. 16-bit files are CTPN_ERR_UNSUPPORTED. Byte-equal to Pillow's decode (tests/test_png.py). Needs no device.
 *   ctpn_png_probe          size, colour type and bit depth from the header
 *   ctpn_png_decode         one file in memory -> h x w x 3 BGR uint8 (capacity in bytes)
 *   ctpn_png_probe_files    info4[i] = {h, w, colour type, bit depth} of n paths on `threads` host threads (<= 0: up to 16); h = 0 marks a
 *                           file ctpn_decode_png_files does not take (unreadable, not a PNG, 16-bit): data, not an error
 *   ctpn_decode_png_files   n files of one size h x w -> n x h x w x 3 BGR uint8 in the caller's host buffer, one file per thread
 *                           (threads <= 0: up to 32); the first failing file is the call's error, its path in ctpn_last_error()
 *   ctpn_debug_png_backend  which DEFLATE back end decodes: returns 1 = libdeflate (dlopen'ed libdeflate.so.0), 0 = zlib's inflate();
 *                           zlib_only = 1 / 0 forces zlib / lifts that (process-wide; < 0 only asks). Test hook: both give the same bytes. */
int    ctpn_debug_png_backend(int zlib_only);
int    ctpn_png_probe(const uint8_t* data, size_t len, int* h, int* w, int* color_type, int* bit_depth);
int    ctpn_png_decode(const uint8_t* data, size_t len, uint8_t* bgr_out, size_t capacity);
int    ctpn_png_probe_files(const char* const* paths, int n, int* info4, int threads);
int    ctpn_decode_png_files(const char* const* paths, int n, int h, int w, uint8_t* bgr_out, int threads);

/* ---- cv2.imwrite for PNG-named result images (reference ctpn/demo.py:28-52: draw_boxes, cv2.resize by 1 / scale, cv2.imwrite under the
 * input's own name, and data/demo holds .png files). Additive to ABI 10, no option and no default changes. "Host work by nature" holds for
 * READING a PNG file; writing one parallelises: the Sub filter reads raw pixels only, and a DEFLATE stream may be tokenised in independent
 * pieces. The file, defined exactly (docs/decode_pipeline.md, "PNG out"): signature, IHDR (8-bit RGB), ONE IDAT, IEND; zlib stream 78 01,
 * one dynamic-Huffman block, Adler-32; every row filtered with Sub; the filtered stream cut into pieces of 256 bytes, each tokenised on its
 * own, greedily, with two candidate matches per position -- a run of the byte before (distance 1) and a repeat of the row above (distance
 * 1 + 3 w, where that is within 32768) --, the longer taken from 3 bytes on (distance 1 on a tie); a literal/length code built from the
 * image's own histogram, limited to 15 bits; a fixed two-symbol distance code. cv2's own writer uses the Sub filter and a run-length match
 * strategy too; the BYTES are not pinned against it or Pillow (other match finders), parity is defined on the decoded pixels, which are
 * exact: zlib, Pillow and ctpn_png_decode return the input from every file. The device form's files equal the host form's byte for byte.
 *   ctpn_png_encode_capacity        upper bound of one h x w file (0 for a bad size): a token codes at least one stream byte in at most 15
 *                                   bits (a literal: one code; a match: 15 + 5 + 1 + 13 bits for three bytes or more), so the block is below
 *                                   2 bytes per stream byte + 171 (header of 1338 bits, EOB, padding); the frame adds 63
 *   ctpn_png_encode                 the host form (needs no device): h x w x 3 BGR uint8, any size up to 65535 x 65535. *bytes_out is the file
 *                                   size, also when it exceeds capacity (CTPN_ERR_CAPACITY; out == NULL with capacity 0 sizes the file)
 *   ctpn_encode_png_batch           the contract of ctpn_encode_jpeg_batch without `quality`: histogram, length, prefix-sum and write passes
 *                                   on the device (png_enc.hip), the code tables and the framing on the ctx's worker pool
 *   ctpn_write_annotated_png_files  the contract of ctpn_write_annotated_files: outlines on a ctx-owned copy, cv2.resize by 1 / scale, then the
 *                                   PNG passes. Takes host images too (images_on_device = 0: PNG batches are decoded on the host; they are
 *                                   copied in the ctx's copy queue)
 *   ctpn_png_encode_device_stats    of the ctx's last PNG call: out4 = {files coded on the device, files handed to the host form, pieces coded
 *                                   on the device, bytes copied device to host}
 * Both ctx calls run in the ctx's copy queue (a live batch of ctpn_decode_jpeg_batch is waited for there), return when the files are coded,
 * and keep buffers that grow to the largest call seen. Only the histograms (1144 bytes per image), one result record (16 bytes) and the
 * files' own bytes cross to the host. An image whose flag is raised is coded by the host form alone. CTPN_ERR_ARG, before any allocation
 * or launch, when h (1 + 3 w) > 2^27 (bit offsets stay below 2^31; the host form takes such images); CTPN_ERR_STATE on a
 * post-processing-only ctx; CTPN_ERR_ARG with the path in ctpn_last_error() for a file that cannot be written. */
size_t ctpn_png_encode_capacity(int h, int w);
int    ctpn_png_encode(const uint8_t* bgr, int h, int w, uint8_t* out, size_t capacity, size_t* bytes_out);
int    ctpn_encode_png_batch(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w, uint8_t* const* out,
                             const size_t* capacities, size_t* bytes_out);
int    ctpn_write_annotated_png_files(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs,
                                      int line_capacity, const int* line_counts, double scale, const char* const* paths);
int    ctpn_png_encode_device_stats(ctpn_ctx* ctx, long long* out4);

/* ---- PNG files of MIXED sizes: a table of images over one source, ragged canvases and line crops. Additive to ABI 10. The writer above,
 * given what the JPEG side has (ctpn_encode_jpeg_mixed, "Ragged batches out", ctpn_write_line_crops): image i is heights[i] x widths[i], its
 * first pixel at source + offsets[i], its rows pitches[i] >= 3 widths[i] bytes apart. One set of kernels: the uniform calls above are
 * tables of equal sizes at pitch 3 w. Every buffer of a call is laid out by prefix sums over its images (the call costs their sum, not n
 * times the largest), and the histogram, length and write kernels run over a one-dimensional grid of work items, one workgroup = 256
 * pieces of ONE image. The source is read BYTE-WISE: no byte outside an image's h x w x 3 pixels is touched, at any pitch or alignment
 * (a weaker demand than the JPEG writer's aligned-dword read). File i is, byte for byte, ctpn_png_encode's file of image i.
 *   ctpn_encode_png_mixed                  the contract of ctpn_encode_jpeg_mixed without `quality`: a host source is copied in the copy
 *                                          queue and every image must lie inside source_bytes; a device source waits for a live decoder
 *                                          batch. out[i] == NULL with capacity 0 sizes the file (CTPN_ERR_CAPACITY with bytes_out[i] set);
 *                                          ctpn_png_encode_capacity(heights[i], widths[i]) always fits
 *   ctpn_write_annotated_png_files_ragged  ctpn_write_annotated_files_ragged without `quality`, through the same pixel stage (canvas copy,
 *                                          outlines per slot, every image resized by its own 1 / scales[i]). Image i's file is what
 *                                          ctpn_write_annotated_png_files writes for that image alone (n = 1, rows [0, heights[i]), its
 *                                          lines, its scale). Takes a host canvas too (canvas_on_device = 0: PNG files are decoded on the host)
 *   ctpn_write_line_crops_png              ctpn_write_line_crops / ctpn_write_line_crops_ragged without `quality`: cut by the same kernel
 *   ctpn_write_line_crops_png_ragged       into the ctx's buffer, crop k coded where it lies as a crop_h x widths[k] image at pitch
 *                                          3 max_w -- the pad columns never enter a file --, lossless: file k decodes to ctpn_crop_lines'
 *                                          crop k. Sizing form (paths == NULL), "no lines is CTPN_OK", *total_out always written and the
 *                                          geometry limits as there
 * CTPN_ERR_ARG, naming the image and before any device work: n <= 0 or a null pointer, a size outside 1 .. 65535, a pitch below 3 w, an
 * image outside a host source, h (1 + 3 w) > 2^27, more than 2^31 - 1 work items or 2^32 pieces in one call. CTPN_ERR_STATE on a
 * post-processing-only ctx. ctpn_png_encode_device_stats keeps its meaning. */
int    ctpn_encode_png_mixed(ctpn_ctx* ctx, const uint8_t* source, int source_on_device, size_t source_bytes, int n, const int* heights,
                             const int* widths, const size_t* pitches, const size_t* offsets, uint8_t* const* out, const size_t* capacities,
                             size_t* bytes_out);
int    ctpn_write_annotated_png_files_ragged(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights,
                                             const double* recs, int line_capacity, const int* line_counts, const double* scales,
                                             const char* const* paths);
int    ctpn_write_line_crops_png(ctpn_ctx* ctx, const uint8_t* images, int images_on_device, int n, int h, int w, const double* recs,
                                 int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value, const char* const* paths,
                                 int* widths_out, int* total_out);
int    ctpn_write_line_crops_png_ragged(ctpn_ctx* ctx, const uint8_t* canvas, int canvas_on_device, int n, int hc, int w, const int* heights,
                                        const double* recs, int line_capacity, const int* line_counts, int crop_h, int max_w, int pad_value,
                                        const char* const* paths, int* widths_out, int* total_out);

/* ---- anchor targets and the RPN loss: the label side of ctpn/train_net.py on the device. Additive to ABI 10, no option, no parameter name, no
 * ctx: like ctpn_page_cut the calls take a device_id, run on a stream of their own and synchronise once, at their end. That stream is
 * non-blocking and waits for no other: with on_device = 1 the work that produces the input arrays must be COMPLETE before the call (synchronise
 * the producing stream first); the outputs are complete when the call returns. Like ctpn_page_cut the calls leave device_id the calling
 * thread's current device. Every call allocates its device blocks and releases them before it returns, and releasing a block waits for the
 * whole device: the results of a ctx's work in flight are not touched, but that work is held up for the moment. What is rebuilt:
 * lib/utils/bbox.pyx (bbox_overlaps, bbox_intersections), lib/rpn_msr/anchor_target_layer_tf.py:10-276 and Network.build_loss with
 * smooth_l1_dist (lib/networks/network.py:367-404) up to model_loss, plus the gradient of model_loss at the heads, where a backward pass would
 * start. Not rebuilt: the backward pass through the network, the optimiser, the data layers, and total_loss's weight-decay term (it depends on
 * the weights alone). Kernels: csrc/targets.hip; their per-thread text, pinned on the CPU: csrc/targets_dev.h.
 *
 *   ctpn_target_config_default  cfg12 = the CTPN_TARGET_CFG_DOUBLES settings of ctpn/text.yml over lib/fast_rcnn/config.py (TRAIN.*):
 *       [0] RPN_NEGATIVE_OVERLAP 0.3   [1] RPN_POSITIVE_OVERLAP 0.7   [2] RPN_CLOBBER_POSITIVES 0   [3] RPN_FG_FRACTION 0.5
 *       [4] RPN_BATCHSIZE 300 (0: no subsampling, the deterministic form for scoring)   [5] DONTCARE_AREA_INTERSECTION_HI 0.5
 *       [6] PRECLUDE_HARD_SAMPLES 1   [7..10] RPN_BBOX_INSIDE_WEIGHTS 0, 1, 0, 1
 *       [11] RPN_POSITIVE_WEIGHT -1: only negative values are built (the uniform weighting of anchor_target_layer_tf.py:211-217: outside
 *            weight 1 on fg, 0 elsewhere); a value >= 0 is CTPN_ERR_UNSUPPORTED.
 *
 *   ctpn_bbox_overlaps  the lib/utils/bbox.pyx seam. boxes n x 4, query k x 4, out n x k, float64 host arrays. intersections = 0: bbox_overlaps
 *       (bbox.pyx:15-55), out[i][j] = iw ih / (area(box i) + area(query j) - iw ih); intersections = 1: bbox_intersections (:57-93),
 *       iw ih / area(query j). Bit-equal to the reference's arithmetic: widths and heights with + 1, the iw > 0 and ih > 0 gates (0 otherwise),
 *       one IEEE double division, no FMA contraction. n = 0 or k = 0 returns CTPN_OK and writes nothing.
 *
 *   ctpn_anchor_targets  anchor_target_layer for n images that share one feature map hf x wf. im_info n x 3 (height, width, scale); ground truth
 *       ragged: gt_boxes total x 5 (x1, y1, x2, y2, class) with gt_offsets (n + 1 ints from 0, never falling), gt_hard (total ints, nullable),
 *       dontcare totalD x 4 with dc_offsets (both nullable); cfg12 (NULL: the defaults); seed for the subsampling. Outputs in the reference's
 *       layouts: labels (n, hf, wf, 10); bbox_targets, inside_weights, outside_weights (n, hf, wf, 40); stats n x 6 = {inside anchors, fg before
 *       sampling, bg before, fg after, bg after, anchors disabled by dontcare / hard}. Nullable stage outputs: labels_presample (like labels),
 *       max_overlap (a double per anchor, 0 outside the image), argmax (an int per anchor, -1 outside). on_device = 1: every tensor-sized array,
 *       in and out (gt_boxes, gt_hard, dontcare, the four outputs, the three stage outputs) is a device pointer on device_id, the
 *       (n, hf, wf, 40) ones 16-byte aligned; im_info, the offsets, cfg12 and stats are always the host's.
 *       The reference's semantics in its order of operations, quirks included:
 *         - anchors: generate_anchors' ten (the proposal layer's table) on the 16-px grid; inside the image means x1 >= 0, y1 >= 0,
 *           x2 < im_info width, y2 < im_info height (_allowed_border = 0). Everything below concerns inside anchors only;
 *         - ground truth is cast float -> double before any arithmetic; overlaps are ctpn_bbox_overlaps' expression;
 *         - argmax is numpy's: the first maximum wins;
 *         - "gt_argmax_overlaps" is EVERY anchor whose overlap equals its column's maximum (np.where(overlaps == gt_max_overlaps), :136): a
 *           ground-truth box that overlaps no inside anchor has maximum 0 and makes every anchor with overlap 0 to it foreground;
 *         - label order: bg (max overlap < NEGATIVE), column-maximum fg, threshold fg (>= POSITIVE); with CLOBBER the bg rule last. Then
 *           dontcare: -1 where the sum over the areas, in index order, of the covered fraction of the anchor exceeds INTERSECTION_HI. Then hard
 *           boxes (gt_hard == 1, with PRECLUDE_HARD_SAMPLES): -1 where the maximum over the hard boxes is >= POSITIVE, and every hard box
 *           disables its FIRST maximal anchor even at overlap 0;
 *         - subsampling (RPN_BATCHSIZE > 0) is this library's own rule, numpy's Mersenne-Twister permutation is not reproduced:
 *             key(image, anchor) = z ^ (z >> 31), z = (z ^ (z >> 27)) * 0x94D049BB133111EB, z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9,
 *             z = seed ^ ((uint64)image << 32 | anchor)      (splitmix64's finaliser; image is the index in the call, anchor (y wf + x) 10 + a)
 *           if fg exceeds int(FG_FRACTION * BATCHSIZE), the fg anchors with the smallest (key, anchor) pairs stay and the rest become -1; then
 *           the same for bg with BATCHSIZE - fg_after. The finaliser is a bijection, so one image's keys never tie. npr.choice picks another
 *           set of the same size;
 *         - bbox_targets = bbox_transform(anchor, gt[argmax]) rounded to float, for EVERY inside anchor, in the reference's mixed precision:
 *           the anchor's side and the differences, quotients and logs are double, but gt's width, height and centre are float32 arithmetic,
 *           because bbox_transform gets the layer's float32 gt_boxes (only bbox_overlaps is given a float64 copy);
 *         - inside weights: cfg12[7..10] on fg, 0 elsewhere; outside weights: 1 on fg, 0 elsewhere (:207-226);
 *         - outside anchors: label -1, targets and weights 0;
 *         - extension: with no ground-truth box the reference crashes on an empty argmax. Here an image with G = 0 gets label 0 on every inside
 *           anchor (dontcare and sampling apply), zero targets, max_overlap 0 and argmax -1.
 *
 *   ctpn_rpn_loss  build_loss without the regulariser. heads: n x hf x wf rows of ld floats, ld 60 or 64 -- ctpn_get_tensor("heads") or the
 *       heads GEMM's rows: [0, 40) ten (dx, dy, dw, dh), [40, 60) ten (bg, fg) logit pairs, [60, ld) never read. The four target arrays as
 *       ctpn_anchor_targets writes them; on_device as there (heads, the four, d_heads). losses n x 3 doubles = {rpn_cross_entropy, rpn_loss_box,
 *       model_loss}, counts n x 2 ints = {kept anchors (label != -1), fg anchors}, both the host's. d_heads (nullable): d model_loss / d heads
 *       as float in the shape of heads, columns [60, ld) written as 0. Double arithmetic from the float inputs: ce = logsumexp(pair) -
 *       pair[label] in the max-shifted form (stable for logits of +-1e4), its mean over the kept anchors; the box loss = the sum over kept
 *       anchors of outside * smooth_l1(inside * (pred - target)) / (fg + 1), smooth_l1 with sigma2 = 9 and the strict < of network.py:370
 *       (|x| = 1/9 takes the linear branch). An image with no kept anchor gets cross entropy 0.0 and counts[0] = 0 (TensorFlow's mean of
 *       nothing is NaN). Sums run in a fixed order that depends on hf x wf alone: image i of a batch gives the bytes of image i alone.
 *
 * CTPN_ERR_ARG, before any device work: a null pointer, offsets that do not start at 0 or fall, hf x wf x 10 > 2^24 or n x hf x wf x 40 > 2^32,
 * n > 65535, a cfg12 value that is not finite, a threshold or fraction outside [0, 1], a batch size that is negative or not whole, ld other
 * than 60 / 64. CTPN_ERR_NODEVICE without a device: there is no CPU fallback. */
#define CTPN_TARGET_CFG_DOUBLES 12
int    ctpn_target_config_default(double* cfg12);
int    ctpn_bbox_overlaps(int device_id, const double* boxes, int n, const double* query, int k, double* out, int intersections);
int    ctpn_anchor_targets(int device_id, int n, int hf, int wf, const float* im_info, const float* gt_boxes, const int* gt_offsets, const int* gt_hard,
                           const float* dontcare, const int* dc_offsets, const double* cfg12, unsigned long long seed, int on_device, float* labels,
                           float* bbox_targets, float* inside_weights, float* outside_weights, int* stats, float* labels_presample,
                           double* max_overlap, int* argmax);
int    ctpn_rpn_loss(int device_id, int n, int hf, int wf, const float* heads, int ld, const float* labels, const float* bbox_targets,
                     const float* inside_weights, const float* outside_weights, int on_device, double* losses, int* counts, float* d_heads);

/* ---- the recurrent tail: forward with saved activations, backward ----
 * What ctpn_rpn_loss's d_heads is for: the gradient of model_loss at the weights people fine-tune, everything behind rpn_conv/3x3 -- the BiLSTM,
 * the lstm_o FC and the two heads, the LAST TEN manifest entries, CTPN_TAIL_FLOATS contiguous floats at the arena's end (arena[17 074 496:]).
 * Two stateless calls with ctpn_anchor_targets' conventions (no ctx, own non-blocking stream, one synchronisation at the end, device blocks
 * allocated and released by the call, the caller's current device put back, on_device = 1: every tensor-sized array is a device pointer, no CPU
 * fallback). All arithmetic is fp32, matrix products on the exact-fp32 MFMA. No floating-point atomics: two calls on the same inputs give the
 * same bytes. d_x is where the backward of rpn_conv/3x3 and the 13 VGG convs starts ("the conv stack: backward", below). The optimisers:
 * "the solver step"; ctpn/finetune_tail.py is the Momentum branch of lib/fast_rcnn/train.py on the host. Not built: the data layers.
 *
 *   x     rpn_conv/3x3's output, a plain n x hf x wf x 512 array: what ctpn_get_tensor("rpn_conv/3x3") returns.
 *   tail  the ten tensors in manifest order and TF's layout: fw kernel [640][512] (rows 0..511 the input part, 512..639 the recurrent part;
 *         gate columns i | j | f | o), fw bias [512], bw kernel, bw bias, lstm_o/weights [256][512], lstm_o/biases [512], rpn_bbox_pred/weights
 *         [512][40], /biases [40], rpn_cls_score/weights [512][20], /biases [20]. Packing, the gate-column permutation and the transposes happen
 *         inside the call.
 *   saved caller-owned plain memory, ctpn_tail_saved_floats(n, hf, wf) = 2048 floats per cell, M = n hf wf cells in (image, row, column) order:
 *             [0, 256 M)         lstm_out  [M][256]      fw 128 | bw 128
 *             [256 M, 768 M)     lstm_o    [M][512]
 *             [768 M, 2048 M)    gates     [M][2 directions][5][128]: the activated i, j (tanh), f (= sigmoid(z_f + 1.0)), o, and the cell state c
 *
 *   ctpn_tail_forward   heads: n hf wf rows of 64 floats, columns 0..39 rpn_bbox_pred, 40..59 rpn_cls_score, 60..63 zero. saved: nullable. The
 *       projection, the FC and the heads are the fp32 forward's own GEMM launches, the recurrence is its exact-gate kernel in a form that also
 *       stores the gates: heads and the saved lstm_out are the bytes of a CTPN_PREC_FP32 ctx's "heads" and "lstm_out" for that ctx's own
 *       "rpn_conv/3x3".
 *   ctpn_tail_backward  d_heads: rows of 64 floats, columns 60..63 ignored (they may hold anything). d_tail: CTPN_TAIL_FLOATS floats in tail's
 *       layout, every one written. d_x (nullable): n x hf x wf x 512. BPTT of the TF-1.3 LSTMCell from the saved activations (forget bias 1.0,
 *       zero initial state, bw runs right to left). The reduction over cells in every weight and bias gradient runs in a FIXED ORDER THAT DEPENDS
 *       ON n hf wf ALONE: the cells are cut into consecutive blocks of B = 256 cells, B doubled until at most 32 blocks cover them; inside a
 *       block an element is an fma chain over the cells in ascending order (a bias: eight interleaved running sums, added pairwise), and the blocks' partial sums are added left to
 *       right. So a call on M <= 256 cells returns one block's sum, and the gradient of M = 256 k cells whose blocks end at sequence ends is
 *       exactly ((g_1 + g_2) + ...) + g_k of the calls on the blocks alone.
 *
 * CTPN_ERR_ARG, before any device work: a null pointer (saved of the forward and d_x excepted), n, hf or wf < 1, n x hf x wf > 2^21 cells,
 * on_device other than 0 / 1, a device pointer that is not 16-byte aligned. ctpn_tail_saved_floats returns -1 for such a shape.
 * CTPN_ERR_NODEVICE without a device.
 *
 * ctpn_debug_tail_bptt (test hook, host arrays): the backward recurrence alone. gates [rows * T][2][5][128] (the saved block's third part),
 *   d_lstm_out [rows * T][256], tail as above (only the two recurrent parts kernel[512:640] are read) -> d_pre [rows * T][1024], the gradient
 *   at the gate pre-activations in TF's column order (fw i | j | f | o, then bw): the stage ctpn_tail_backward keeps to itself. */
#define CTPN_TAIL_FLOATS 818748
long long ctpn_tail_saved_floats(int n, int hf, int wf);
int    ctpn_tail_forward(int device_id, int n, int hf, int wf, const float* x, const float* tail, int on_device, float* heads, float* saved);
int    ctpn_tail_backward(int device_id, int n, int hf, int wf, const float* x, const float* tail, const float* saved, const float* d_heads,
                          int on_device, float* d_tail, float* d_x);
int    ctpn_debug_tail_bptt(int device_id, int rows, int T, const float* d_lstm_out, const float* gates, const float* tail, float* d_pre);

/* ---- the conv stack: backward ----
 * Where ctpn_tail_backward's d_x goes on: the gradient through rpn_conv/3x3 and the 13 VGG convs back to conv1_1, one layer per call, so that
 * all 17 893 244 weights have a gradient (the reference trains all of them: lib/networks/VGGnet_train.py freezes no conv). Stateless calls with
 * the tail's conventions (no ctx, own non-blocking stream, one synchronisation at the end, device blocks allocated and released by the call, the
 * caller's current device put back, on_device = 1: every tensor-sized array is a device pointer, 16-byte aligned; no CPU fallback). All
 * arithmetic is fp32, products on the exact-fp32 MFMA, no floating-point atomics: two calls on the same inputs give the same bytes.
 * ctpn_amd.network_gradients (Python) walks these calls over a ctx's stored activations fetched to the host; network_gradients_device walks
 * them over the tensors of ctpn_hip_train.h's device-resident form of ctpn_get_tensor, and "the solver step" (below) is the optimiser. Not built: the data layers.
 *
 * Tensors are plain and dense: activations NHWC, w_hwio TF's [3][3][ci][co], padding SAME (zeros outside the image; a tap never crosses from
 * one image of the batch into the next). ci is 3 (conv1_1; d_x must then be NULL) or a multiple of 32, co a multiple of 64, both <= 2048.
 *
 *   ctpn_conv3x3_backward   the layer y = relu(conv(x, w) + b). x: n h w ci, the layer's input; y: n h w co, its stored post-ReLU output;
 *       d_y: the gradient at y. With dZ = d_y where y > 0 and 0 elsewhere:
 *         d_x[n,i,j,c]    = sum over ky, kx, o of dZ[n, i-ky+1, j-kx+1, o] w[ky][kx][c][o]     (nullable) one fma chain per element
 *         d_w[ky][kx][c][o] = sum over pixels of x[n, i+ky-1, j+kx-1, c] dZ[n,i,j,o]
 *         d_b[o]          = sum over pixels of dZ[n,i,j,o]
 *       The sums over pixels run in a FIXED ORDER THAT DEPENDS ON (n, h, w, ci, co) ALONE, never on the device: the n h w pixels are cut, in
 *       (image, row, column) order, into `blocks` consecutive blocks of `block_pixels` (the last one may be short); inside a block an element
 *       of d_w is an fma chain over the pixels in ascending order (of d_b: eight interleaved running sums, added pairwise, as in the tail), and
 *       the blocks' partial sums are added left to right.
 *   ctpn_conv3x3_backward_plan   that plan, pure host arithmetic, no device: with tiles = ceil(ci / 16) (co / 64), the blocks wanted are
 *       ceil(1024 / tiles) held to 1 .. 32; block_pixels = ceil(n h w / wanted) rounded up to a multiple of 64; blocks = ceil(n h w /
 *       block_pixels) <= 32. (conv1_2 at 600 x 900: 32 blocks of 16 896 pixels; conv5_x: 4 blocks of 576.) Scratch is blocks copies of d_w.
 *   ctpn_maxpool2x2_backward   the 2x2 / stride 2 VALID max-pool. y_full: n h w c, the pool's input; d_pool: n (h/2) (w/2) c; d_full: n h w c,
 *       EVERY element written: d_pool at the FIRST maximum of each window in (row, column) scan order (torch's rule; exact ties are real in
 *       ReLU data), zero elsewhere, zero in the last row / column of an odd-sized map. c is a multiple of 4. With h or w = 1 the pooled map
 *       is empty: d_full is all zeros, d_pool is not read and may be NULL.
 *
 * CTPN_ERR_ARG, before any device work: a null pointer (d_x, and d_pool of an empty pooled map, excepted), a size < 1, other channel counts, a
 * non-NULL d_x with ci = 3, on_device other than 0 / 1, a device pointer that is not 16-byte aligned, n h w beyond 2^28 pixels.
 * CTPN_ERR_NODEVICE without a device. */
int    ctpn_conv3x3_backward(int device_id, int n, int h, int w, int ci, int co, const float* x, const float* w_hwio, const float* y,
                             const float* d_y, int on_device, float* d_w, float* d_b, float* d_x);
int    ctpn_maxpool2x2_backward(int device_id, int n, int h, int w, int c, const float* y_full, const float* d_pool, int on_device, float* d_full);
int    ctpn_conv3x3_backward_plan(int n, int h, int w, int ci, int co, long long* block_pixels, int* blocks);

/* ---- the solver step ----
 * What the gradient is for: one step of lib/fast_rcnn/train.py's optimiser over a flat fp32 vector -- the arena, or the part of it that is
 * trained -- with the gradient of total_loss = model_loss + the L2 terms formed on the way: tf.clip_by_global_norm(grads, clip), then
 * tf.train.MomentumOptimizer, AdamOptimizer (ApplyAdam) or RMSPropOptimizer (ApplyRMSProp). Stateless calls with the gradient units'
 * conventions (no ctx, own non-blocking stream, device blocks allocated and released by the call, the caller's current device put back, no CPU
 * fallback). on_device = 1: w, g, s1, s2 are device pointers, at ANY 4-byte alignment (16-byte aligned vectors are read and written 16 bytes
 * at a time; others 4 bytes at a time by the same threads in the same order); seg_end, seg_decay, hyper8 and out2 are always host arrays.
 *
 *   ctpn_solver_plan      pure host arithmetic: the vector is cut into `blocks` consecutive blocks of `block_floats` (the last may be short),
 *       block_floats = ceil(count / 2048) rounded up to a multiple of 1024, blocks <= 2048. THE ORDER OF BOTH SUMS DEPENDS ON count ALONE:
 *       inside a block, lane l of 256 adds the terms of elements 4 q .. 4 q + 3 for q = l, l + 256, ... in ascending order to one running
 *       double; the 256 lane sums are added pairwise (v[i] += v[i + stride], stride 128, 64, .. 1); the blocks' sums are added left to right on
 *       the host. No atomics: two calls on the same inputs give the same bytes.
 *   ctpn_solver_defaults  hyper8 of a solver: [0] lr  [1] momentum | beta1 | decay  [2] - | beta2 | RMS momentum  [3] - | epsilon | epsilon
 *       [4] clip norm  [5] the value s1 starts at  [6] the value s2 starts at  [7] zero. Momentum: 0.001, 0.9. Adam: 0.001, 0.9, 0.999, 1e-8.
 *       RMS: 0.001, 0.9, 0.0, 1e-10, and [5] = 1.0: TF's `rms` slot starts at ONES. Clip norm 10.0 for all three.
 *   ctpn_solver_step      updates w, s1, s2 (s1: the momentum accumulator | Adam's m | RMS's ms; s2: unused and nullable | v | mom) in place.
 *       seg_end[n_seg] ascending, the last equal to count; element e belongs to the first segment with e < seg_end; seg_decay[n_seg] is the
 *       segment's weight decay d. t is the 1-based step (Adam's bias correction). Per element, fp32, every operation rounded on its own:
 *         ge = g + d w                       (d = 0: ge = g, the product is not formed)
 *         out2[0] = sum ge^2,  out2[1] = sum d w^2 / 2      in double, in the plan's order, of the weights BEFORE the update
 *         norm = sqrt(out2[0]) in double;  gc = ge (float)(clip / norm) if norm > clip, else ge
 *         Momentum   s1 = mu s1 + gc;  w = w - lr s1
 *         Adam       lr_t = (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t)) in double on the host;
 *                    s1 += (gc - s1)(1.0f - beta1);  s2 += (gc gc - s2)(1.0f - beta2);  w -= (s1 lr_t) / (sqrtf(s2) + eps)
 *         RMS        s1 += (gc gc - s1)(1.0f - decay);  s2 = s2 momentum + (gc lr) / sqrtf(s1 + eps);  w -= s2
 *       A non-finite out2[0] is CTPN_ERR_ARG with out2 filled and w, s1, s2 untouched.
 *
 * CTPN_ERR_ARG, before any device work: an unknown solver, count outside 1 .. 2^40, a null pointer (s2 of Momentum excepted), n_seg outside
 * 1 .. 64, segments not ascending or not ending at count, a non-finite decay or hyper value, a clip norm <= 0, t < 1, on_device other than
 * 0 / 1, a pointer that is not 4-byte aligned. CTPN_ERR_NODEVICE without a device (ctpn_solver_plan and ctpn_solver_defaults need none). */
#define CTPN_SOLVER_MOMENTUM 0
#define CTPN_SOLVER_ADAM     1
#define CTPN_SOLVER_RMS      2
int    ctpn_solver_plan(long long count, long long* block_floats, int* blocks);
int    ctpn_solver_defaults(int solver, double* hyper8);
int    ctpn_solver_step(int device_id, int solver, long long count, float* w, const float* g, float* s1, float* s2, const long long* seg_end,
                        const float* seg_decay, int n_seg, const double* hyper8, long long t, int on_device, double* out2);

#ifdef __cplusplus
}
#endif
#endif /* CTPN_HIP_H */
