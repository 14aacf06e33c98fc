/* libctpn_hip.so, the training-side companion of ctpn_hip.h: what a training step needs beyond inference. ctpn_hip.h is the inference ABI; its
 * stateless training calls (anchor targets, the loss, the two backward passes, the solver step) need no ctx and live there. The one call
 * declared in this file reads a ctx's stored activations. The three stateless calls of the training data layer, which turn a labelled folder
 * into what a step reads, come with this header too: they are declared in ctpn_hip_data_layer.h, which it includes at its end (this file
 * itself keeps to the calls that take a ctx: tests/test_solver.py holds its list and the binding's _declare_train to exactly those).
 * ABI version: ctpn_hip.h's (10). */
#ifndef CTPN_HIP_TRAIN_H
#define CTPN_HIP_TRAIN_H

#include "ctpn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ctpn_get_tensor with the result left in HBM: out_dev is a pointer into the ctx's device's memory, and the stored block is unpacked by a
 * kernel instead of a host loop -- the one-pixel border of conv and pool maps stripped, bf16 / fp16 values widened, hi + lo added in split
 * precision, lstm_pre's gate columns put back in TF's order, the heads' four pad columns dropped. Same names, same shapes, same values bit for
 * bit, same errors (the keep_acts refusals, the rpn_* refusal before ctpn_proposals, CTPN_ERR_CAPACITY with shape4 filled: capacity_floats = 0
 * is the probe). Like ctpn_get_tensor it first drains the forward's streams; the kernel runs on the ctx's stream and the call returns when
 * out_dev is complete. out_dev need only be 4-byte aligned (16-byte aligned output is written 16 bytes at a time).
 * With a batch in flight (ctpn_detect_submit without its collect) it behaves as ctpn_get_tensor does: it reads the most recent forward's
 * blocks after draining that forward's streams, writes out_dev alone and changes neither batch (tests/test_gpu_train.py). */
int ctpn_get_tensor_device(ctpn_ctx* ctx, const char* name, float* out_dev, size_t capacity_floats, int shape4[4]);

#ifdef __cplusplus
}
#endif

#include "ctpn_hip_data_layer.h"

#endif /* CTPN_HIP_TRAIN_H */
