"""GPU property / differential tests (hypothesis): generated CTPN-shaped inputs through the C ABI against the oracle.
  * the NMS seam (ctpn_nms via lib.utils.gpu_nms): keep list identical to oracle/postproc.py::nms, ties included;
  * the proposal layer on host heads (ctpn_proposals_from_host, i.e. decode -> sort -> column NMS): rois against
    oracle/postproc.py::proposal_layer within 1e-3 px (the device's expf vs numpy's exp in the height decode);
  * the same layer on raw heads (ctpn_debug_proposals_from_heads: the softmax inside decode_kernel) against the oracle fed the float64 softmax."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import ctpn_amd
from ctpn_amd.lib.utils.gpu_nms import gpu_nms
from oracle import postproc as P
from util import match_rois

pytestmark = pytest.mark.gpu


@settings(max_examples=40, deadline=None)
@given(st.integers(min_value=0, max_value=2 ** 31 - 1), st.integers(min_value=0, max_value=700), st.sampled_from([0.2, 0.5, 0.7]))
def test_nms_seam_equals_oracle_on_generated_boxes(seed, n, thr):
    rng = np.random.default_rng(seed)
    col = rng.integers(0, 30, n)
    y1 = rng.integers(0, 200, n).astype(np.float32) + rng.choice([0.0, 0.25, 0.5], n).astype(np.float32)
    h = rng.integers(4, 120, n).astype(np.float32)
    free_x = rng.random() < 0.3                                   # some cases off the anchor grid: arbitrary x as the B1 seam allows
    x1 = (rng.uniform(0, 480, n).astype(np.float32) if free_x else (16.0 * col).astype(np.float32))
    w = (rng.uniform(4, 80, n).astype(np.float32) if free_x else np.full(n, 15.0, np.float32))
    score = rng.choice(np.linspace(0.05, 1.0, 16).astype(np.float32), n)       # ties on purpose
    dets = np.stack([x1, y1, x1 + w, y1 + h, score], axis=1).astype(np.float32)
    assert [int(k) for k in gpu_nms(dets, thr)] == [int(k) for k in P.nms(dets, thr)]


@settings(max_examples=25, deadline=None)
@given(st.integers(min_value=0, max_value=2 ** 31 - 1), st.integers(min_value=2, max_value=14), st.integers(min_value=3, max_value=24),
       st.sampled_from([1.0, 1.25, 2.0]))
def test_proposal_layer_equals_oracle_on_generated_heads(seed, hf, wf, scale):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((1, hf, wf, 10, 2)).astype(np.float32) * 2.0
    e = np.exp(logits - logits.max(-1, keepdims=True))
    cls_prob = (e / e.sum(-1, keepdims=True)).reshape(1, hf, wf, 20).astype(np.float32)
    bbox = (rng.standard_normal((1, hf, wf, 40)) * 0.3).astype(np.float32)
    im_info = np.array([[hf * 16, wf * 16, scale]], np.float32)
    want = P.proposal_layer(cls_prob, bbox, im_info)
    with ctpn_amd.Context(0, 1, hf * 16, wf * 16, "bf16", postproc_only=True) as ctx:
        got = ctx.proposals_from_host(cls_prob, bbox, im_info)[0]
    # an IoU within an ulp of the threshold may resolve differently after the device's expf: allow a stray row, not a pattern
    assert abs(len(got) - len(want)) <= 2, (got.shape, want.shape)
    if len(want) and len(got):
        assert match_rois(got, want, px_tol=1e-3, score_tol=1e-6) >= 0.99


@settings(max_examples=25, deadline=None)
@given(st.integers(min_value=0, max_value=2 ** 31 - 1), st.integers(min_value=2, max_value=14), st.integers(min_value=3, max_value=24),
       st.sampled_from([1.0, 1.25, 2.0]))
def test_proposal_layer_on_raw_heads_equals_oracle_fed_the_float64_softmax(seed, hf, wf, scale):
    """the production branch of decode_kernel (ctpn_debug_proposals_from_heads: the softmax inside the kernel, rows of 64 floats) against the
    oracle on the float64 pair softmax of the same logits"""
    rng = np.random.default_rng(seed)
    heads = np.full((1, hf, wf, 64), np.nan, np.float32)
    heads[..., :40] = (rng.standard_normal((1, hf, wf, 40)) * 0.3).astype(np.float32)
    heads[..., 40:60] = (rng.standard_normal((1, hf, wf, 20)) * 2.0).astype(np.float32)
    logits = heads[..., 40:60].reshape(1, hf, wf, 10, 2).astype(np.float64)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    cls_prob = (e / e.sum(-1, keepdims=True)).reshape(1, hf, wf, 20).astype(np.float32)
    im_info = np.array([[hf * 16, wf * 16, scale]], np.float32)
    want = P.proposal_layer(cls_prob, heads[..., :40], im_info)
    with ctpn_amd.Context(0, 1, hf * 16, wf * 16, "bf16", postproc_only=True) as ctx:
        rois, _, got_cls, got_bbox = ctx.proposals_from_heads(heads, im_info)
    assert np.array_equal(got_bbox, heads[..., :40]) and np.abs(got_cls - cls_prob).max() <= 1e-6
    got = rois[0]
    assert abs(len(got) - len(want)) <= 2, (got.shape, want.shape)
    if len(want) and len(got):
        assert match_rois(got, want, px_tol=1e-3, score_tol=1e-6) >= 0.99
