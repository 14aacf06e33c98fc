"""GPU: two submitted batches in flight -- the forward sets of a ctx (csrc/ctx.h, FwdSet: a forward stream and the buffers a forward writes).

A submit that finds the other slot in flight runs on a second set, on a second stream, its conv stack gated behind the other set's
(profiles/ab_two_forwards.txt); a measurement build (make ablation, CTPN_TWO_FORWARDS = 0 .. 3) can keep both slots on set 0, let the
forwards overlap freely or move the gate, and these tests hold in every mode: a batch submitted beside another batch in flight gives the bytes it gives run
alone through a fresh ctx's synchronous detect; each set keeps its own geometry; a ragged batch, a rejected submit, a keep_acts ctx and a
synchronous-only ctx behave as with one set; profile mode 2 reports the union of the forwards' conv intervals.

Shapes (tests/conv_forms.py walk_cells, 256 CUs, production path): A = 3 x 32 x 1040 crosses wr, p_16x16, p_8x32, p_flat64 with forked im2col,
edge2, edge_pool2 and edge_pool4 strips in bf16; B = 3 x 304 x 264 crosses wr, p_8x32, p_flat, p_flat64 with forked im2col, edge_pool2 and
edge_pool4 strips. Three images: with one or two the edge strips take the deep form in the layer's stream anyway."""
import time

import numpy as np
import pytest

import ctpn_amd

pytestmark = pytest.mark.gpu

A = (3, 32, 1040)
B = (3, 304, 264)
MAXS = (3, 304, 1040)


def images(shape, seed):
    return ctpn_amd.weights.synthetic_images(shape[0], shape[1], shape[2], seed)


def same(got, want):
    (gl, gr), (wl, wr) = got, want
    assert len(gl) == len(wl) and len(gr) == len(wr)
    for x, y in zip(gl, wl):
        assert x.shape == y.shape and np.array_equal(x, y)
    for x, y in zip(gr, wr):
        assert x.shape == y.shape and np.array_equal(x, y)


def two_sets(ctx, in_flight=None):
    """the library's own account of its forward sets is consistent: one set, everything on it -- or two, the second with memory behind it and
    (in_flight given: the slots' sets expected with two sets) the two batches in flight on different ones"""
    sets, last, set1_bytes, flying = ctx.forward_sets()
    assert sets in (1, 2) and last < sets and (set1_bytes > 0) == (sets == 2)
    if sets == 1:
        assert all(f in (None, 0) for f in flying)
    elif in_flight is not None:
        assert flying == in_flight
    return sets == 2


_alone = {}


def alone(arena, prec, key, imgs, heights=None, maxs=MAXS, options=None):
    """(lines, rois, heads) of one batch through a fresh ctx's synchronous detect: computed once per (precision, batch), shared, not modified"""
    k = (prec, key)
    if k not in _alone:
        with ctpn_amd.Context(0, maxs[0], maxs[1], maxs[2], prec, options=options or {}) as ctx:
            ctx.load_weights(arena)
            if heights is None:
                lines, rois = ctx.detect(imgs, want_rois=True)
            else:
                lines, rois = ctx.detect_ragged(imgs, heights, want_rois=True)
            _alone[k] = (lines, rois, ctx.get_tensor("heads"))
            assert ctx.forward_sets()[0] == 1
        assert sum(len(r) for r in rois) > 0, "the alone run found no proposal: the comparison would be empty"
    return _alone[k]


@pytest.mark.parametrize("first_slot", [0, 1])
@pytest.mark.parametrize("prec", ["bf16", "split", "fp32"])
def test_pipelined_equals_alone(arena, prec, first_slot):
    """six alternating submit / collect rounds over two different batches in the bench's order (submit k + 1, then collect k); then with the slots swapped"""
    a, b = images(A, 21), images(B, 22)
    want = [alone(arena, prec, "A21", a), alone(arena, prec, "B22", b)]
    batches = [a, b]
    with ctpn_amd.Context(0, *MAXS, prec) as ctx:
        ctx.load_weights(arena)
        got = []
        for k in range(6):
            ctx.detect_submit(images=batches[k & 1], slot=(k & 1) ^ first_slot)
            if k == 1:
                two = two_sets(ctx, (0, 1) if first_slot == 0 else (1, 0))
                assert two or ctpn_amd.lib_path().endswith("_ablation.so")      # the product library: two sets
            if k > 0:
                got.append(ctx.detect_collect(((k - 1) & 1) ^ first_slot, want_rois=True))
        got.append(ctx.detect_collect((5 & 1) ^ first_slot, want_rois=True))
        heads = ctx.get_tensor("heads")                    # of the last submit: batch b, on the second set where there is one
        assert ctx.forward_sets()[1] == (1 if two else 0)
    for k in range(6):
        same(got[k], want[k & 1][:2])
    assert np.array_equal(heads, want[1][2])


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_a_geometry_per_slot(arena, prec):
    """2 x 64 x 96 in slot 0 and 1 x 96 x 160 in slot 1, alternating, then the two shapes swap sets: each set zeroes its own borders for its own
    geometry, and a set that changes geometry is re-zeroed"""
    maxs = (2, 96, 160)
    a, b = images((2, 64, 96), 31), images((1, 96, 160), 32)
    wa, wb = alone(arena, prec, "g31", a, maxs=maxs), alone(arena, prec, "g32", b, maxs=maxs)
    with ctpn_amd.Context(0, *maxs, prec) as ctx:
        ctx.load_weights(arena)
        order = [(a, wa), (b, wb), (a, wa), (b, wb), (b, wb), (a, wa), (b, wb), (a, wa)]      # round 4 puts b on the set that held a
        got = []
        for k, (im, _) in enumerate(order):
            ctx.detect_submit(images=im, slot=k & 1)
            if k > 0:
                got.append(ctx.detect_collect((k - 1) & 1, want_rois=True))
        got.append(ctx.detect_collect((len(order) - 1) & 1, want_rois=True))
        two_sets(ctx)
    for g, (_, w) in zip(got, order):
        same(g, w[:2])


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_ragged_beside_uniform(arena, prec):
    """a ragged submit in one slot beside a uniform one in the other, both ways round (the ragged forward stores conv1_1's map, which the second
    set gets only then)"""
    maxs = (3, 96, 160)
    u, canvas = images((3, 96, 160), 41), images((3, 96, 160), 42)
    heights = np.array([96, 48, 70], np.int32)
    wu = alone(arena, prec, "u41", u, maxs=maxs)
    wr = alone(arena, prec, "r42", canvas, heights=heights, maxs=maxs)
    with ctpn_amd.Context(0, *maxs, prec) as ctx:
        ctx.load_weights(arena)
        got = []
        ctx.detect_submit(images=u, slot=0)
        ctx.detect_submit(images=canvas, slot=1, heights=heights)      # ragged on set 1
        got.append((ctx.detect_collect(0, want_rois=True), wu))
        ctx.detect_submit(images=canvas, slot=0, heights=heights)      # ragged on set 0
        got.append((ctx.detect_collect(1, want_rois=True), wr))
        ctx.detect_submit(images=u, slot=1)                            # uniform on set 1, behind a ragged batch there
        got.append((ctx.detect_collect(0, want_rois=True), wr))
        got.append((ctx.detect_collect(1, want_rois=True), wu))
        two_sets(ctx)
    for g, w in got:
        same(g, w[:2])


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_rejected_submit_beside_a_batch_in_flight(arena, prec):
    """a submit refused for its shape while the other slot is in flight: the batch in flight collects with the alone run's bytes, the next submit works"""
    maxs = (3, 96, 160)
    u, v = images((3, 96, 160), 41), images((3, 96, 160), 43)
    wu, wv = alone(arena, prec, "u41", u, maxs=maxs), alone(arena, prec, "v43", v, maxs=maxs)
    too_tall = np.zeros((1, 112, 160, 3), np.uint8)
    with ctpn_amd.Context(0, *maxs, prec) as ctx:
        ctx.load_weights(arena)
        ctx.detect_submit(images=u, slot=0)
        with pytest.raises(ctpn_amd.CtpnError):
            ctx.detect_submit(images=too_tall, slot=1)
        assert ctx.forward_sets()[3] == (0, None)
        ctx.detect_submit(images=v, slot=1)
        same(ctx.detect_collect(0, want_rois=True), wu[:2])
        with pytest.raises(ctpn_amd.CtpnError):
            ctx.detect_submit(images=too_tall, slot=0)                 # ... and with the batch in flight on the second set
        ctx.detect_submit(images=u, slot=0)
        same(ctx.detect_collect(1, want_rois=True), wv[:2])
        same(ctx.detect_collect(0, want_rois=True), wu[:2])


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_second_set_only_where_it_is_used(arena, prec):
    """a ctx used synchronously allocates no second set; a keep_acts ctx used pipelined stays on one set, in the single-stream order, with its bytes"""
    maxs = (3, 96, 160)
    u, v = images((3, 96, 160), 41), images((3, 96, 160), 43)
    with ctpn_amd.Context(0, *maxs, prec) as ctx:
        ctx.load_weights(arena)
        ctx.detect(u)
        ctx.forward(v)
        ctx.detect_submit(images=u, slot=1)
        ctx.detect_collect(1)
        ctx.detect(v)
        assert ctx.forward_sets()[:3] == (1, 0, 0)
    ku = alone(arena, prec, "ku41", u, maxs=maxs, options={"keep_acts": 1})
    kv = alone(arena, prec, "kv43", v, maxs=maxs, options={"keep_acts": 1})
    with ctpn_amd.Context(0, *maxs, prec, options={"keep_acts": 1}) as ctx:
        ctx.load_weights(arena)
        ctx.detect_submit(images=u, slot=0)
        ctx.detect_submit(images=v, slot=1)
        assert ctx.forward_sets() == (1, 0, 0, (0, 0))
        same(ctx.detect_collect(0, want_rois=True), ku[:2])
        ctx.detect_submit(images=u, slot=0)
        same(ctx.detect_collect(1, want_rois=True), kv[:2])
        same(ctx.detect_collect(0, want_rois=True), ku[:2])
        assert np.array_equal(ctx.get_tensor("heads"), ku[2])
        assert ctx.get_tensor("conv1_2").shape == (3, 96, 160, 64)      # the kept maps are still there
        assert ctx.forward_sets()[0] == 1


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_profile_mode_2_counts_overlapping_forwards_once(arena, prec):
    """four pipelined steps in profile mode 2: conv_gemm's time is the union of the forwards' conv intervals, so it cannot exceed the wall-clock
    span of the region; work and launches are four forwards'. Synchronous forwards: one interval each, no overlap, the plain sum."""
    a = images(A, 21)
    with ctpn_amd.Context(0, *MAXS, prec) as ctx:
        ctx.load_weights(arena)
        ctx.profile_enable(2)
        ctx.profile_reset()
        t0 = time.perf_counter()
        ctx.forward(a)
        ctx.sync()
        one = ctx.profile_read()["conv_gemm"]
        wall_one = (time.perf_counter() - t0) * 1e3
        print("one synchronous forward: conv_gemm %.4f ms of %.3f ms wall" % (one["ms"], wall_one))
        assert one["launches"] == 13 and 0 < one["ms"] <= wall_one
        ctx.forward(a)
        ctx.forward(a)
        two = ctx.profile_read()["conv_gemm"]
        assert two["launches"] == 39 and two["work"] == 3 * one["work"] and two["ms"] > one["ms"]
        for k in range(2):                                  # warm both sets (the second is allocated and zeroed here)
            ctx.detect_submit(images=a, slot=k)
        for k in range(2):
            ctx.detect_collect(k)
        ctx.sync()
        ctx.profile_reset()
        t0 = time.perf_counter()
        for k in range(4):
            ctx.detect_submit(images=a, slot=k & 1)
            if k > 0:
                ctx.detect_collect((k - 1) & 1)
        ctx.detect_collect(1)
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        p = ctx.profile_read()["conv_gemm"]
        ctx.profile_enable(False)
        print("four pipelined steps: conv_gemm %.4f ms of %.3f ms wall, %d forward set(s)" % (p["ms"], wall, 2 if two_sets(ctx) else 1))
        assert p["launches"] == 52 and p["work"] == 4 * one["work"]
        assert 0 < p["ms"] <= wall
