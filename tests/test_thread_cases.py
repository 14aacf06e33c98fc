"""CPU: the cases and the harness of the thread tests (tests/thread_cases.py) before they reach a GPU -- the schedule covers what it claims, the
harness reports a wrong byte, a raising worker and a missing worker as what they are (pure-Python fake ops, no library), the shapes reach the
shared paths they are there for (through the device-free plan function tests/test_conv_forms.py uses), and every scenario's inputs build
without a device and fit the ctx."""
import itertools
import os
import threading

import numpy as np
import pytest

import conv_forms as F
import ctx_walks as W
import thread_cases as T


# ---- the schedule ----
@pytest.mark.parametrize("threads", [4, 5, 6])
def test_schedule_is_uniform_first_then_covers_every_pair_twice(threads):
    rounds = T.schedule(T.OPS6, threads)
    assert len(rounds) == 1 + 2 * len(T.OPS6) and all(len(r) == threads for r in rounds)
    assert set(rounds[0]) == {"uE"}                                                   # round 0: one op on every thread
    for half in (rounds[1:7], rounds[7:]):                                             # each pass of the square on its own
        together = {frozenset(p) for r in half for p in itertools.combinations(r, 2)}
        assert {frozenset(p) for p in itertools.combinations(T.OPS6, 2)} <= together
        assert all(len(set(r)) == threads for r in half)                               # no op twice in a round
    for t in range(threads):
        mine = [r[t] for r in rounds]
        assert all(mine.count(op) >= 2 for op in T.OPS6)


def test_schedule_refuses_a_thread_count_that_leaves_pairs_out():
    with pytest.raises(ValueError):
        T.schedule(T.OPS6, 3)
    with pytest.raises(ValueError):
        T.schedule(T.OPS6, 7)


def test_the_walks_of_ctx_walks_are_untouched():
    assert "uE" not in W.OP and "uE" in T.OP and set(T.OP) == set(W.OP) | {"uE"}
    assert len(W.OPS) == 17 and len(W.pair_walk(len(W.OPS))) == 290


# ---- the harness, on fake ops ----
class Fake:
    """run(op) -> (bytes of the op's name repeated, a count); bad: {(round, thread)} where one byte is flipped; raises / stuck: (round, thread)"""

    def __init__(self, t, bad=(), raises=None, stuck=None, release=None):
        self.t, self.bad, self.raises, self.stuck, self.release, self.round = t, bad, raises, stuck, release, -1
        self.started = self.stopped = False

    def start(self):
        self.started = True

    def stop(self):
        self.stopped = True

    def run(self, op):
        self.round += 1
        if self.raises == (self.round, self.t):
            raise RuntimeError("device lost")
        if self.stuck == (self.round, self.t):
            self.release.wait()          # never reaches the next barrier while the test runs
        x = fake_alone(op)[0].copy()
        if (self.round, self.t) in self.bad:
            x[5] ^= 1
        return (x, len(op))


def fake_alone(op):
    return (np.frombuffer((op * 8).encode(), np.uint8), len(op))


ROUNDS = T.schedule(T.OPS6, 4)


def test_a_clean_run_is_clean():
    workers = [Fake(t) for t in range(4)]
    results = T.run_together(workers, ROUNDS, timeout=5.0)
    assert len(results) == 4 * len(ROUNDS) and T.mismatches(results, ROUNDS, lambda t, op: fake_alone(op)) == []
    assert all(w.started and w.stopped for w in workers)
    back, extra = T.unpack(_through_a_file(T.pack(results, {"seconds": 1.5})))
    assert T.mismatches(back, ROUNDS, lambda t, op: fake_alone(op)) == [] and float(extra["seconds"]) == 1.5


def _through_a_file(arrays):
    import io
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    buf.seek(0)
    return np.load(buf)


def test_one_wrong_byte_in_one_round_and_thread_is_named():
    results = T.run_together([Fake(t, bad={(5, 2)}) for t in range(4)], ROUNDS, timeout=5.0)
    bad = T.mismatches(results, ROUNDS, lambda t, op: fake_alone(op))
    assert len(bad) == 1 and bad[0].startswith("round 5 thread 2: %s differs from the alone result in element 0" % ROUNDS[5][2]), bad
    results.pop((3, 1))
    assert "round 3 thread 1: %s has no result" % ROUNDS[3][1] in T.mismatches(results, ROUNDS, lambda t, op: fake_alone(op))


def test_results_of_other_kinds_are_compared_and_survive_the_file():
    res = {(0, 0): (np.arange(3, dtype=np.int32), 7, "ctpn_nms: boxes must be N x (>=4)"), (0, 1): (np.zeros((0, 5), np.float32), -4, "")}
    back, _ = T.unpack(_through_a_file(T.pack(res)))
    assert all(W.same(back[k], res[k]) is None for k in res)
    assert W.same(back[(0, 0)], res[(0, 0)][:2] + ("another text",)) == 2
    assert W.same(back[(0, 1)], (np.zeros((0, 5), np.float32), -1, "")) == 1


def test_a_raising_worker_is_reported_with_its_round_and_op():
    workers = [Fake(t, raises=(4, 3)) for t in range(4)]
    with pytest.raises(T.WorkerError) as e:
        T.run_together(workers, ROUNDS, timeout=5.0)
    assert (e.value.round, e.value.thread, e.value.op) == (4, 3, ROUNDS[4][3]) and "device lost" in str(e.value)
    assert isinstance(e.value.__cause__, RuntimeError)
    assert all(w.stopped for w in workers)                                             # the others were released and stopped


def test_a_worker_that_never_reaches_the_barrier_is_a_broken_barrier():
    release = threading.Event()
    try:
        with pytest.raises(T.BarrierBroken) as e:
            T.run_together([Fake(t, stuck=(2, 1), release=release) for t in range(4)], ROUNDS, timeout=0.2)
        assert e.value.round == 3 and e.value.missing == [1] and "broken barrier" in str(e.value)
    finally:
        release.set()


# ---- the shapes reach the shared paths ----
def cells(prec, op):
    return F.walk_cells(prec, *T.SHAPES[op], False)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_uE_forks_a_16_bit_edge_strip_beside_a_wr_launch(prec):
    n, h, w = T.E
    assert n == 3 and (w // 2) % 16 == 1 and w // 2 + 2 > 114
    p = F.B.conv3x3_plan(prec, n, h // 2, w // 2, 64, 128, False, cu_count=F.CU)      # conv2_1
    assert (p.main, p.strip, p.deep) == ("wr", "edge", 0) and p.cols == 1
    assert "/wr/" in cells(prec, "uE")["conv2_1"] and "/edge1/fork/" in cells(prec, "uE")["conv2_1"]


def test_fp32_ops_fork_im2col_strips():
    for op in ("uA", "uB"):
        assert any("/im2col" in c and "/fork/" in c for c in cells("fp32", op).values()), op


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_conv1_2_of_every_16_bit_op_is_weights_in_registers(prec):
    for op in T.SHAPES:
        assert cells(prec, op)["conv1_2"].split("/")[1] == "wr", op


def test_nms_sizes_cross_the_caches_initial_capacity():
    assert T.NMS_SIZES == (63, 20000, 64) and T.NMS_SIZES[0] < T.NMS_CACHE_INITIAL < T.NMS_SIZES[1] > T.NMS_SIZES[2]
    src = open(os.path.join(os.path.dirname(os.path.abspath(F.B.__file__)), "csrc", "api_proposals.hip")).read()
    assert "boxes_num < %d ? %d : boxes_num" % (T.NMS_CACHE_INITIAL, T.NMS_CACHE_INITIAL) in src


# ---- the scenarios ----
def test_the_scenarios_are_the_eight():
    assert list(T.SCENARIOS) == ["same[%s]" % p for p in W.PRECS] + ["mixed", "stateless", "codecs", "lifecycle"]
    assert [len(T.SCENARIOS[n].workers) for n in T.SCENARIOS] == [4, 4, 4, 4, 5, 4, 4, 3]
    for name, sc in T.SCENARIOS.items():
        assert all(len(row) == len(sc.workers) for row in sc.rounds), name
        ctxs = sum(s.kind in ("ctx", "errors") for s in sc.workers) + sum(len(col) for s, col in zip(sc.workers, zip(*sc.rounds)) if s.kind == "churn")
        calls = sum(op is not None for row in sc.rounds for op in row)
        assert ctxs <= 14 and calls <= 100, (name, ctxs, calls)
    mixed = T.SCENARIOS["mixed"]
    assert [s.prec for s in mixed.workers[:4]] == list(W.PRECS) and mixed.workers[4] == T.WorkerSpec("errors", "bf16")
    assert {row[4] for row in mixed.rounds} == set(T.ERROR_OPS) and [row[:4] for row in mixed.rounds] == T.schedule(T.OPS6, 4)
    life = T.SCENARIOS["lifecycle"]
    assert [(s.kind, s.prec) for s in life.workers] == [("ctx", "fp16"), ("churn", "bf16"), ("churn", "split")]
    assert [row[1:] for row in life.rounds] == [("uC", "uC")] * 6 and {row[0] for row in life.rounds} == {"uC", "uE"}
    state = T.SCENARIOS["stateless"]
    third = [row[3] for row in state.rounds]
    assert third[:5] == ["nms63", "nms20000", "nms64", "page1000x2", "page20000x1024"] and third[5:] == third[:5]
    assert {row[0] for row in state.rounds} == {"pAB", "pRC"}


def test_every_op_of_every_scenario_exists_and_its_inputs_build_without_a_device(tmp_path):
    names = {op for sc in T.SCENARIOS.values() for row in sc.rounds for op in row if op is not None}
    known = set(T.OP) | set(T.ERROR_OPS) | set(T.FREE_OPS) | set(T.CODEC_OPS)
    assert names <= known
    n, h, w = W.CAP
    x = dict(W.inputs(), **T.extra_inputs())
    for name in ("E", "A", "B", "C", "W"):
        assert x[name].dtype == np.uint8 and x[name].shape[0] <= n and x[name].shape[1] <= h and x[name].shape[2] <= w, name
    assert x["E"].shape == T.E + (3,) and W.weights().dtype == np.float32
    free = T.free_inputs()
    assert [len(free["nms%d" % r]) for r in T.NMS_SIZES] == list(T.NMS_SIZES)
    assert [len(free["page%dx%d" % p]) for p in T.PAGE_NMS] == [r for r, _ in T.PAGE_NMS]
    assert (free["page20000x1024"][:, 0] == 16 * 1023).any()                          # the last of the 1024 columns is used
    assert free["scene"]["hf"] * free["scene"]["wf"] == 48 and np.isfinite(free["heads"]).all()
    assert [free["tail%dx%dx%d" % s][0].shape for _, s in T.TAIL_CASES] == [(1, 1, 1, 512), (1, 15, 2, 512)]
    c = T.codec_inputs()
    assert len(c["jpeg"]) == 5 <= n and len(c["huff"]) == 3 and c["png"].shape == (2, 9, 85, 3) and len(c["mixed"]) == 5
    assert all(im.shape[0] <= h and im.shape[1] <= w for im in c["mixed"])
    paths = T.png_files(str(tmp_path / "png"))
    from PIL import Image
    assert all(np.array_equal(np.asarray(Image.open(p))[:, :, ::-1], im) for p, im in zip(paths, c["png"]))
    for name in T.SCENARIOS:
        assert T.alone_keys(name)
