"""GPU: several ctxs on concurrent host threads -- the use include/ctpn_hip.h invites (any number of ctxs per device, each used by one host
thread at a time, distinct ctxs and the stateless calls concurrently), and the first time the per-device shared state runs contended: the
weights-in-registers kernel's dump page, claim slots and ticket (csrc/conv3x3.hip c3_wr_resources), the strip stream and its event pair under
strip_mu, the function-attribute flags and the CU count under launch_state_mutex (csrc/common.h), the pixel LUT (csrc/conv_first.hip), the
ctpn_nms and ctpn_page_nms caches and their re-growth, the PNG decode team, the per-call blocks of ctpn_anchor_targets / ctpn_rpn_loss /
ctpn_tail_forward / ctpn_tail_backward, the thread-local error text, the live-resource counters.

Every scenario of tests/thread_cases.py runs in a fresh child process (tests/thread_child.py, subprocess.run with a 60 s limit -- a hang guard,
not a measurement), so that the process's first forward, first NMS and first decode are the contended ones and a deadlock ends in a killed
child. The reference is the same call made alone, by this process: the op on a new ctx of capacity CAP in that precision that has done
nothing else (alone(), like fresh() of tests/test_gpu_ctx_forgets.py), the stateless and codec calls alone; each computed once, shared,
asserted not to be empty. The alone calls are tied to the oracle, the numpy restatements and Pillow by the suites of their own. Every
comparison is ctx_walks.same, byte for byte: no tolerance appears anywhere.

  same[prec]   4 threads, 4 ctxs of one precision, 13 rounds: uE everywhere, then the cyclic square over uE uA uB uC rW pAB twice
  mixed        one ctx per precision on that schedule; a fifth thread (bf16 ctx) loops over eN, eH and a bad-argument ctpn_nms: its codes and
               texts are the alone ones, the data threads' texts stay empty
  stateless    a bf16 ctx repeats pAB / pRC | anchor_targets, rpn_loss | tail_forward, tail_backward | ctpn_nms at 63, 20 000, 64 boxes (the
               cache grows under the others' work, then is reused) and ctpn_page_nms at 1000 x 2 and 20 000 x 1024 columns
  codecs       ctpn_decode_png_files | JPEG decode, host entropy | JPEG decode and the Huffman decoder on the device | PNG batch encode, mixed JPEG encode
  lifecycle    an fp16 ctx runs uC, uE while two threads each create -> load_weights -> uC -> destroy six times (bf16, split); the live-resource
               counts behind the threads are the counts in front of them. The caches that live for the process are outside that comparison:
               the LUT, the strip stream with its events, the dump page and the claim slots are raw HIP objects the counters never see; g_nms
               and g_page_nms are counted, and no op of this scenario calls ctpn_nms or ctpn_page_nms, so they do not exist in its process.

Stopping rule: a child that is killed at the limit, dies of a signal or ends with a non-zero exit code (a worker raised, a barrier broke) fails
its test with the child's stderr and makes every remaining test of this module skip -- nothing more of this kind is started on a device that
has just hung or faulted. A child that ends cleanly with results that differ fails its test alone. No retries.

Wall time of run_together inside each child on one MI355X (the child's own clock; the whole child, imports and inputs included, is what
pytest --durations shows):

  scenario      run_together   the whole test (child start, imports, inputs, the alone results it is first to ask for)
  same[fp32]    0.50 s         3.5 s
  same[split]   0.39 s         2.8 s
  same[fp16]    0.35 s         2.8 s
  same[bf16]    0.32 s         2.8 s
  mixed         0.44 s         2.8 s  (4.7 s when it is the first to ask for the alone results)
  stateless     0.29 s         3.3 s
  codecs        0.24 s         3.1 s
  lifecycle     0.41 s         2.6 s

None comes near the ten seconds at which a scenario would be split (asserted on the child's own clock)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ctpn_amd
import ctx_walks as W
import thread_cases as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 60          # seconds: a hang guard
SPLIT_ABOVE = 10.0  # seconds: a scenario that takes longer is to be split

_hung = []          # why the rest of the module is skipped
_alone = {}


def alone(prec, op, directory):
    """the op made alone: on a new ctx of capacity CAP in `prec` that has done nothing else (prec None: without a ctx)"""
    key = (prec, op)
    if key not in _alone:
        if prec is None:
            res = T.run_op(op, None, directory)
        else:
            with ctpn_amd.Context(0, *W.CAP, prec) as ctx:
                ctx.load_weights(W.weights())
                res = T.run_op(op, ctx, directory)
        why = T.not_empty(op, res)
        assert why is None, "%s %s alone: %s, an equality with it would be empty" % (prec, op, why)
        _alone[key] = res
    return _alone[key]


@pytest.fixture(scope="module")
def files_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("thread_files"))


def run_child(name, tmp_path):
    """-> (results, extra) of the scenario run in a fresh process"""
    if _hung:
        pytest.skip("not started: " + _hung[0])
    out = str(tmp_path / "out.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(HERE, "thread_child.py"), name, out]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        _hung.append("the child of %s was killed at %d s" % (name, LIMIT))
        err = e.stderr.decode("utf-8", "replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("%s: killed at %d s\n%s" % (name, LIMIT, err[-4000:]))
    if r.returncode < 0:
        _hung.append("the child of %s died of signal %d" % (name, -r.returncode))
        pytest.fail("%s: died of signal %d\n%s" % (name, -r.returncode, r.stderr[-4000:]))
    if r.returncode != 0:      # a worker raised (a HIP error among the possible causes) or a barrier broke (a worker hung): the same caution
        _hung.append("the child of %s ended with exit code %d" % (name, r.returncode))
        pytest.fail("%s: exit code %d\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    results, extra = T.unpack(np.load(out))
    print(r.stdout.strip())
    assert float(extra["seconds"]) < SPLIT_ABOVE, "%s took %.1f s: split it" % (name, float(extra["seconds"]))
    return results, extra


def check(name, results, files_dir):
    sc = T.SCENARIOS[name]
    bad = T.mismatches(results, sc.rounds, lambda t, op: alone(None if op in T.CTXLESS else sc.workers[t].prec, op, files_dir))
    assert not bad, "%s: %d of %d results: %s" % (name, len(bad), len(results), "; ".join(bad[:8]))
    assert len(results) == sum(op is not None for row in sc.rounds for op in row)


def texts_are_empty(name, extra):
    sc = T.SCENARIOS[name]
    for t, spec in enumerate(sc.workers):
        if spec.kind == "ctx":
            texts = [str(x) for x in extra["texts_t%d" % t]]
            assert len(texts) == len(sc.rounds) and not any(texts), "%s thread %d: error texts %r" % (name, t, sorted(set(texts)))


@pytest.mark.parametrize("prec", W.PRECS)
def test_four_ctxs_of_one_precision(prec, tmp_path, files_dir):
    name = "same[%s]" % prec
    results, extra = run_child(name, tmp_path)
    check(name, results, files_dir)
    texts_are_empty(name, extra)


def test_one_ctx_per_precision_and_a_thread_of_errors(tmp_path, files_dir):
    results, extra = run_child("mixed", tmp_path)
    check("mixed", results, files_dir)      # the fifth thread's (code, text) pairs are compared like everything else: with the alone call's
    texts_are_empty("mixed", extra)
    sc = T.SCENARIOS["mixed"]
    for rnd, row in enumerate(sc.rounds):
        code, text = results[(rnd, 4)]
        assert (code,) == T.ERROR_CODES[row[4]] and text, (rnd, row[4], code, text)
    assert len({alone("bf16", op, files_dir)[1] for op in T.ERROR_OPS}) == 3      # three different texts: one read from another thread would show


def test_stateless_calls_beside_a_ctx_with_batches_in_flight(tmp_path, files_dir):
    results, extra = run_child("stateless", tmp_path)
    check("stateless", results, files_dir)
    texts_are_empty("stateless", extra)
    assert T.NMS_SIZES[0] < T.NMS_CACHE_INITIAL < T.NMS_SIZES[1] and T.NMS_SIZES[2] < T.NMS_CACHE_INITIAL


def test_codecs_side_by_side(tmp_path, files_dir):
    results, extra = run_child("codecs", tmp_path)
    check("codecs", results, files_dir)
    texts_are_empty("codecs", extra)


def test_ctxs_come_and_go_beside_a_working_one(tmp_path, files_dir):
    results, extra = run_child("lifecycle", tmp_path)
    check("lifecycle", results, files_dir)
    texts_are_empty("lifecycle", extra)
    # in front of the threads no ctx exists and no cache that the counters see (module docstring); behind them every ctx is destroyed
    print("live resources in front of the threads", extra["live_before"].tolist(), "behind them", extra["live_after"].tolist())
    assert extra["live_before"].tolist() == extra["live_after"].tolist(), (extra["live_before"], extra["live_after"])
