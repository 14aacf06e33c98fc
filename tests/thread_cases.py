"""Cases and harness of the tests that put several ctxs on concurrent host threads (tests/test_thread_cases.py, tests/thread_child.py,
tests/test_gpu_threads.py). The contract (include/ctpn_hip.h): any number of ctxs per device, each used by one host thread at a time; distinct
ctxs and the stateless calls run concurrently. What they share per device -- the weights-in-registers kernel's dump page and claim slots, the
strip stream and its event pair, the function-attribute flags and the CU count, the pixel LUT, the ctpn_nms / ctpn_page_nms caches, the PNG
decode team, the thread-local error text, the live-resource counters -- runs contended here. Test infrastructure only: nothing here needs a
GPU to import, to build its inputs or to build a scenario; an op's run does.

Ops: tests/ctx_walks.py's (OP, inputs, weights, same, CAP, PRECS) and, here alone so that the walks of tests/test_ctx_walks.py enumerate what
they did,

  uE   detect of 3 x 32 x 226, mode H, rois too: conv2_1 runs at 16 x 113 (W mod 16 = 1, not flat) in a batch of 3, where the 16-bit plan
       forks a one-column edge strip onto the device's strip stream beside a weights-in-registers main launch

and the stateless and codec calls (FREE_OPS, CODEC_OPS below): name -> run(ctx or None, files directory) -> a tuple of numpy arrays and ints.

schedule(ops, threads): the rounds of a scenario. run_together(workers, rounds): one thread per worker, a barrier in front of every round.
mismatches(results, rounds, alone): the comparison, byte for byte (ctx_walks.same). SCENARIOS: name -> Scenario(workers, rounds)."""
import collections
import functools
import os
import threading
import time

import numpy as np

import ctx_walks as W

E = (3, 32, 226)
OPS6 = ("uE", "uA", "uB", "uC", "rW", "pAB")          # uE first: round 0 runs it on every thread, and it reaches every first-use path at once
NMS_SIZES = (63, 20000, 64)                            # NmsCache starts at 16 384 boxes: below, above (the blocks are re-grown), below again (reused)
NMS_CACHE_INITIAL = 16384                              # csrc/api_proposals.hip, ctpn_nms
PAGE_NMS = ((1000, 2), (20000, 1024))                  # (r, ncols) of tests/test_gpu_page.py's generator
TARGET_SCENE = "three"                                 # a 6 x 8 map: no scene of tests/golden/anchor_targets.npz is smaller
TAIL_CASES = (("biased", (1, 1, 1)), ("biased", (1, 15, 2)))      # the smallest shape, and the smallest with a recurrence (tests/test_gpu_tail_grad.py)
HUFF_CASES = ("1x1-q90-420", "8x8-flat-gray", "17x9-q90-420")     # the smallest files of tests/jpeg_huff_cases.py
PNG_IMAGES = ("9x85", "9x85-page")                     # one size, the smallest stride-256 pair of tests/png_enc_ref.py


# ---- ops ----
@functools.lru_cache(maxsize=None)
def extra_inputs():
    import ctpn_amd
    x = {"E": ctpn_amd.weights.synthetic_images(*E, 71)}
    for v in x.values():
        v.setflags(write=False)
    return x


def _uE(ctx):
    return W._flat(ctx.detect(extra_inputs()["E"], mode="H", want_rois=True))


OP = dict(W.OP)
OP["uE"] = W.Op("uE", "uniform", _uE)
SHAPES = {"uE": E, "uA": W.A, "uB": W.B, "uC": W.C, "rW": (5, 96, 82)}


def last_error():
    """this thread's error text"""
    from ctpn_amd import _binding as B
    return B.load_library().ctpn_last_error().decode("utf-8", "replace")


def failing(call):
    """-> (return code, this thread's error text) of a call that is expected to fail"""
    import ctpn_amd
    try:
        call()
    except ctpn_amd.CtpnError as e:
        return (int(e.code), last_error())
    return (0, last_error())


def _bad_nms():
    from ctpn_amd import _binding as B
    return B.nms_sorted(np.ones((4, 3), np.float32), 0.7, 0)      # three columns: CTPN_ERR_ARG


ERROR_OPS = {
    "eN": lambda ctx, d=None: failing(lambda: ctx.detect(W.inputs()["six"], want_rois=True)),
    "eH": lambda ctx, d=None: failing(lambda: ctx.forward_ragged(W.inputs()["W"], W.inputs()["Wbad"])),
    "badnms": lambda ctx, d=None: failing(_bad_nms),
}
ERROR_CODES = dict(W.ERROR_CODES, badnms=(-1,))                   # CTPN_ERR_ARG


@functools.lru_cache(maxsize=None)
def free_inputs():
    """the inputs of the stateless calls, generated once, read-only"""
    import page_cases as K
    import tail_grad_cases as TG
    import test_anchor_targets as T
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_targets.npz"))
    maps = {n: int(np.prod(golden[n + "/map"])) for n in T.SCENES}
    assert maps[TARGET_SCENE] == min(maps.values())
    s = T.scene(golden, TARGET_SCENE)
    x = {"scene": s, "heads": T.seeded_heads(s["hf"] * s["wf"], 64, 3).reshape(1, s["hf"], s["wf"], 64)}
    x["heads"][..., 60:] = 0.0
    for r in NMS_SIZES:
        x["nms%d" % r] = K.column_boxes(7 * r + 2, r, 2, span=2400.0)
    for r, ncols in PAGE_NMS:
        x["page%dx%d" % (r, ncols)] = K.column_boxes(7 * r + ncols, r, ncols, span=600.0 if ncols > 2 else 2400.0)
    for kind, (n, hf, wf) in TAIL_CASES:
        x["tail%dx%dx%d" % (n, hf, wf)] = (TG.features(n, hf, wf, kind, 1), TG.tail_weights(kind), TG.head_gradient(n, hf, wf, 1))
    return x


def _targets(ctx, d):
    import ctpn_amd
    s = free_inputs()["scene"]
    t = ctpn_amd.anchor_targets(s["hf"], s["wf"], [s["im_info"]], [s["gt"]], None if s["hard"] is None else [s["hard"]],
                                None if s["dontcare"] is None else [s["dontcare"]], s["cfg12"], 12345, stages=True)
    return tuple(np.asarray(v) for v in t)


def _loss(ctx, d):
    import ctpn_amd
    t = _targets(ctx, d)
    r = ctpn_amd.rpn_loss(free_inputs()["heads"], t[0], t[1], t[2], t[3], want_grad=True)
    return (r.losses, r.counts, r.d_heads)


def _tail(backward):
    def run(ctx, d):
        import ctpn_amd
        out = ()
        for _kind, (n, hf, wf) in TAIL_CASES:
            x, tail, g = free_inputs()["tail%dx%dx%d" % (n, hf, wf)]
            f = ctpn_amd.tail_forward(x, tail)
            if backward:
                b = ctpn_amd.tail_backward(x, tail, f.saved, g, want_dx=True)
                out += (b.d_tail, b.d_x)
            else:
                out += (f.heads, f.saved)
        return out
    return run


def _nms(name, page):
    def run(ctx, d):
        from ctpn_amd import _binding as B
        b = free_inputs()[name]
        keep = (B.page_nms_sorted if page else B.nms_sorted)(b, 0.7, 0)
        return (np.asarray(keep), int(len(keep)))
    return run


FREE_OPS = {"tgt": _targets, "loss": _loss, "tfwd": _tail(False), "tbwd": _tail(True)}
FREE_OPS.update({"nms%d" % r: _nms("nms%d" % r, False) for r in NMS_SIZES})
FREE_OPS.update({"page%dx%d" % p: _nms("page%dx%d" % p, True) for p in PAGE_NMS})


def png_files(directory):
    """PNG_IMAGES as files of `directory`, written by Pillow (once) -> their paths"""
    from PIL import Image
    import png_enc_ref as PR
    os.makedirs(directory, exist_ok=True)
    paths = []
    for name in PNG_IMAGES:
        p = os.path.join(directory, name + ".png")
        if not os.path.exists(p):
            Image.fromarray(np.ascontiguousarray(PR.images()[name][:, :, ::-1])).save(p)
        paths.append(p)
    return paths


@functools.lru_cache(maxsize=None)
def codec_inputs():
    import jpeg_huff_cases as JH
    import jpeg_ragged_cases as JR
    import out_ragged_cases as OR
    import png_enc_ref as PR
    canvas, heights = OR.host_canvas()
    huff = JH.cases()
    return {"jpeg": JR.files(), "huff": [huff[k] for k in HUFF_CASES], "png": np.stack([PR.images()[k] for k in PNG_IMAGES]),
            "mixed": [OR.lone(canvas, heights, i) for i in range(len(heights))]}


def _bytes(files):
    return tuple(np.frombuffer(f, np.uint8) for f in files)


def _png_dec(ctx, d):
    from ctpn_amd import _binding as B
    h, w = codec_inputs()["png"].shape[1:3]
    return (B.decode_png_files(png_files(d), h, w, threads=2),)


def _jpeg_dec(entropy):
    def run(ctx, d):
        import jpeg_ragged_cases as JR
        (ptr, shape), heights = ctx.decode_jpeg_ragged(codec_inputs()["jpeg"], JR.SIZES, JR.FACTORS, JR.HC, JR.WC, entropy=entropy)
        return (ctx.jpeg_batch_fetch(ptr, shape), np.asarray(heights))
    return run


def _huff_dev(ctx, d):
    from ctpn_amd import _binding as B
    return tuple(B.jpeg_entropy_decode_device(ctx, codec_inputs()["huff"]))


CODEC_OPS = {
    "png_dec": _png_dec,
    "jpg_host": _jpeg_dec("host"),
    "jpg_dev": _jpeg_dec("device"),
    "huff_dev": _huff_dev,
    "png_enc": lambda ctx, d: _bytes(ctx.encode_png_batch(codec_inputs()["png"])),
    "jpg_mixed": lambda ctx, d: _bytes(ctx.encode_jpeg_mixed(codec_inputs()["mixed"], quality=95)),
}
CTXLESS = set(FREE_OPS) | {"png_dec"}


def run_op(name, ctx, directory=None):
    """any op of this module by name (eN and eH in the form of ERROR_OPS: with the text)"""
    for table in (ERROR_OPS, FREE_OPS, CODEC_OPS):
        if name in table:
            return table[name](ctx, directory)
    return OP[name].run(ctx)


def not_empty(name, res):
    """None, or why an equality with this alone result would be an equality of nothing (rois > 0, keep count > 0, file bytes > 0, data that
    is not all zero)"""
    if name in ERROR_OPS:
        return None if (res[0],) == ERROR_CODES[name] and res[1] else "code %r, text %r" % (res[0], res[1])
    if name in OP:
        rois = sum(x.shape[0] for x in res if isinstance(x, np.ndarray) and x.ndim == 2 and x.shape[1] == 5 and x.dtype == np.float32)
        return None if rois > 0 else "no roi"
    if name.startswith(("nms", "page")):
        return None if 0 < res[1] <= len(free_inputs()[name]) and len(res[0]) == res[1] else "keep count %d" % res[1]
    empty = [i for i, x in enumerate(res) if not (isinstance(x, np.ndarray) and x.size > 0)]
    if empty:
        return "element %d is empty" % empty[0]
    big = max(res, key=lambda x: x.size)
    return None if big.size >= 64 and np.ascontiguousarray(big).reshape(-1).view(np.uint8).any() else "the largest element is all zero"


# ---- the schedule ----
def schedule(ops, threads):
    """Rounds as tuples of one op per thread. Round 0: ops[0] on every thread -- the process's first forward contends on every first-use path
    at once. Then the cyclic Latin square over the ops (round r, thread t: ops[(r + t) mod k]), in which ops at distance 1 .. threads - 1 run
    side by side, so with threads - 1 >= k // 2 every unordered pair of distinct ops is simultaneous in some round. Then the square again,
    with nothing left to initialise."""
    k = len(ops)
    if threads < 2 or threads - 1 < k // 2 or threads > k:
        raise ValueError("the cyclic square over %d ops covers every pair with %d .. %d threads, not %d" % (k, k // 2 + 1, k, threads))
    square = [tuple(ops[(r + t) % k] for t in range(threads)) for r in range(k)]
    return [tuple(ops[0] for _ in range(threads))] + square + square


# ---- the harness ----
class WorkerError(Exception):
    """a worker raised: .round, .thread, .op and the exception as __cause__"""

    def __init__(self, rnd, thread, op, exc):
        super().__init__("thread %d raised in round %d, op %r: %s: %s" % (thread, rnd, op, type(exc).__name__, exc))
        self.round, self.thread, self.op = rnd, thread, op


class BarrierBroken(Exception):
    """no worker raised, and not every worker reached a round's barrier in time: .round, .missing (threads)"""

    def __init__(self, rnd, missing, timeout):
        super().__init__("broken barrier: round %d, thread(s) %s did not reach it within %.1f s" % (rnd, ", ".join(map(str, missing)) or "?", timeout))
        self.round, self.missing = rnd, missing


def run_together(workers, rounds, timeout=20.0):
    """One threading.Thread per worker; worker.start() (if it has one) runs on its thread before the first round -- a worker creates and owns
    its ctx there -- and worker.stop() after the last. A Barrier(len(workers), timeout) stands in front of every round, so the calls of a round
    start together; rounds[r][t] is handed to workers[t].run; None idles the thread for the round.
    -> {(round, thread): what run returned}. A worker's exception aborts the barrier and is re-raised here as WorkerError (round -1: start,
    round len(rounds): stop); a barrier that broke without one is BarrierBroken."""
    n = len(workers)
    assert all(len(r) == n for r in rounds)
    barrier = threading.Barrier(n, timeout=timeout)
    results, raised, broken = {}, [], []
    at = [-2] * n          # the last round whose barrier the thread reached
    lock = threading.Lock()

    def body(t):
        w = workers[t]
        rnd, op = -1, "start"
        try:
            if hasattr(w, "start"):
                w.start()
            for rnd, item in enumerate(rounds):
                op = item[t]
                at[t] = rnd
                barrier.wait()
                if op is not None:
                    res = w.run(op)
                    with lock:
                        results[(rnd, t)] = res
            rnd, op = len(rounds), "stop"
        except threading.BrokenBarrierError:
            with lock:
                broken.append((rnd, t))
        except BaseException as e:      # noqa: B036 -- reported on the main thread, whatever it is
            with lock:
                raised.append((rnd, t, op, e))
            barrier.abort()
        finally:
            try:
                if hasattr(w, "stop"):
                    w.stop()
            except BaseException as e:      # noqa: B036
                with lock:
                    raised.append((len(rounds), t, "stop", e))
                barrier.abort()

    threads = [threading.Thread(target=body, args=(t,), name="worker-%d" % t, daemon=True) for t in range(n)]
    for th in threads:
        th.start()
    failed_at = None       # once a worker raised or the barrier broke, the others get `timeout` to finish their call and stop
    for th in threads:
        while th.is_alive():
            th.join(0.02)
            if raised or broken:
                failed_at = failed_at or time.monotonic()
                if time.monotonic() - failed_at > timeout:
                    break
    if raised:
        rnd, t, op, e = min(raised, key=lambda x: (x[0], x[1]))
        raise WorkerError(rnd, t, op, e) from e
    stuck = [t for t, th in enumerate(threads) if th.is_alive()]
    if broken or stuck:
        rnd = max([r for r, _ in broken] + [at[t] for t in stuck])
        raise BarrierBroken(rnd, sorted(set(stuck) | {t for t in range(n) if at[t] < rnd}), timeout)
    return results


def mismatches(results, rounds, alone):
    """alone(thread, op) -> the op's result made alone. -> one message per (round, thread) whose result is not that, byte for byte, and per
    (round, thread) that has no result"""
    out = []
    for rnd, item in enumerate(rounds):
        for t, op in enumerate(item):
            if op is None:
                continue
            if (rnd, t) not in results:
                out.append("round %d thread %d: %s has no result" % (rnd, t, op))
                continue
            i = W.same(results[(rnd, t)], alone(t, op))
            if i is not None:
                out.append("round %d thread %d: %s differs from the alone result in element %d (beside %s)" %
                           (rnd, t, op, i, " ".join(str(o) for k, o in enumerate(item) if k != t)))
    return out


# ---- results as a file: {(round, thread): tuple of arrays, ints and strs} <-> the arrays of an .npz ----
def pack(results, extra=None):
    out = {}
    for (rnd, t), res in results.items():
        out["r%d_t%d_n" % (rnd, t)] = np.array(len(res), np.int64)
        for i, x in enumerate(res):
            key = "r%d_t%d_%d" % (rnd, t, i)
            if isinstance(x, np.ndarray):
                out[key + "_a"] = x
            elif isinstance(x, str):
                out[key + "_s"] = np.frombuffer(x.encode("utf-8"), np.uint8)
            elif isinstance(x, (int, np.integer)) and not isinstance(x, bool):
                out[key + "_i"] = np.array(int(x), np.int64)
            else:
                raise TypeError("result element of type %s" % type(x).__name__)
    for k, v in (extra or {}).items():
        out["x_" + k] = np.asarray(v)
    return out


def unpack(npz):
    """-> (results, extra)"""
    results, extra = {}, {}
    for key in npz.files:
        if key.startswith("x_"):
            extra[key[2:]] = npz[key]
        elif key.endswith("_n"):
            r, t = key[:-2].split("_")
            res = []
            for i in range(int(npz[key])):
                base = "%s_%s_%d" % (r, t, i)
                if base + "_a" in npz.files:
                    res.append(npz[base + "_a"])
                elif base + "_s" in npz.files:
                    res.append(npz[base + "_s"].tobytes().decode("utf-8"))
                else:
                    res.append(int(npz[base + "_i"]))
            results[(int(r[1:]), int(t[1:]))] = tuple(res)
    return results, extra


# ---- scenarios ----
# kind: "ctx" -- owns one ctx of capacity CAP in `prec` from start to stop, runs ops on it and notes its thread's error text after every op;
# "errors" -- the same with ERROR_OPS; "free" -- no ctx; "churn" -- every item is create -> load_weights -> the op -> destroy
WorkerSpec = collections.namedtuple("WorkerSpec", "kind prec")
Scenario = collections.namedtuple("Scenario", "workers rounds")


def _cycle(items, n):
    return [items[i % len(items)] for i in range(n)]


def _columns(*cols):
    return [tuple(c[r] for c in cols) for r in range(len(cols[0]))]


def _scenarios():
    s = {}
    grid = schedule(OPS6, 4)
    for prec in W.PRECS:
        s["same[%s]" % prec] = Scenario(tuple(WorkerSpec("ctx", prec) for _ in range(4)), grid)
    s["mixed"] = Scenario(tuple(WorkerSpec("ctx", p) for p in W.PRECS) + (WorkerSpec("errors", "bf16"),),
                          [row + (e,) for row, e in zip(grid, _cycle(("eN", "eH", "badnms"), len(grid)))])
    n = 10      # thread 3's five sizes twice: the second time every block is there
    s["stateless"] = Scenario((WorkerSpec("ctx", "bf16"), WorkerSpec("free", None), WorkerSpec("free", None), WorkerSpec("free", None)),
                              _columns(_cycle(("pAB", "pRC"), n), _cycle(("tgt", "loss"), n), _cycle(("tfwd", "tbwd"), n),
                                       _cycle(tuple("nms%d" % r for r in NMS_SIZES) + tuple("page%dx%d" % p for p in PAGE_NMS), n)))
    n = 6
    s["codecs"] = Scenario((WorkerSpec("free", None),) + tuple(WorkerSpec("ctx", "bf16") for _ in range(3)),
                           _columns(_cycle(("png_dec",), n), _cycle(("jpg_host",), n), _cycle(("jpg_dev", "huff_dev"), n), _cycle(("png_enc", "jpg_mixed"), n)))
    s["lifecycle"] = Scenario((WorkerSpec("ctx", "fp16"), WorkerSpec("churn", "bf16"), WorkerSpec("churn", "split")),
                              _columns(_cycle(("uC", "uE"), n), _cycle(("uC",), n), _cycle(("uC",), n)))
    return s


SCENARIOS = _scenarios()


def alone_keys(name):
    """the (precision or None, op) pairs whose alone results the scenario is held against"""
    sc = SCENARIOS[name]
    return sorted({(sc.workers[t].prec if op not in CTXLESS else None, op) for row in sc.rounds for t, op in enumerate(row) if op is not None},
                  key=lambda k: (str(k[0]), k[1]))
