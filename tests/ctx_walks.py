"""Cases for the tests that hold a ctx to have no memory (tests/test_ctx_walks.py, tests/test_gpu_ctx_forgets.py): a call's result depends
on its arguments and on the ctx's options and parameters, not on what the ctx did before. Test infrastructure only; nothing here needs a GPU
to import or to build its inputs -- an op's run(ctx) does.

Data-ops: name -> Op(kind, run), run(ctx) -> a tuple of numpy arrays and ints. Everything fits a ctx of capacity CAP = (5, 304, 1040). Shapes
that cross kernel forms at small size: A and B of tests/test_gpu_two_forwards.py, the w = 82 ragged set of tests/ragged_ref.py.

  uA   detect of 3 x 32 x 1040, mode H                uB   detect of 3 x 304 x 264              uC   detect of 2 x 64 x 96
  uC2  other images of uC's geometry (no re-zero)     uC1  uC's first image alone               dC   uC's images through device_ptr= (= uC)
  uD   detect of 1 x 96 x 160, mode O                 rW   detect_ragged 5 x 96 x 82, heights 96, 80, 49, 16, 33
  rW2  rW's images in another order                   rF   the canvas with every height 96      uW   the canvas as a uniform batch
  tA   forward(A), heads, rpn_conv/3x3, proposals     bD   forward_blob of D's float blob, proposals, heads (ctpn_forward_blob takes a blob in
  pAB  submit A slot 0, B slot 1, collect 0, 1             every precision: the op is in every precision's set)
  pRC  submit rW slot 1, uC slot 0, collect 1, 0      eN   detect of 6 images: the error code   eH   forward_ragged with a height of 15: the code

Every detect form asks for the rois too. Weights: tests/util.py's "biased" arena.

pair_walk(k): every ordered pair of k ops exactly once as neighbours. random_walk(seed, steps): data-ops with the state-only actions between them
whose results the suite holds to be byte-invariant. same(a, b): the comparison."""
import collections
import functools

import numpy as np

import ragged_ref as R
import util

CAP = (5, 304, 1040)
PRECS = ("fp32", "split", "fp16", "bf16")
A, B, C, D = (3, 32, 1040), (3, 304, 264), (2, 64, 96), (1, 96, 160)
W_ORDER = (3, 0, 4, 2, 1)

Op = collections.namedtuple("Op", "name kind run")


@functools.lru_cache(maxsize=None)
def weights():
    w = util.stress_arena("biased")
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> array: generated once, read-only"""
    import ctpn_amd
    from oracle import network as N
    syn = ctpn_amd.weights.synthetic_images
    x = {"A": syn(*A, 21), "B": syn(*B, 22), "C": syn(*C, 31), "C2": syn(*C, 51), "D": syn(*D, 32)}
    x["C1"] = np.ascontiguousarray(x["C"][:1])
    canvas, heights = R.canvas_of(R.images(11), R.HC)
    x["W"], x["Wh"] = canvas, heights
    x["W2"], x["W2h"] = np.ascontiguousarray(canvas[list(W_ORDER)]), np.ascontiguousarray(heights[list(W_ORDER)])
    x["Wfull"] = np.full(len(heights), R.HC, np.int32)
    x["Wbad"] = np.array([96, 80, 49, 15, 33], np.int32)
    x["Dblob"] = np.ascontiguousarray(N.image_blob(x["D"]), dtype=np.float32)
    x["six"] = syn(6, 16, 16, 61)
    for v in x.values():
        v.setflags(write=False)
    return x


def _flat(*results):
    """(lines, rois) pairs of detect calls -> one tuple of arrays"""
    out = []
    for lines, rois in results:
        out += list(lines) + list(rois)
    return tuple(out)


def _info(heights, w):
    return np.array([[h, w, 1.0] for h in heights], np.float32)


_dev = {}


def _on_device(name):
    """the input as a device tensor of this process (torch), uploaded once"""
    import torch
    if name not in _dev:
        _dev[name] = torch.from_numpy(np.array(inputs()[name])).cuda()
        torch.cuda.synchronize()
    return _dev[name]


def _code(call):
    import ctpn_amd
    try:
        call()
    except ctpn_amd.CtpnError as e:
        return (int(e.code),)
    return (0,)


def _detect(name, mode="H"):
    return lambda ctx: _flat(ctx.detect(inputs()[name], mode=mode, want_rois=True))


def _ragged(canvas, heights):
    return lambda ctx: _flat(ctx.detect_ragged(inputs()[canvas], inputs()[heights], want_rois=True))


def _dC(ctx):
    t = _on_device("C")
    return _flat(ctx.detect(device_ptr=t.data_ptr(), shape=C, want_rois=True))


def _tA(ctx):
    ctx.forward(inputs()["A"])
    heads, rpn = ctx.get_tensor("heads"), ctx.get_tensor("rpn_conv/3x3")
    rois, anchors = ctx.proposals(_info([A[1]] * A[0], A[2]), want_anchors=True)
    return (heads, rpn) + tuple(rois) + tuple(anchors)


def _bD(ctx):
    ctx.forward_blob(inputs()["Dblob"])
    rois = ctx.proposals(_info([D[1]], D[2]))
    return tuple(rois) + (ctx.get_tensor("heads"),)


def _pAB(ctx):
    ctx.detect_submit(images=inputs()["A"], slot=0)
    ctx.detect_submit(images=inputs()["B"], slot=1)
    a = ctx.detect_collect(0, want_rois=True)
    return _flat(a, ctx.detect_collect(1, want_rois=True))


def _pRC(ctx):
    ctx.detect_submit(images=inputs()["W"], slot=1, heights=inputs()["Wh"])
    ctx.detect_submit(images=inputs()["C"], slot=0)
    r = ctx.detect_collect(1, want_rois=True)
    return _flat(r, ctx.detect_collect(0, want_rois=True))


OPS = (
    Op("uA", "uniform", _detect("A")),
    Op("uB", "uniform", _detect("B")),
    Op("uC", "uniform", _detect("C")),
    Op("uC2", "uniform", _detect("C2")),
    Op("uC1", "uniform", _detect("C1")),
    Op("dC", "uniform", _dC),
    Op("uD", "uniform", _detect("D", "O")),
    Op("rW", "ragged", _ragged("W", "Wh")),
    Op("rW2", "ragged", _ragged("W2", "W2h")),
    Op("rF", "ragged", _ragged("W", "Wfull")),
    Op("uW", "uniform", _detect("W")),
    Op("tA", "uniform", _tA),
    Op("bD", "uniform", _bD),
    Op("pAB", "pipelined", _pAB),
    Op("pRC", "pipelined", _pRC),
    Op("eN", "error", lambda ctx: _code(lambda: ctx.detect(inputs()["six"], want_rois=True))),
    Op("eH", "error", lambda ctx: _code(lambda: ctx.forward_ragged(inputs()["W"], inputs()["Wbad"]))),
)
OP = {o.name: o for o in OPS}
KINDS = ("uniform", "ragged", "pipelined", "error")
ERROR_CODES = {"eN": (-4,), "eH": (-1,)}          # CTPN_ERR_CAPACITY, CTPN_ERR_ARG (include/ctpn_hip.h)
# how many leading elements of a result are text-line arrays, and in which DETECT_MODE (the non-empty condition of the GPU tests)
LINES = {"uA": (3, "H"), "uB": (3, "H"), "uC": (2, "H"), "uC2": (2, "H"), "uC1": (1, "H"), "dC": (2, "H"), "uD": (1, "O"), "rW": (5, "H"),
         "rW2": (5, "H"), "rF": (5, "H"), "uW": (5, "H")}

# state-only actions: ("option", name, value) -> ctx.set_option, ("reserve", n) -> ctx.reserve_proposals (RPN_POST_NMS_TOP_N stays 1000)
STATE_ACTIONS = tuple(("option", "nms_columns", v) for v in range(4)) + \
    tuple(("option", nm, v) for nm in ("nms_prefix", "nms_check", "connect_device", "tail_overlap", "tail_confine") for v in (0, 1)) + \
    tuple(("reserve", n) for n in (1000, 2048, 4096))


def apply_action(ctx, action):
    if action[0] == "option":
        ctx.set_option(action[1], action[2])
    else:
        ctx.reserve_proposals(action[1])


def pair_walk(k):
    """An Eulerian circuit of the complete directed graph with self-loops on k nodes, by Hierholzer from node 0, every node's edges taken in
    ascending order of their target: k * k + 1 indices in which every ordered pair (x, y), x == y included, occurs exactly once as neighbours."""
    nxt = [0] * k
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            nxt[v] += 1
            stack.append(nxt[v] - 1)
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def random_walk(seed, steps):
    """`steps` data-ops with state-only actions between them, from numpy.random.default_rng(seed): a list of ("op", name) and STATE_ACTIONS
    items. Every (action, kind of data-op) cell is drawn once per walk, in shuffled order and with a random op of the kind, as an action
    directly in front of the op, while `steps` lasts; the remaining ops are random and follow their predecessor directly."""
    rng = np.random.default_rng(seed)
    cells = [(a, kind) for a in STATE_ACTIONS for kind in KINDS]
    cells = [cells[i] for i in rng.permutation(len(cells))][:steps]
    by_kind = {kind: [o.name for o in OPS if o.kind == kind] for kind in KINDS}
    slots = [None] * (steps - len(cells)) + cells
    slots = [slots[i] for i in rng.permutation(len(slots))]
    walk = []
    for cell in slots:
        if cell is None:
            walk.append(("op", OPS[int(rng.integers(len(OPS)))].name))
        else:
            names = by_kind[cell[1]]
            walk += [cell[0], ("op", names[int(rng.integers(len(names)))])]
    return walk


def same(a, b):
    """None where the tuples a and b agree in length and, element by element, in kind, shape, dtype and bytes; else the index of the first
    element that differs (the shorter length where one tuple is a prefix of the other)."""
    for i, (x, y) in enumerate(zip(a, b)):
        xa, ya = isinstance(x, np.ndarray), isinstance(y, np.ndarray)
        if xa != ya:
            return i
        if xa:
            if x.shape != y.shape or x.dtype != y.dtype or np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes():
                return i
        elif type(x) is not type(y) or x != y:
            return i
    return None if len(a) == len(b) else min(len(a), len(b))
