"""CPU: the cases of tests/test_gpu_ctx_forgets.py cannot pass vacuously -- the pair walk holds every ordered pair, the seeded walks put every
state-only action in front of every kind of data-op, and the comparison notices one bit, a dtype, a shape (tests/ctx_walks.py)."""
import collections

import numpy as np
import pytest

import ctx_walks as W

SEEDS = (1, 2, 3)          # the seeds of tests/test_gpu_ctx_forgets.py
STEPS = 120


@pytest.mark.parametrize("k", [1, 2, 3, len(W.OPS)])
def test_pair_walk_holds_every_ordered_pair_once(k):
    walk = W.pair_walk(k)
    assert len(walk) == k * k + 1 and walk[0] == walk[-1] and all(0 <= v < k for v in walk)
    pairs = collections.Counter(zip(walk, walk[1:]))
    assert len(pairs) == k * k and set(pairs.values()) == {1}
    assert set(pairs) == {(x, y) for x in range(k) for y in range(k)}
    assert W.pair_walk(k) == walk


def test_the_ops_are_the_issues():
    names = [o.name for o in W.OPS]
    assert names == ["uA", "uB", "uC", "uC2", "uC1", "dC", "uD", "rW", "rW2", "rF", "uW", "tA", "bD", "pAB", "pRC", "eN", "eH"]
    assert len(set(names)) == len(names) and {o.kind for o in W.OPS} == set(W.KINDS)
    assert set(W.ERROR_CODES) == {o.name for o in W.OPS if o.kind == "error"}
    assert {m for _, m in W.LINES.values()} == {"H", "O"}


def test_inputs_are_what_the_ops_say_and_read_only():
    x = W.inputs()
    assert x is W.inputs()
    assert x["A"].shape == (3, 32, 1040, 3) and x["B"].shape == (3, 304, 264, 3) and x["D"].shape == (1, 96, 160, 3)
    assert x["C"].shape == x["C2"].shape == (2, 64, 96, 3) and not np.array_equal(x["C"], x["C2"]) and np.array_equal(x["C1"][0], x["C"][0])
    assert x["W"].shape == (5, 96, 82, 3) and list(x["Wh"]) == [96, 80, 49, 16, 33] and list(x["Wfull"]) == [96] * 5 and list(x["Wbad"]) == [96, 80, 49, 15, 33]
    assert sorted(W.W_ORDER) == list(range(5)) and list(W.W_ORDER) != list(range(5))
    for j, i in enumerate(W.W_ORDER):
        assert np.array_equal(x["W2"][j], x["W"][i]) and x["W2h"][j] == x["Wh"][i]
    assert x["Dblob"].dtype == np.float32 and x["Dblob"].shape == x["D"].shape and x["six"].shape[0] == W.CAP[0] + 1
    for shape in (W.A, W.B, W.C, W.D, x["W"].shape[:3]):
        assert all(s <= c for s, c in zip(shape, W.CAP))
    assert all(not v.flags.writeable for v in x.values()) and not W.weights().flags.writeable


def test_random_walk_is_reproducible_and_covers_every_action_before_every_kind():
    seen = set()
    for seed in SEEDS:
        walk = W.random_walk(seed, STEPS)
        assert walk == W.random_walk(seed, STEPS)
        assert sum(1 for it in walk if it[0] == "op") == STEPS
        assert all(it in W.STATE_ACTIONS or (it[0] == "op" and it[1] in W.OP) for it in walk)
        for a, b in zip(walk, walk[1:]):
            if a[0] != "op":
                assert b[0] == "op"                       # an action stands directly in front of a data-op
                seen.add((a, W.OP[b[1]].kind))
    assert W.random_walk(SEEDS[0], STEPS) != W.random_walk(SEEDS[1], STEPS)
    assert len(W.STATE_ACTIONS) == 17
    assert seen == {(a, kind) for a in W.STATE_ACTIONS for kind in W.KINDS}


def _result():
    rng = np.random.default_rng(5)
    return (rng.standard_normal((3, 9)), rng.standard_normal((2, 5)).astype(np.float32), np.zeros((0, 9)), rng.integers(0, 99, (4,)).astype(np.int32), -4)


def test_same_has_teeth():
    a = _result()
    assert W.same(a, _result()) is None and W.same((), ()) is None
    for i, x in enumerate(a):
        if not isinstance(x, np.ndarray):
            assert W.same(a, a[:i] + (x + 1,) + a[i + 1:]) == i
            assert W.same(a, a[:i] + (np.array([x]),) + a[i + 1:]) == i and W.same(a[:i] + (np.array([x]),) + a[i + 1:], a) == i
            continue
        for bit in range(x.nbytes * 8):                                        # one flipped bit, any bit of any element
            raw = bytearray(x.tobytes())
            raw[bit >> 3] ^= 1 << (bit & 7)
            y = np.frombuffer(bytes(raw), x.dtype).reshape(x.shape)
            assert W.same(a, a[:i] + (y,) + a[i + 1:]) == i, (i, bit)
        other = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.int32, np.dtype(np.int32): np.float32}[x.dtype]
        assert W.same(a, a[:i] + (x.view(other),) + a[i + 1:]) == i              # the same bytes under another dtype
        assert W.same(a, a[:i] + (x.reshape(x.shape[::-1] if x.ndim > 1 else (2, -1)),) + a[i + 1:]) == i   # ... and in another shape
    assert W.same(a, a[:-1]) == len(a) - 1 and W.same(a[:2], a) == 2           # a prefix is not the tuple
    assert W.same((np.float32(-0.0).reshape(1),), (np.float32(0.0).reshape(1),)) == 0      # bytes, not values
