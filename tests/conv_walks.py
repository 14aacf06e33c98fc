"""The tile walks of the persistent conv3x3 kernels (conv3x3_p_kernel, conv3x3_wr_kernel), enumerated through the library's own walk function
(ctpn_debug_conv3x3_walk_plan: the struct c3_launch_p / c3_launch_wr copy into the kernel argument, csrc/conv3x3_plan.h c3_walk) -- no device
needed, the CU count is an argument. tests/conv_forms.py enumerates WHICH kernel a shape takes, at the smallest shape, where no workgroup
starts a second tile; this census enumerates where a tile falls in the walk, with the CU count of the launch overridden
(ctpn_debug_conv3x3_walk's cu_count: G = 3 .. 24 workgroups on maps of a few thousand pixels).

A WALK CELL is precision / main form / situation. The situations of a persistent form (G workers, `total` whole-tile items, HT = a form that
splits tail tiles into halves: p_flat, p_16x16, p_8x32_half):
    rounds            total = q G, q >= 3, no halves: every worker runs a first, a middle and a last item
    partial           total = q G + r, q >= 1, 2 r > G, no halves: some workers run one item fewer and end on the "current item again" prefetch
    tail              HT: ht_full > 0 and ht_r > 0 -- workers go whole -> half 0, whole -> half 1 and, where r allows (2 r < G), whole -> nothing;
                      some second half holds pixels of the map (a half below the last row stores nothing)
    halves            HT: every item is a half (2 total <= G's CU count); the default at the small shapes of tests/conv_form_cases.py, the anchor
    deal_lt8          G < 8: the XCD deal of w0 with xq = 0;   deal_rem: G = 8 k + j, k >= 1, j != 0; both with a second round
    slice{2,4}_keep   tiles_n 2 / 4, G a multiple of it: a worker keeps its channel slice from item to item
    slice{2,4}_change tiles_n 2 / 4, G odd: every item changes it
                      (a walk with half items -- a tail tile's slice is its tile's, not its item's -- is judged from the schedule: p_8x32_half's cells)
    seam_stacked      stacked tile rows, n = 3: a tile across the seam of two images is some worker's second or later item
    seam_half         stacked tile rows (two or three images): a tile that runs as two halves lies across the seam of two images
    seam_per_image    n = 3, H < 16 (never stacked), no pool: tiles restart per image, later items lie in later images
    seam_pooled       n = 3 with the fused pool (tiles per image)
    seam_flat         flat windows, n = 3: a window across two images is a second or later item
    chunks_odd/_even  an odd / even number of 128-byte K chunks per tile with a second item per worker (wpar's parity at a tile's start)
and of the weights-in-registers kernel (W workers per group and slice; the fused conv1_1 form "wr_fused" walks the same way):
    static2 .. 5      the busiest worker runs that many items, all static (per_group <= 5 W)
    claims            W = 1 and per_group >= 8: every worker's sixth and later items come from the group's counter, three at least
    uneven            pixel tiles not a multiple of 8, more than one item per worker: the last non-empty range is shorter than the others, its workers end early
    empty             fewer tiles than groups: whole groups leave through the early exit, and still count as finished
    sets              one worker ends on register set 0 (odd number of items), another on set 1
NO_CASE names what a form cannot reach, and why.

census() -> {cell: (n, h, w, ci, co, pool, keep_full, dup_hi, cu_count)}, the cheapest shape (n h w ci co) of GRID that reaches each cell;
conv_walk_cases.CASES is the committed table (regenerate from the repository root: PYTHONPATH=. python tests/conv_walks.py > tests/conv_walk_cases.py).
DEVICE_CASES is the second, small list at cu_count 0 (the device's own count; generated for 256 CUs): per form and precision the cheapest shape
with two or more rounds, and per 16-bit mode one wr launch at Co = 128 whose ranges outlast the static items (per_group > 80).
tests/test_conv_walks.py keeps the table true, re-derives every case's situation from restate() + schedule_p() / schedule_wr() (an independent
Python restatement of the walk) and shows that defective walks fail the judges; tests/test_gpu_conv_walks.py runs every case."""
import functools

import numpy as np

from ctpn_amd import _binding as B
from oracle.rounding import bf16_round, fp16_round

CU = 256                                       # the CU count DEVICE_CASES is generated for
PRECS = ("fp32", "split", "fp16", "bf16")
P_FORMS = ("p64", "p_flat", "p_flat64", "p_16x16", "p_8x32", "p_8x32_half")
HT_FORMS = ("p_flat", "p_16x16", "p_8x32_half")
P_SITUATIONS = ("rounds", "partial", "tail", "halves", "deal_lt8", "deal_rem", "slice2_keep", "slice2_change", "slice4_keep", "slice4_change",
                "seam_stacked", "seam_half", "seam_per_image", "seam_pooled", "seam_flat", "chunks_odd", "chunks_even")
WR_SITUATIONS = ("static2", "static3", "static4", "static5", "claims", "uneven", "empty", "sets")
WR_MODES = (("full", False, True), ("pool", True, False), ("pool+full", True, True))
# the search grid of the override list
GRID_N = (1, 2, 3)
GRID_H = (6, 8, 9, 15, 16, 17, 20, 24, 25, 32, 33, 41, 48, 64)      # 25, 41: h % 16 = 9 -- three images in 16-row patches stack (conv4_x's 75 rows)
GRID_W = (16, 24, 32, 40, 48, 64, 72, 96, 104, 112, 120, 128, 144, 152, 160, 192, 256)      # none of them has a strip: the walk covers the width
GRID_CH = ((64, 64), (128, 64), (64, 128), (128, 128), (64, 256), (64, 512))
GRID_CH_FP32 = ((32, 128), (96, 128))          # fp32 K chunks are 32 channels: one and three chunks per tile
GRID_POOL = ((False, True), (True, False), (True, True))
GRID_CU = (3, 4, 5, 7, 8, 9, 12, 16, 24)
MAX_ITEMS = 400
# What no case can reach. Keys are cell prefixes.
NO_CASE = {
    "*/p_flat64/rounds|partial|tail|halves|deal_*|slice*_change|seam_*|chunks_*": "the plan takes p_flat64 only where every 64-pixel item has a CU of its own "
        "(t64 <= CU count): one round, one item per worker, whatever the override. Its cells are `one_round` (anchor) and slice{2,4}_keep.",
    "*/p_8x32_half": "`rounds` and `partial` ARE reached although the plan takes this form for a last round at most half full: the plan counts tiles per "
        "image, the launcher stacks the tile rows of two images, and the stacked count can be a whole number of rounds. Its slice cells include walks "
        "with half items (a tail tile's slice is its tile's, not its item's): they are judged from the schedule",
    "*/p64/slice*": "Co = 64 is one channel slice",
    "*/p64|p_8x32|p_flat64/tail|halves": "these forms never split a tile",
    "*/p_flat|p_flat64/seam_stacked|seam_per_image|seam_pooled": "flat windows have no 2D tiles and no pool: seam_flat is their seam",
    "*/p64|p_16x16|p_8x32|p_8x32_half/seam_flat": "2D patches",
    "*/p_8x32_half/seam_stacked|seam_per_image|seam_pooled": "p_8x32_half is taken for one or two images: its seam is seam_half",
    "*/p64|p_8x32|p_flat|p_flat64/seam_half": "no half items, or no 2D tiles",
    "*/p_8x32_half/seam_half": "not reached: a search over two images of 16 .. 69 rows and 16 .. 256 columns at 3 .. 32 CUs finds no stacked walk of this form "
        "whose tail reaches back to the tile row across the seam (the tail is at most half a round and lies in the second image)",
    "chunks": "the issue expected an odd chunk count in p64 alone (split precision, Ci = 64: 3). Ci = 64 gives 3 chunks in every split-precision form and 1 in "
              "the 16-bit forms behind Co = 256 / 512, Ci = 32 / 96 give 1 / 3 in fp32: the census holds them",
}


@functools.lru_cache(maxsize=None)
def main_names():
    return B.conv3x3_form_names()[0]


def walk_of(prec, case, cu=None):
    """the library's walk of one case (ConvWalk); cu: another CU count than the case's (0: the current device's)"""
    n, h, w, ci, co, pool, keep, dup, cu_case = case
    return B.conv3x3_walk_plan(prec, n, h, w, ci, co, pool, keep or not pool, dup, cu_count=cu_case if cu is None else cu)


# ---------------------------------------------------------------------------------------------------------------
# an independent restatement of the walk: the launchers' numbers from the shape, then which worker runs which item
# ---------------------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def restate(prec, form, case):
    """the numbers of ctpn_debug_conv3x3_walk_plan from (form, shape, CU count), in Python: a dict with ConvWalk's fields"""
    n, h, w, ci, co, pool, keep, _dup, cu = case
    keep = keep or not pool
    he, we = (h, w) if keep else (h & ~1, w & ~1)      # a pool that keeps no full map never reads an odd last row / column (no strip in GRID_W)
    k = dict(main=form, tiles_x=0, tiles_y=0, tiles_n=0, stacked=0, total=0, workers=0, ht_full=0, ht_r=0, groups=0, per_group=0, grid=0,
             chunks=(3 * ci if prec == "split" else ci) // (32 if prec == "fp32" else 64), ht=0)
    if form == "wr":
        k.update(tiles_x=_ceil(we, 32), tiles_y=_ceil(he, 8), tiles_n=co // 64, groups=8)
        k["total"] = n * k["tiles_x"] * k["tiles_y"]
        k["per_group"] = _ceil(k["total"], 8)
        k["workers"] = min(max(cu // k["tiles_n"] // 8, 1), k["per_group"])
        k["grid"] = k["workers"] * 8 * k["tiles_n"]
        return k
    flat = form in ("p_flat", "p_flat64")
    tw = 16 if form == "p_16x16" else 32
    bn, bm = (64 if form == "p64" else 128), (64 if form == "p_flat64" else 256)
    k["ht"] = int(form in HT_FORMS)
    k["tiles_n"] = _ceil(co, bn)
    if flat:
        ptiles = _ceil(n * (h + 2) * (w + 2), bm)
    else:
        th = 256 // tw
        k["tiles_x"], k["tiles_y"] = _ceil(we, tw), _ceil(he, th)
        ptiles = n * k["tiles_x"] * k["tiles_y"]
        stacked_rows = _ceil(n * (h + 2) - 2, th)
        if not pool and h >= 16 and n > 1 and stacked_rows < n * k["tiles_y"]:
            k["stacked"], k["tiles_y"] = 1, stacked_rows
            ptiles = k["tiles_x"] * stacked_rows
    total = k["total"] = ptiles * k["tiles_n"]
    k["workers"], k["ht_full"] = min(total, cu), total
    if k["ht"]:
        if 2 * total <= cu:
            k["ht_full"], k["ht_r"], k["workers"] = 0, total, 2 * total
        else:
            r = total % k["workers"]
            if r > 0 and 2 * r <= k["workers"]:
                k["ht_r"], k["ht_full"] = r, total - r
    k["grid"] = k["workers"]
    return k


def schedule_p(k):
    """conv3x3_p_kernel: [worker (workgroup id)] -> [(tile, half)] in the order it runs them; half -1 = whole, 0 / 1 = first / second 128 pixels"""
    G = k["workers"]
    xq, xr = G >> 3, G & 7
    out = []
    for bid in range(G):
        xcd = bid & 7
        w0 = (xcd * (xq + 1) if xcd < xr else xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3)
        items, lid = [], w0
        while lid < k["ht_full"] + 2 * k["ht_r"]:
            if lid < k["ht_full"]:
                items.append((lid, -1))
            else:
                o = lid - k["ht_full"]
                items.append((k["ht_full"] + (o >> 1), o & 1))
            lid += G
        out.append(items)
    return out


def schedule_wr(k):
    """conv3x3_wr_kernel: {(group, worker)} -> [tile] per channel slice; the five static items, then the group's counter -- which worker a claim
    goes to is decided at run time unless the group has one worker, so claimed tiles are listed for W = 1 only (else: the key "claimed")"""
    W, per, total = k["workers"], k["per_group"], k["total"]
    out = {}
    for grp in range(8):
        lo, end = grp * per, min(grp * per + per, total)
        for j in range(W):
            out[(grp, j)] = [lo + j + i * W for i in range(5) if lo + j + i * W < end]
        claimed = list(range(lo + 5 * W, end))
        if W == 1:
            out[(grp, 0)] += claimed
        elif claimed:
            out[(grp, "claimed")] = claimed
    return out


def _tile_spans_images(k, case, tile):
    """does the pixel tile of item `tile` hold output rows / pixels of two images (stacked tile rows, flat windows)"""
    n, h, w = case[:3]
    pt = tile // k["tiles_n"]
    if k["main"] in ("p_flat", "p_flat64"):
        bm, per = (64 if k["main"] == "p_flat64" else 256), (h + 2) * (w + 2)
        return pt * bm // per != min((pt + 1) * bm - 1, n * per - 1) // per
    if not k["stacked"]:
        return False
    th = 16 if k["main"] == "p_16x16" else 8
    y0 = (pt // k["tiles_x"]) * th
    return (y0 + 1) // (h + 2) != min(y0 + th, n * (h + 2) - 1) // (h + 2)


def _half_live(k, case, tile, half):
    """does half `half` of the pixel tile of item `tile` hold a pixel of the map (a half beyond the last row stores nothing)"""
    n, h, w = case[:3]
    pt = tile // k["tiles_n"]
    if k["main"] == "p_flat":
        per = (h + 2) * (w + 2)
        q = np.arange(pt * 256 + 128 * half, min(pt * 256 + 128 * half + 128, n * per))
        y, x = q % per // (w + 2), q % per % (w + 2)
        return bool(((y >= 1) & (y <= h) & (x >= 1) & (x <= w)).any())
    th = 16 if k["main"] == "p_16x16" else 8
    if k["stacked"]:
        r = (pt // k["tiles_x"]) * th + half * (th // 2) + 1 + np.arange(th // 2)
        return bool(((r < n * (h + 2) - 1) & (r % (h + 2) >= 1) & (r % (h + 2) <= h)).any())
    return (pt % (k["tiles_x"] * k["tiles_y"])) // k["tiles_x"] * th + half * (th // 2) < h


def _second_halves_live(k, case):
    """some tile that runs as two halves has pixels of the map in its second half"""
    return any(_half_live(k, case, t, 1) for t in range(k["ht_full"], k["ht_full"] + k["ht_r"]))


def _slice_situations(k, sched):
    """slice{2,4}_keep / _change from which item every worker runs. Whole rounds only: G a multiple of tiles_n / G odd, as the cells are defined;
    with half items (a tail tile's index is not its item's) whatever the schedule shows"""
    tn, G, found = k["tiles_n"], k["workers"], set()
    slices = [[t % tn for t, _ in v] for v in sched]
    if all(len(set(s)) == 1 for s in slices) and (k["ht_r"] or G % tn == 0):
        found.add("slice%d_keep" % tn)
    if all(a != b for s in slices for a, b in zip(s, s[1:])) and (k["ht_r"] or G % 2):
        found.add("slice%d_change" % tn)
    return found


def situations_from_schedule(prec, form, case):
    """the situations of a case, from restate() and the schedule alone -- no call into the library"""
    n, h, w, ci, co, pool, keep, _dup, cu = case
    k = restate(prec, form, case)
    found = set()
    if form == "wr":
        sched = schedule_wr(k)
        workers = {key: v for key, v in sched.items() if key[1] != "claimed"}
        counts = [len(v) for v in workers.values()]
        has_claims = any(key[1] == "claimed" for key in sched) or any(len(v) > 5 for v in workers.values())
        if not has_claims and 2 <= max(counts) <= 5:
            found.add("static%d" % max(counts))
        if k["workers"] == 1 and min(len(v) for v in workers.values()) >= 8:
            found.add("claims")
        lens = [max(0, min(g * k["per_group"] + k["per_group"], k["total"]) - g * k["per_group"]) for g in range(8)]
        if k["total"] % 8 and k["per_group"] > k["workers"] and any(0 < x < k["per_group"] for x in lens):
            found.add("uneven")
        if k["total"] < 8:
            found.add("empty")
        if not has_claims or k["workers"] == 1:
            par = {c & 1 for c in counts if c}
            if par == {0, 1}:
                found.add("sets")
        return found
    sched = schedule_p(k)
    counts = [len(v) for v in sched]
    G, total = k["workers"], k["total"]
    halves = [it for v in sched for it in v if it[1] >= 0]
    two = min(counts) >= 2
    if form == "p_flat64":
        assert max(counts) == 1
        found.add("one_round")
        if k["tiles_n"] in (2, 4) and G % k["tiles_n"] == 0:
            found.add("slice%d_keep" % k["tiles_n"])
        return found
    if not halves and min(counts) == max(counts) >= 3:
        found.add("rounds")
    if not halves and max(counts) == min(counts) + 1 and min(counts) >= 1 and 2 * sum(c == max(counts) for c in counts) > G:
        found.add("partial")
    if halves and len(halves) < sum(counts):
        ends = {(v[-2][1], v[-1][1]) for v in sched if len(v) > 1}
        if (-1, 0) in ends and (-1, 1) in ends and (any(v[-1][1] < 0 for v in sched) or 2 * k["ht_r"] == G) and any(_half_live(k, case, t, 1) for t, hf in halves if hf):
            found.add("tail")
    if halves and len(halves) == sum(counts) and any(_half_live(k, case, t, 1) for t, hf in halves if hf):
        found.add("halves")
    if max(counts) >= 2:
        if G < 8:
            found.add("deal_lt8")
        elif G % 8:
            found.add("deal_rem")
    if k["tiles_n"] in (2, 4) and two:
        found |= _slice_situations(k, sched)
    if n == 3 and two:
        later = [t for v in sched for t, _ in v[1:]]
        if form in ("p_flat",):
            if any(_tile_spans_images(k, case, t) for t in later):
                found.add("seam_flat")
        elif pool:
            found.add("seam_pooled")
        elif k["stacked"]:
            if any(_tile_spans_images(k, case, t) for t in later):
                found.add("seam_stacked")
        elif h < 16:
            per_img = k["tiles_x"] * k["tiles_y"] * k["tiles_n"]
            if any(t // per_img >= 1 for t in later):
                found.add("seam_per_image")
    if k["stacked"] and any(_tile_spans_images(k, case, t) for t, hf in halves if hf):
        found.add("seam_half")
    if two:
        found.add("chunks_odd" if k["chunks"] % 2 else "chunks_even")
    return found


def situations(k, case):
    """the same situations by arithmetic on the library's numbers (ConvWalk k) -- what the census uses; the schedule is consulted for the seams only"""
    n, h, _w, _ci, _co, pool, _keep, _dup, _cu = case
    found = set()
    G, total = k.workers, k.total
    if k.main == "wr":
        W, per = k.workers, k.per_group
        lens = [max(0, min(g * per + per, total) - g * per) for g in range(8)]
        most = max(_ceil(max(x - j, 0), W) for x in lens for j in range(W))      # items of the busiest worker while everything is static
        if per <= 5 * W and 2 <= most <= 5:
            found.add("static%d" % most)
        if W == 1 and min(lens) >= 8:
            found.add("claims")
        if total % 8 and per > W and any(0 < x < per for x in lens):
            found.add("uneven")
        if total < 8:
            found.add("empty")
        if per <= 5 * W or W == 1:
            counts = [x if W == 1 else _ceil(max(x - j, 0), W) for x in lens for j in range(W)]
            if {c & 1 for c in counts if c} == {0, 1}:
                found.add("sets")
        return found
    if k.main == "p_flat64":
        found.add("one_round")
        if k.tiles_n in (2, 4) and G % k.tiles_n == 0:
            found.add("slice%d_keep" % k.tiles_n)
        return found
    items = k.ht_full + 2 * k.ht_r
    q, r = divmod(items, G)
    if k.ht_r == 0 and r == 0 and q >= 3:
        found.add("rounds")
    if k.ht_r == 0 and q >= 1 and 2 * r > G:
        found.add("partial")
    if k.ht_r > 0 and _second_halves_live(k._asdict(), case):
        found.add("tail" if k.ht_full > 0 else "halves")
    if items > G and (G < 8 or G % 8):
        found.add("deal_lt8" if G < 8 else "deal_rem")
    if k.tiles_n in (2, 4) and q >= 2:
        if k.ht_r:                                   # half items: a tail tile's index is not its item's, so ask the schedule
            found |= _slice_situations(k._asdict(), schedule_p(k._asdict()))
        else:
            if G % k.tiles_n == 0:
                found.add("slice%d_keep" % k.tiles_n)
            if G % 2:
                found.add("slice%d_change" % k.tiles_n)
    if k.stacked and k.ht_r and any(_tile_spans_images(k._asdict(), case, t) for t in range(k.ht_full, k.ht_full + k.ht_r)):
        found.add("seam_half")
    if q >= 2:
        found.add("chunks_odd" if k.chunks % 2 else "chunks_even")
        if n == 3:
            kd = k._asdict()
            later = [t for v in schedule_p(kd) for t, _ in v[1:]]
            if k.main == "p_flat":
                if any(_tile_spans_images(kd, case, t) for t in later):
                    found.add("seam_flat")
            elif pool:
                found.add("seam_pooled")
            elif k.stacked:
                if any(_tile_spans_images(kd, case, t) for t in later):
                    found.add("seam_stacked")
            elif h < 16 and any(t // (k.tiles_x * k.tiles_y * k.tiles_n) >= 1 for t in later):
                found.add("seam_per_image")
    return found


def one_item_per_worker(k):
    """no workgroup of this launch starts a second item: the walk the cells of tests/conv_form_cases.py pin"""
    return k.per_group <= k.workers if k.main == "wr" else k.ht_full + 2 * k.ht_r <= k.workers


def reference_cu(prec, case, device_cu):
    """the cu_count of the launch a case's bytes are compared with: 0 (the device's own) where that keeps the main form and gives every item a
    worker of its own, else the nearest override below the device's count that does -- or, where the form is taken at the smallest counts only,
    the smallest count (whole tiles on one worker each). A count whose launch is the case's own (the anchors: all halves on as many workers)
    compares a launch with itself and is taken only when no other count qualifies; None if none does"""
    own = walk_of(prec, case)
    same = None
    for cu in list(range(device_cu, case[8], -1)) + list(range(1, case[8])):
        k = walk_of(prec, case, cu)
        if k.main == own.main and one_item_per_worker(k):
            if k != own:
                return 0 if cu == device_cu else cu
            same = cu if same is None else same
    return same


# ---------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------
def _cost(case):
    n, h, w, ci, co = case[:5]
    return (n * h * w * ci * co, n * h * w, case)


def _offer(found, cell, case):
    if cell not in found or _cost(case) < _cost(found[cell]):
        found[cell] = case


def census(precs=PRECS):
    """{cell: case} over GRID at the overridden CU counts GRID_CU: persistent forms and wr; the fused conv1_1 form takes wr's pooled Co = 64 walk"""
    names, found = main_names(), {}
    w0, wn = GRID_W[0], GRID_W[-1] - GRID_W[0] + 1
    for prec in precs:
        chans = GRID_CH + (GRID_CH_FP32 if prec == "fp32" else ())
        for ci, co in chans:
            if prec == "split" and co > 64 and co % 128:
                continue
            for pool, keep in GRID_POOL:
                for n in GRID_N:
                    for h in GRID_H:
                        if pool and h < 2:
                            continue
                        for cu in GRID_CU:
                            rows = B.conv3x3_walk_sweep(prec, n, h, w0, wn, ci, co, pool, keep or not pool, False, cu_count=cu)
                            for w in GRID_W:
                                row = [int(v) for v in rows[w - w0]]
                                form = names[row[0]]
                                if form != "wr" and form not in P_FORMS:
                                    continue
                                k = B.ConvWalk(form, *row[1:])
                                if k.ht_full + 2 * k.ht_r > MAX_ITEMS or k.total > MAX_ITEMS:
                                    continue
                                case = (n, h, w, ci, co, int(pool), int(keep and pool), 0, cu)
                                mode = ("pool+full" if keep else "pool") if pool else "full"
                                for s in situations(k, case):
                                    if form == "wr":
                                        _offer(found, "%s/wr/%s/co%d/%s" % (prec, mode, co, s), case)
                                        if pool and not keep and co == 64 and h >= 16:      # ctpn_debug_conv1_fused: n x h x w images, 16 pixels at least
                                            _offer(found, "%s/wr_fused/pool/co64/%s" % (prec, s), case)
                                    else:
                                        _offer(found, "%s/%s/%s" % (prec, form, s), case)
    return found


def device_census(cu=CU, precs=PRECS):
    """{cell: case with cu_count 0}: per precision and persistent form the cheapest shape with two or more rounds on `cu` CUs (Ci <= 128, 64 for
    p64; at most 2^18 output pixels), and one wr `claims` case per 16-bit mode at Co = 128 with per_group > 80"""
    names, found = main_names(), {}
    for prec in precs:
        chans = ((64, 64), (64, 128), (128, 128), (64, 256), (64, 512)) + (((32, 128), (32, 512)) if prec == "fp32" else ())
        for ci, co in chans:
            for pool, keep in GRID_POOL:
                for n in (1, 2, 3):
                    for h in (16, 24, 32, 40, 48, 64, 96):
                        rows = B.conv3x3_walk_sweep(prec, n, h, 16, 1024 - 15, ci, co, pool, keep or not pool, False, cu_count=cu)
                        for w in range(16, 1025, 16):
                            row = [int(v) for v in rows[w - 16]]
                            form = names[row[0]]
                            if form not in P_FORMS or n * h * w > 1 << 18 or (form == "p64" and ci > 64):
                                continue
                            k = B.ConvWalk(form, *row[1:])
                            if k.ht_full + 2 * k.ht_r > k.workers:
                                _offer(found, "%s/%s/two_rounds" % (prec, form), (n, h, w, ci, co, int(pool), int(keep and pool), 0, 0))
    for prec in ("bf16", "fp16"):
        case = (1, 168, 1024, 64, 128, 0, 0, 0, 0)
        k = walk_of(prec, case, cu)
        assert k.main == "wr" and k.per_group > 80 and k.per_group > 5 * k.workers
        found["%s/wr/full/co128/claims_device" % prec] = case
    return found


# ---------------------------------------------------------------------------------------------------------------
# the exact recipe: integer data whose sums are exact in fp32 in any order
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def exact_problem(prec, n, h, w, ci, co):
    """(x, weights, bias, expected full map, expected pooled map) as float32: inputs 0 .. 3, weights -2 .. 2, integer bias; every partial sum is an
    integer below 9 * 128 * 6 + 4096 < 2^14, so fp32 accumulation is exact in any order and the stored value is the rounding of the exact one:
    fp32 and split precision (hi + lo spans 16 bits) the value itself, the 16-bit modes oracle/rounding.py of it. The sums of zero-mean weights
    stay near +-100, where bf16 and fp16 hold every integer: three channels of four carry a bias of 256 .. 4096, so that their values need the
    rounding (bf16 above 256, fp16 above 2048) and the lo plane; every fourth channel has a bias of -64 .. 64 and meets the ReLU"""
    from oracle import network as N
    assert ci <= 128
    rng = np.random.default_rng(((n * 137 + h) * 1031 + w) * 13 + ci + 3 * co)
    x = rng.integers(0, 4, (n, h, w, ci)).astype(np.float32)
    wt = rng.integers(-2, 3, (3, 3, ci, co)).astype(np.float32)
    b = np.where(np.arange(co) % 4 == 0, rng.integers(-64, 65, co), rng.integers(256, 4097, co)).astype(np.float32)
    ref = N.conv3x3_relu(x.astype(np.float64), wt.astype(np.float64), b.astype(np.float64))
    assert np.array_equal(ref, np.rint(ref)) and float(ref.max()) < 2 ** 14
    ref32 = ref.astype(np.float32)
    want = {"bf16": bf16_round, "fp16": fp16_round}.get(prec, lambda a: a)(ref32)
    pooled = N.maxpool2x2(want) if h >= 2 and w >= 2 else np.zeros((n, h // 2, w // 2, co), np.float32)
    for a in (x, wt, b, want, pooled):
        a.setflags(write=False)
    return x, wt, b, want, pooled


def judge_bits(what, got, want):
    """bit for bit; returns the number of values compared"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(axis=-1))
    assert bad.size == 0, (what, "%d pixels differ" % len(bad), bad[:4].tolist())
    return got.size


# ---------------------------------------------------------------------------------------------------------------
# the guarded map of ctpn_debug_conv3x3_walk, restated: what the hook checks after the launch
# ---------------------------------------------------------------------------------------------------------------
FILL, GUARD_ROWS = 0xC3, 64


def guarded_map(n, h, w, pix_bytes):
    """the hook's output buffer before the launch: [n (h + 2) + 64 guard rows][w + 2][pixel bytes] of the fill"""
    return np.full((n * (h + 2) + GUARD_ROWS, w + 2, pix_bytes), FILL, np.uint8)


def guarded_map_violation(buf, n, h):
    """None, or (image, bordered row) of the first border pixel that no longer holds the fill; ("guard", row) for a guard row"""
    for img in range(n):
        for y in range(h + 2):
            r = buf[img * (h + 2) + y]
            if not ((r == FILL).all() if y in (0, h + 1) else ((r[0] == FILL).all() and (r[-1] == FILL).all())):
                return img, y
    g = np.argwhere((buf[n * (h + 2):] != FILL).any(axis=(1, 2)))
    return ("guard", int(g[0, 0])) if g.size else None


if __name__ == "__main__":
    cells, dev = census(), device_census()
    print('"""Generated by `python tests/conv_walks.py`: walk cell -> (n, h, w, ci, co, pool, want_full, dup_hi, cu_count), the cheapest shape of the\n'
          'census (tests/conv_walks.py) that reaches the cell. %d cells at an overridden CU count, %d at the device\'s own (cu_count 0; generated for %d CUs)."""'
          % (len(cells), len(dev), CU))
    for name, table in (("CASES", cells), ("DEVICE_CASES", dev)):
        print("%s = {" % name)
        for cell in sorted(table):
            print("    %r: %r," % (cell, tuple(int(v) for v in table[cell])))
        print("}")
