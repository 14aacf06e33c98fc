#!/usr/bin/env python
"""Where the machine stands idle, and which kernels of two forwards run side by side, out of a rocprofv3 kernel trace (CSV) of a few
pipelined bench steps:  rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python bench.py --steps 8 --warmup 3 --stage-events off
usage: overlap_timeline.py DIR/.../trace_kernel_trace.csv [first_step [steps [--timeline]]]

A step starts at an image_to_q launch (the uint8 feed of the 16-bit modes). Over `steps` steps from `first_step` it prints, per step: the span,
the time no kernel was running, the time kernels of two different forward queues were running together, the time a conv3x3 main kernel was
running; per hardware queue: the kernels that ran on it; per kernel name: launches per step, mean duration, and how much of it passed beside
a kernel of ANOTHER forward queue. --timeline adds one step's dispatches in start order."""
import collections
import csv
import sys

FORWARD = ("image_to_q", "conv_first", "conv3x3", "lstm_pre", "bilstm", "igemm", "ragged")


def short(name):
    name = name.replace("ctpn::", "").replace("void ", "")
    return name[:name.index("(")][:64] if "(" in name else name[:64]


def union_len(iv):
    tot, end = 0, None
    for a, b in sorted(iv):
        if end is None or a > end:
            tot += b - a
            end = b
        elif b > end:
            tot += b - end
            end = b
    return tot


def intersect(xs, ys):
    """intervals where both sorted, merged lists are busy"""
    out, i, j = [], 0, 0
    while i < len(xs) and j < len(ys):
        a, b = max(xs[i][0], ys[j][0]), min(xs[i][1], ys[j][1])
        if a < b:
            out.append((a, b))
        if xs[i][1] < ys[j][1]:
            i += 1
        else:
            j += 1
    return out


def merged(iv):
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def main(path, first=3, steps=4, timeline=False):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], short(r["Kernel_Name"]),
                         int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 0)) or 0), int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)))
    rows.sort()
    starts = [r[0] for r in rows if "image_to_q" in r[3]]
    if len(starts) < first + steps + 1:
        raise SystemExit("only %d steps in the trace" % len(starts))
    t0, t1 = starts[first], starts[first + steps]
    win = [r for r in rows if t0 <= r[0] < t1]
    fq = collections.Counter(r[2] for r in win if "conv3x3" in r[3] and "edge" not in r[3])
    fwd_queues = sorted(fq)
    print("window: steps %d .. %d, %.1f us per step, %d dispatches per step" % (first, first + steps - 1, (t1 - t0) / 1e3 / steps, len(win) / steps))
    print("queues that ran conv3x3 main kernels:", dict(fq))
    busy = merged((r[0], min(r[1], t1)) for r in win)
    print("no kernel running:               %8.1f us per step" % ((t1 - t0 - union_len(busy)) / 1e3 / steps))
    per_q = {q: merged((r[0], min(r[1], t1)) for r in win if r[2] == q and any(k in r[3] for k in FORWARD)) for q in fwd_queues}
    both = []
    for i, q in enumerate(fwd_queues):
        for p in fwd_queues[i + 1:]:
            both += intersect(per_q[q], per_q[p])
    both = merged(both)
    print("two forward queues running:      %8.1f us per step" % (union_len(both) / 1e3 / steps))
    conv = merged((r[0], min(r[1], t1)) for r in win if "conv3x3" in r[3] and "edge" not in r[3])
    print("a conv3x3 main kernel running:   %8.1f us per step" % (union_len(conv) / 1e3 / steps))
    gaps = [(b[0] - a[1]) / 1e3 for a, b in zip(busy, busy[1:])]
    print("idle gaps: %d per step, the ten longest (us): %s" % (len(gaps) / steps, " ".join("%.1f" % g for g in sorted(gaps)[-10:])))
    print()
    print("per queue:")
    for q in sorted({r[2] for r in win}):
        names = collections.Counter(r[3] for r in win if r[2] == q)
        print("  q=%s busy %.1f us per step: %s" % (q, union_len([(r[0], r[1]) for r in win if r[2] == q]) / 1e3 / steps,
                                                   ", ".join("%s x%d" % (n[:28], c) for n, c in names.most_common(8))))
    print()
    print("per kernel (launches per step, mean us, us per step, share of its time beside a kernel of another forward queue):")
    by = collections.defaultdict(list)
    for r in win:
        by[r[3]].append(r)
    for name, rs in sorted(by.items(), key=lambda kv: -sum(r[1] - r[0] for r in kv[1])):
        tot = sum(r[1] - r[0] for r in rs)
        beside = 0
        for r in rs:
            if r[2] in per_q:
                for q in fwd_queues:
                    if q != r[2]:
                        beside += union_len(intersect([(r[0], r[1])], per_q[q]))
        print("  %-64s %5.1f %8.1f %8.1f  %3.0f %%" % (name, len(rs) / steps, tot / 1e3 / len(rs), tot / 1e3 / steps, 100.0 * beside / max(tot, 1)))
    if timeline:
        a, b = starts[first + 1], starts[first + 2]
        print()
        print("one step in start order (start, end, us, queue, grid / workgroup, kernel); the other forward's kernels included:")
        for r in rows:
            if a <= r[0] < b:
                print("%9.1f %9.1f %8.1f  q=%s %8d/%-4d %s" % ((r[0] - a) / 1e3, (r[1] - a) / 1e3, (r[1] - r[0]) / 1e3, r[2], r[5], r[4], r[3]))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0], int(args[1]) if len(args) > 1 else 3, int(args[2]) if len(args) > 2 else 4, "--timeline" in sys.argv)
