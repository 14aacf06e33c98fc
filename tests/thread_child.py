"""One scenario of tests/thread_cases.py in a process of its own: python tests/thread_child.py NAME OUT.npz (started by
tests/test_gpu_threads.py; needs a GPU). A fresh process, because the process's first forward, first NMS and first decode are the contended
ones, and because a deadlock then ends in a killed child, not in a hung test session.

Builds every input on the main thread without touching the device, runs the scenario through thread_cases.run_together -- every worker creates
its ctx on its own thread -- and writes every (round, thread) result to OUT.npz (thread_cases.pack), with: texts_t<T>, the thread's
ctpn_last_error() text after each of its ops, for every worker that owns a ctx for the run; live_before / live_after,
ctpn_debug_live_resources in front of the threads and behind them; seconds, the wall time of run_together.
Exit code 0: no worker raised and no barrier broke; 1: a worker raised (the traceback is on stderr); 3: a broken barrier."""
import os
import sys
import time
import traceback

os.environ["CTPN_HOST_THREADS"] = "4"      # read by ctpn_create: up to five ctxs' worker pools stay within 16 CPUs

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import ctx_walks as W  # noqa: E402
import thread_cases as T  # noqa: E402


class CtxWorker:
    """owns a ctx of capacity CAP from start to stop"""

    def __init__(self, prec, directory, note_texts):
        self.prec, self.directory, self.ctx, self.texts = prec, directory, None, [] if note_texts else None

    def start(self):
        import ctpn_amd
        self.ctx = ctpn_amd.Context(0, *W.CAP, self.prec)
        self.ctx.load_weights(W.weights())

    def run(self, op):
        res = T.run_op(op, self.ctx, self.directory)
        if self.texts is not None:
            self.texts.append(T.last_error())
        return res

    def stop(self):
        if self.ctx is not None:
            self.ctx.close()


class FreeWorker:
    def __init__(self, directory):
        self.directory = directory

    def run(self, op):
        return T.run_op(op, None, self.directory)


class ChurnWorker:
    """every op on a ctx made for it: create -> load_weights -> op -> destroy"""

    def __init__(self, prec, directory):
        self.prec, self.directory = prec, directory

    def run(self, op):
        import ctpn_amd
        with ctpn_amd.Context(0, *W.CAP, self.prec) as ctx:
            ctx.load_weights(W.weights())
            return T.run_op(op, ctx, self.directory)


def make_worker(spec, directory):
    if spec.kind == "free":
        return FreeWorker(directory)
    if spec.kind == "churn":
        return ChurnWorker(spec.prec, directory)
    return CtxWorker(spec.prec, directory, spec.kind == "ctx")


def main(name, out):
    from ctpn_amd import _binding as B
    sc = T.SCENARIOS[name]
    directory = os.path.join(os.path.dirname(os.path.abspath(out)), "files_" + str(os.getpid()))
    ops = {op for row in sc.rounds for op in row if op is not None}
    W.inputs(), W.weights(), T.extra_inputs()
    if ops & set(T.FREE_OPS):
        T.free_inputs()
    if ops & set(T.CODEC_OPS):
        T.codec_inputs(), T.png_files(directory)
    B.load_library()
    workers = [make_worker(spec, directory) for spec in sc.workers]
    extra = {"live_before": np.array(B.live_resources(), np.int64)}
    t0 = time.perf_counter()
    try:
        results = T.run_together(workers, sc.rounds)
    except T.WorkerError:
        traceback.print_exc()
        return 1
    except T.BarrierBroken as e:
        print(e, file=sys.stderr, flush=True)
        os._exit(3)      # a thread may still sit in a call that never returns: no interpreter shutdown that would wait for it
    extra["seconds"] = np.array(time.perf_counter() - t0)
    extra["live_after"] = np.array(B.live_resources(), np.int64)
    for t, w in enumerate(workers):
        if getattr(w, "texts", None) is not None:
            extra["texts_t%d" % t] = np.array(w.texts)
    np.savez(out, **T.pack(results, extra))
    print("%s: %d results in %.2f s" % (name, len(results), float(extra["seconds"])))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in T.SCENARIOS:
        sys.exit("usage: thread_child.py NAME OUT.npz; NAME one of " + ", ".join(T.SCENARIOS))
    sys.exit(main(sys.argv[1], sys.argv[2]))
