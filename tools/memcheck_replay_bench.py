"""lh_memcheck_replay against the witness pass beside it (development aid, outside bench.py): shapes (num_vars, mem_vars)
with an image, in ONE process on one ctx, each with two traces - `uniform` (random cells) and `hot` (every operation on
cell 0: one segment over every tile, every carry passes through store-free tiles).  Per shape and trace: the replay
(lh_memcheck_replay) and, on the trace it produced, memcheck_trace through lh_debug_memcheck_witness - the same sort plus
one neighbour pass, the only measured yardstick for a pass over the sorted trace.  One untimed pass, then --reps timed
ones of each, alternating; a time is the launch record's (device events around the sort and the passes, the flag readback
included), the host's wall clock around the call is recorded beside it.  The replay's output is compared with a numpy
restatement once per trace.  With --prove SHAPE a segment proof and a plain proof of the same uniform trace are timed in
the manner of tools/memcheck_bench.py (both verified).  One JSON line per shape and trace is appended to --out
(profiles/memcheck_replay_bench.jsonl).

    timeout -k 10 600 python tools/memcheck_replay_bench.py [--shapes 20:16 24:20] [--reps 7] [--prove 20:16]
"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_lasso_amd as hl  # noqa: E402
import numpy as np  # noqa: E402


def make_ops(rng, n, l, kind):
    N = 1 << n
    addr = np.zeros(N, dtype=np.uint32) if kind == "hot" else rng.integers(0, 1 << l, size=N, dtype=np.uint32)
    store = (rng.integers(0, 3, size=N) > 0).astype(np.uint32)
    val = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    return addr, store, val


def restate(addr, store, val, image):
    """rv, wv, final without a loop over the operations (tools/memcheck_bench.py make_trace)"""
    N = len(addr)
    order = np.argsort(addr, kind="stable")
    sa, k = addr[order], np.arange(N)
    first = np.concatenate(([True], sa[1:] != sa[:-1]))
    start = np.maximum.accumulate(np.where(first, k, 0))
    src = np.maximum.accumulate(np.where(store[order] != 0, k, -1))
    wv_s = np.where(src >= start, val[order][np.maximum(src, 0)], image[sa]).astype(np.uint32)
    rv_s = np.where(k > start, np.concatenate(([0], wv_s[:-1])), image[sa]).astype(np.uint32)
    rv, wv = np.empty(N, dtype=np.uint32), np.empty(N, dtype=np.uint32)
    rv[order], wv[order] = rv_s, wv_s
    final = image.copy()
    last = np.concatenate((sa[1:] != sa[:-1], [True]))
    final[sa[last]] = wv_s[last]
    return rv, wv, final


def timed(ctx, name, fn):
    """-> (launch record ms summed over `name`, wall ms, bytes of the record)"""
    hl.profile_enable(ctx, True)
    try:
        ctx.sync()
        t = time.perf_counter()
        fn()
        ctx.sync()
        wall = (time.perf_counter() - t) * 1e3
        recs = [r for r in hl.profile_read(ctx) if r["name"] == name]
    finally:
        hl.profile_enable(ctx, False)
    return sum(r["ms"] for r in recs), wall, sum(r["bytes"] for r in recs)


def witness_call(ctx, trace, n, l, init):
    """lh_debug_memcheck_witness on device buffers kept for all calls (hl.memcheck_witness would download four columns)
    -> a function that runs it and returns `bad`"""
    t = hl._ffi.lh_memcheck_trace()
    t.d_addr, t.d_rv, t.d_wv = [C.cast(C.c_void_p(c.ptr), C.POINTER(C.c_uint32)) for c in trace]
    bufs = [ctx.alloc(s) for s in (4 << n, 4 << l, 4 << l, 4 << n)]

    def run():
        bad = C.c_int(0)
        hl._check(ctx.lib.lh_debug_memcheck_witness(ctx.h, C.byref(t), n, l, init, *[b.ptr for b in bufs], C.byref(bad)))
        return bad.value
    return run


def med(xs):
    return round(statistics.median(xs), 4)


def prove_pair(ctx, n, l, cols, image_dev, image_host, reps):
    rng = np.random.default_rng(77 * n + l)
    ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
    pp = hl.MultilinearKzg.setup(ctx, ss)
    vp = hl.MultilinearKzgVerifierParams.setup(ss)
    init = (C.c_uint32 * len(image_host)).from_buffer_copy(image_host.tobytes())
    out = {}
    for which in ("plain", "segment"):
        ms = []
        for rep in range(reps + 1):
            tr = hl.Keccak256Transcript()
            ctx.sync()
            t = time.perf_counter()
            if which == "plain":
                hl.memcheck_prove(pp, *cols, l, tr, init=init)
            else:
                hl.memcheck_prove_segment(pp, *cols, l, image_dev, tr)
            ctx.sync()
            dt = (time.perf_counter() - t) * 1e3
            proof = tr.into_proof()
            if rep:
                ms.append(round(dt, 3))
        if which == "plain":
            hl.memcheck_verify(vp, n, l, hl.Keccak256Transcript.from_proof(proof), init=init)
        else:
            hl.memcheck_verify_segment(vp, n, l, hl.Keccak256Transcript.from_proof(proof))
        out[which] = dict(ms=ms, ms_median=med(ms), proof_bytes=len(proof))
    out["segment_minus_plain_ms"] = round(out["segment"]["ms_median"] - out["plain"]["ms_median"], 3)
    pp.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20:16", "24:20"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prove", nargs="*", default=[], help="shapes at which a segment proof is timed against a plain one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memcheck_replay_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=550, help="seconds for the whole run: the process ends there")
    args = ap.parse_args()

    def expired(signum, frame):
        sys.stderr.write("exceeded the %d s limit\n" % args.limit)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)

    ctx = hl.Context(0)
    for text in args.shapes:
        n, l = [int(v) for v in text.split(":")]
        rng = np.random.default_rng(1000 * n + l)
        image_host = rng.integers(0, 1 << 32, size=1 << l, dtype=np.uint64).astype(np.uint32)
        image = hl.U32Column(ctx.upload(image_host.tobytes()), l)
        init = (C.c_uint32 * len(image_host)).from_buffer_copy(image_host.tobytes())
        for kind in ("uniform", "hot"):
            ops = make_ops(rng, n, l, kind)
            cols = [hl.U32Column(ctx.upload(c.tobytes()), n) for c in ops]
            rv, wv, final = hl.memcheck_replay(ctx, *cols, l, image=image)  # (the untimed pass; checked once)
            want = restate(*ops, image_host)
            for got, w, what in zip((rv, wv, final), want, ("rv", "wv", "final")):
                assert np.array_equal(np.frombuffer(got.buf.read(), dtype=np.uint32), w), what
            trace = (cols[0], rv, wv)
            witness = witness_call(ctx, trace, n, l, init)
            assert not witness(), "the replayed trace is not consistent"
            replay_ms, replay_wall, trace_ms, trace_wall = [], [], [], []
            for rep in range(args.reps):
                ms, wall, replay_bytes = timed(ctx, "memcheck_replay", lambda: hl.memcheck_replay(ctx, *cols, l, image=image))
                replay_ms.append(ms), replay_wall.append(wall)
                # (the debug entry also counts the multiplicities: the record's time is the sort and the pass alone)
                ms, wall, trace_bytes = timed(ctx, "memcheck_trace", witness)
                trace_ms.append(ms), trace_wall.append(wall)
            r, t = med(replay_ms), med(trace_ms)
            rec = dict(shape=dict(num_vars=n, mem_vars=l), trace=kind, reps=args.reps,
                       replay_ms=[round(v, 4) for v in replay_ms], replay_ms_median=r, replay_wall_ms_median=med(replay_wall),
                       trace_ms=[round(v, 4) for v in trace_ms], trace_ms_median=t, replay_over_trace=round(r / t, 3),
                       replay_bytes=replay_bytes, replay_gb_per_s=round(replay_bytes / r / 1e6, 1),
                       trace_bytes=trace_bytes, trace_gb_per_s=round(trace_bytes / t / 1e6, 1))
            if kind == "uniform" and text in args.prove:
                rec["proofs"] = prove_pair(ctx, n, l, trace, image, image_host, 3)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            del cols, rv, wv, final, trace, witness


if __name__ == "__main__":
    main()
