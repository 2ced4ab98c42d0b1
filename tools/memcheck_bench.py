"""Read-write memory-checking proofs (development aid, outside bench.py): shapes (num_vars, mem_vars) over multilinear
KZG with an initial image, in ONE process on one ctx, each with two traces - the extremes of the histogram of time
differences: `uniform` (random cells) and `hot` (every operation on cell 0: every difference is 0).  One untimed pass, then
--proofs timed proofs per trace; a proof's time is the host's wall clock around lh_memcheck_prove with the stream drained
before and after, and EVERY timed proof is verified on the host.  A profiled pass follows (per-kernel records, summed by
name).  One JSON line per shape and trace is appended to --out (profiles/memcheck_bench.jsonl).

    timeout -k 10 900 python tools/memcheck_bench.py [--shapes 20:16 24:20] [--proofs 5]
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


def make_trace(rng, n, l, kind, init):
    """a consistent trace without a loop over the operations: two in three are stores, a load repeats the cell's value"""
    N = 1 << n
    addr = np.zeros(N, dtype=np.uint32) if kind == "hot" else rng.integers(0, 1 << l, size=N, dtype=np.uint32)
    store = rng.integers(0, 3, size=N) > 0
    words = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    order = np.argsort(addr, kind="stable")
    sa, k = addr[order], np.arange(N)
    start = np.maximum.accumulate(np.where(np.concatenate(([True], sa[1:] != sa[:-1])), k, 0))  # first position of the run
    src = np.maximum.accumulate(np.where(store[order], k, -1))  # the latest store at or before k, in sorted order
    wv_s = np.where(src >= start, words[order][np.maximum(src, 0)], init[sa])
    rv_s = np.where(k > start, np.concatenate(([0], wv_s[:-1])), init[sa]).astype(np.uint32)
    rv, wv = np.empty(N, dtype=np.uint32), np.empty(N, dtype=np.uint32)
    rv[order], wv[order] = rv_s, wv_s
    return addr, rv, wv


def by_name(recs):
    out = {}
    for r in recs:
        e = out.setdefault(r["name"], {"launches": 0, "ms": 0.0, "bytes": 0.0})
        e["launches"] += 1
        e["ms"] = round(e["ms"] + r["ms"], 4)
        e["bytes"] += r["bytes"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20:16", "24:20"])
    ap.add_argument("--proofs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memcheck_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=800, help="seconds for the whole run: the process ends there")
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
        ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
        pp = hl.MultilinearKzg.setup(ctx, ss)
        vp = hl.MultilinearKzgVerifierParams.setup(ss)
        init = rng.integers(0, 1 << 32, size=1 << l, dtype=np.uint64).astype(np.uint32)
        image = (C.c_uint32 * len(init)).from_buffer_copy(init.tobytes())  # (marshalled once, outside the timed calls)
        for kind in ("uniform", "hot"):
            cols = [hl.U32Column(ctx.upload(c.tobytes()), n) for c in make_trace(rng, n, l, kind, init)]

            def prove():
                tr = hl.Keccak256Transcript()
                ctx.sync()
                t = time.perf_counter()
                hl.memcheck_prove(pp, *cols, l, tr, init=image)
                ctx.sync()
                return (time.perf_counter() - t) * 1e3, tr.into_proof()

            def verify(proof):
                t = time.perf_counter()
                hl.memcheck_verify(vp, n, l, hl.Keccak256Transcript.from_proof(proof), init=image)  # (raises unless valid)
                return (time.perf_counter() - t) * 1e3

            ms, verify_ms, proofs = [], [], set()
            for rep in range(args.proofs + 1):
                dt, proof = prove()
                proofs.add(proof)
                if rep:  # (the first pass is untimed)
                    ms.append(round(dt, 3))
                    verify_ms.append(verify(proof))
            assert len(proofs) == 1, "two proofs of one trace differ"
            hl.profile_enable(ctx, True)
            try:
                prove()
                kernels = by_name(hl.profile_read(ctx))
            finally:
                hl.profile_enable(ctx, False)
            rec = dict(shape=dict(num_vars=n, mem_vars=l), trace=kind, pcs="mkzg", proofs=args.proofs,
                       proof_bytes=len(next(iter(proofs))), ms=ms, ms_median=round(statistics.median(ms), 3),
                       spread_ms=round(max(ms) - min(ms), 3), host_verify_ms_median=round(statistics.median(verify_ms), 1),
                       memcheck_kernels={k: v for k, v in kernels.items() if k.startswith("memcheck_")}, kernels=kernels)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            del cols
        pp.free()


if __name__ == "__main__":
    main()
