"""Spark commitments and openings (development aid, outside bench.py): shapes (num_vars, dim_vars, num_dims) over
multilinear KZG in ONE process on one ctx, uniform random indices and full-width random values.  Per shape: the commit
(timed once, after an untimed one), then one untimed opening and --proofs timed ones of ONE handle, each at a fresh random
point; a time is the host's wall clock around the call with the stream drained before and after, and EVERY timed proof is
verified on the host.  A profiled opening follows (per-kernel records, summed by name; the split between MSM, sum-check
rounds and Spark's own kernels is read from it).  One JSON line per shape is appended to --out
(profiles/spark_bench.jsonl).

    timeout -k 10 900 python tools/spark_bench.py [--shapes 20:16:2 20:20:2 24:16:2] [--proofs 5]
"""
import argparse
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


def random_fr_bytes(rng, count):
    """`count` field elements as device bytes: any 256-bit word below the modulus is some element's Montgomery form"""
    limbs = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    limbs[:, 3] >>= 4  # below 2^252 < r
    return limbs.tobytes()


def by_name(recs):
    out = {}
    for r in recs:
        e = out.setdefault(r["name"], {"launches": 0, "ms": 0.0, "bytes": 0.0})
        e["launches"] += 1
        e["ms"] = round(e["ms"] + r["ms"], 4)
        e["bytes"] += r["bytes"]
    return out


def split(kernels):
    """the profiled opening's time by kind: MSM batches, sum-check rounds and binds, Spark's own kernels, everything else"""
    kinds = {"msm": 0.0, "rounds": 0.0, "trees": 0.0, "spark": 0.0, "other": 0.0}
    for name, e in kernels.items():
        kind = "msm" if name.startswith("msm_") else "spark" if name.startswith("spark_") else \
            "trees" if name.startswith("tree_") else "rounds" if name.startswith(("sc_", "gkr_", "fix_var")) else "other"
        kinds[kind] = round(kinds[kind] + e["ms"], 3)
    return kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20:16:2", "20:20:2", "24:16:2"])
    ap.add_argument("--proofs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spark_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=800, help="seconds for the whole run: the process ends there")
    args = ap.parse_args()

    def expired(signum, frame):
        sys.stderr.write("exceeded the %d s limit\n" % args.limit)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)

    ctx = hl.Context(0)
    for text in args.shapes:
        n, l, c = [int(v) for v in text.split(":")]
        rng = np.random.default_rng(1000 * n + 10 * l + c)
        ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
        pp = hl.MultilinearKzg.setup(ctx, ss)
        vp = hl.MultilinearKzgVerifierParams.setup(ss)
        dims = [hl.U32Column(ctx.upload(rng.integers(0, 1 << l, size=1 << n, dtype=np.uint32).tobytes()), n) for _ in range(c)]
        val = hl.MultilinearPolynomial(ctx, ctx.upload(random_fr_bytes(rng, 1 << n)), n)

        def commit():
            ctx.sync()
            t = time.perf_counter()
            poly = hl.spark_commit(ctx, pp, dims, val, l)
            ctx.sync()
            return (time.perf_counter() - t) * 1e3, poly

        _, poly = commit()
        poly.free()
        commit_ms, poly = commit()

        def open_once():
            point = [int(v) for v in rng.integers(1, 1 << 62, size=c * l)]
            ctx.sync()
            t = time.perf_counter()
            value, proof = hl.spark_open(ctx, pp, poly, point)
            ctx.sync()
            return (time.perf_counter() - t) * 1e3, point, value, proof

        ms, verify_ms, sizes = [], [], set()
        for rep in range(args.proofs + 1):
            dt, point, value, proof = open_once()
            sizes.add(len(proof))
            if rep:  # (the first opening is untimed)
                ms.append(round(dt, 3))
                t = time.perf_counter()
                hl.spark_verify(vp, n, l, c, poly.commitment, point, value, proof)  # (raises unless valid)
                verify_ms.append((time.perf_counter() - t) * 1e3)
        hl.profile_enable(ctx, True)
        try:
            open_once()
            kernels = by_name(hl.profile_read(ctx))
        finally:
            hl.profile_enable(ctx, False)
        own = {k: dict(v, gb_per_s=round(v["bytes"] / v["ms"] / 1e6, 1) if v["ms"] else None)
               for k, v in kernels.items() if k.startswith("spark_")}
        rec = dict(shape=dict(num_vars=n, dim_vars=l, num_dims=c), pcs="mkzg", commit_ms=round(commit_ms, 3),
                   commitment_bytes=len(poly.commitment), proofs=args.proofs, proof_bytes=sorted(sizes), ms=ms,
                   ms_median=round(statistics.median(ms), 3), spread_ms=round(max(ms) - min(ms), 3),
                   host_verify_ms_median=round(statistics.median(verify_ms), 1), spark_kernels=own,
                   profiled_split_ms=split(kernels), kernels=kernels)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        poly.free()
        del dims, val
        pp.free()


if __name__ == "__main__":
    main()
