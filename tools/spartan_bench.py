"""Spartan keys and proofs (development aid, outside bench.py): shapes (num_vars, dim_vars) over multilinear KZG in ONE process
on one ctx, full-width random values, three public inputs.  Per shape two instances: `uniform` - uniform random positions in
A and B - and `skewed` - every other entry of B in the constant column (index 2^(dim_vars-1)), the column that in a real
circuit may hold every entry of a matrix.  The instance is made satisfiable on the device: a first key with C = 0 gives Az
and Bz through the keyed-sum entry, and C gets the entry (i, constant column, (Az)[i] (Bz)[i]) for every row i (so
2^num_vars >= 2^dim_vars), zeros elsewhere.  Per instance: the key (timed once, after an untimed one), one untimed proof and
--proofs timed ones of ONE key; a time is the host's wall clock around the call with the stream drained before and after, and
EVERY timed proof is verified on the host.  A profiled proof follows (per-kernel records, summed by name, and split into
MSM / rounds / Spark's kernels / spartan_spmv / other; the share of the three Spark openings is read between the first
spark_e record and the end).  One JSON line per instance is appended to --out (profiles/spartan_bench.jsonl).

    timeout -k 10 900 python tools/spartan_bench.py [--shapes 20:16 20:20 24:20] [--proofs 5]
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

PUBLIC = 3


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
    kinds = {"msm": 0.0, "rounds": 0.0, "spark": 0.0, "spartan_spmv": 0.0, "other": 0.0}
    for name, e in kernels.items():
        kind = "msm" if name.startswith("msm_") else "spark" if name.startswith("spark_") else \
            "spartan_spmv" if name == "spartan_spmv" else "rounds" if name.startswith(("sc_", "gkr_", "fix_var")) else "other"
        kinds[kind] = round(kinds[kind] + e["ms"], 3)
    return kinds


def fr_ptr(buf):
    return C.cast(C.c_void_p(buf.ptr), C.POINTER(hl.lh_fr))


def instance(ctx, pp, rng, n, l, skewed, x):
    """-> (matrices, d_w): device columns of a satisfiable instance"""
    N, M, half = 1 << n, 1 << l, 1 << (l - 1)
    assert N >= M, "one entry of C per row"
    col = lambda a: hl.U32Column(ctx.upload(a.astype(np.uint32).tobytes()), n)
    fr = lambda data, nv: hl.MultilinearPolynomial(ctx, ctx.upload(data), nv)
    b_col = rng.integers(0, M, size=N, dtype=np.uint32)
    if skewed:
        b_col[1::2] = half
    A = (col(rng.integers(0, M, size=N)), col(rng.integers(0, M, size=N)), fr(random_fr_bytes(rng, N), n))
    B = (col(rng.integers(0, M, size=N)), col(b_col), fr(random_fr_bytes(rng, N), n))
    rows = np.concatenate([np.arange(M, dtype=np.uint32), rng.integers(0, M, size=N - M, dtype=np.uint32)])
    cols = np.concatenate([np.full(M, half, dtype=np.uint32), rng.integers(0, M, size=N - M, dtype=np.uint32)])
    c_val = ctx.upload(bytes(32 * N))
    Cm = (col(rows), col(cols), hl.MultilinearPolynomial(ctx, c_val, n))
    w_bytes = random_fr_bytes(rng, half)
    d_w = fr(w_bytes, l - 1)
    # z = (w, x, 0) on the device, Az and Bz by the keyed sum of a first key (C = 0), their product into C's first M values
    z = ctx.upload(bytes(32 * M))
    z.write(w_bytes, 0)
    z.write(hl.frs_to_bytes(x), 32 * half)
    outs = [ctx.alloc(32 * M) for _ in range(3)]
    with hl.r1cs_commit(ctx, pp, [A, B, Cm], l) as key:
        hl._check(ctx.lib.lh_debug_spartan_spmv(ctx.h, key.h, 0, fr_ptr(z), C.cast(hl._ptr_array(outs), C.POINTER(C.POINTER(hl.lh_fr)))))
    hl._check(ctx.lib.lh_fr_mul(ctx.h, fr_ptr(outs[0]), fr_ptr(outs[1]), M, fr_ptr(c_val)))
    ctx.sync()
    for b in outs + [z]:
        b.free()
    return [A, B, Cm], d_w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20:16", "20:20", "24:20"])
    ap.add_argument("--proofs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spartan_bench.jsonl"))
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
        rng = np.random.default_rng(1000 * n + 10 * l)
        ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
        pp = hl.MultilinearKzg.setup(ctx, ss)
        vp = hl.MultilinearKzgVerifierParams.setup(ss)
        x = [1] + [int(v) for v in rng.integers(1, 1 << 62, size=PUBLIC - 1)]
        for skewed in (False, True):
            mats, d_w = instance(ctx, pp, rng, n, l, skewed, x)

            def commit():
                ctx.sync()
                t = time.perf_counter()
                key = hl.r1cs_commit(ctx, pp, mats, l)
                ctx.sync()
                return (time.perf_counter() - t) * 1e3, key

            _, key = commit()
            key.free()
            key_ms, key = commit()

            def prove_once():
                ctx.sync()
                t = time.perf_counter()
                proof = hl.spartan_prove(ctx, pp, key, d_w, x)
                ctx.sync()
                return (time.perf_counter() - t) * 1e3, proof

            ms, verify_ms, sizes = [], [], set()
            for rep in range(args.proofs + 1):
                dt, proof = prove_once()
                sizes.add(len(proof))
                if rep:  # (the first proof is untimed)
                    ms.append(round(dt, 3))
                    t = time.perf_counter()
                    hl.spartan_verify(vp, n, l, key.commitment, x, proof)  # (raises unless valid)
                    verify_ms.append((time.perf_counter() - t) * 1e3)
            hl.profile_enable(ctx, True)
            try:
                prove_once()
                recs = hl.profile_read(ctx)
            finally:
                hl.profile_enable(ctx, False)
            kernels = by_name(recs)
            first_e = next(i for i, r in enumerate(recs) if r["name"] == "spark_e")
            total = sum(r["ms"] for r in recs)
            openings = sum(r["ms"] for r in recs[first_e - 2:])  # (from the two eq tables of the first opening on)
            rate = lambda r: dict(ms=round(r["ms"], 4), bytes=r["bytes"], gb_per_s=round(r["bytes"] / r["ms"] / 1e6, 1))
            spmv = [rate(r) for r in recs if r["name"] == "spartan_spmv"]
            spark_e = [rate(r) for r in recs if r["name"] == "spark_e"]
            rec = dict(shape=dict(num_vars=n, dim_vars=l, num_public=PUBLIC), positions="skewed" if skewed else "uniform",
                       pcs="mkzg", key_ms=round(key_ms, 3), key_bytes=len(key.commitment), proofs=args.proofs,
                       proof_bytes=sorted(sizes), ms=ms, ms_median=round(statistics.median(ms), 3),
                       spread_ms=round(max(ms) - min(ms), 3), host_verify_ms_median=round(statistics.median(verify_ms), 1),
                       spartan_spmv=dict(by_rows=spmv[0], by_columns=spmv[1]), spark_e=spark_e,
                       profiled_total_ms=round(total, 3), profiled_spark_openings_ms=round(openings, 3),
                       profiled_split_ms=split(kernels), kernels=kernels)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            key.free()
            del mats, d_w
        pp.free()


if __name__ == "__main__":
    main()
