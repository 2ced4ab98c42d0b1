"""Nova fold steps and relaxed Spartan proofs (development aid, outside bench.py): shapes (num_vars, dim_vars) over multilinear
KZG in ONE process on one ctx, full-width random values, three public inputs, `uniform` and `skewed` positions - the
instances of tools/spartan_bench.py, whose C is closed over ONE assignment (w, x).  The step that is timed is the usual one:
a running relaxed instance takes a fresh one.  The running instance is made on the device without a second satisfying
assignment: ANY (w', x') with the error vector E' = Az' o Bz' - x'[0] Cz' satisfies the relaxed relation, so w' is random,
E' comes from the keyed sum and the cross-term entry (mz2 = (0, Bz', 0), u2 = x'[0]), and its blob is put together from two
commitments; the cross term of the fold is then a full-width vector, as in a real chain.

Per instance, in one run: the fold step (median of --reps, spread, every fold verified on the host, a profiled one split into
MSM / nova_spmv2 / element-wise / other), the relaxed proof of the folded instance (verified), the host times of fold-verify
and relaxed verify, lh_spartan_prove of the same key and assignment, and the yardstick of nova_spmv2: per repetition the
profiled time of ONE nova_spmv2 launch set over (z1, z2) against TWO spartan_spmv launch sets over the same vectors, median
against median, with the spread of the two launches among their own repetitions.  One JSON line per instance is appended to
--out (profiles/nova_bench.jsonl).

    timeout -k 10 1100 python tools/nova_bench.py [--shapes 20:16 20:20 24:20] [--reps 5]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import halo2_lasso_amd as hl  # noqa: E402
import numpy as np  # noqa: E402
from spartan_bench import PUBLIC, by_name, fr_ptr, instance, random_fr_bytes  # noqa: E402


def split(kernels):
    kinds = {"msm": 0.0, "nova_spmv2": 0.0, "element_wise": 0.0, "other": 0.0}
    for name, e in kernels.items():
        kind = "msm" if name.startswith("msm_") else "nova_spmv2" if name == "nova_spmv2" else \
            "element_wise" if name in ("nova_cross_term", "nova_fold") else "other"
        kinds[kind] = round(kinds[kind] + e["ms"], 3)
    return kinds


def fr_pp(bufs):
    return C.cast(hl._ptr_array(bufs), C.POINTER(C.POINTER(hl.lh_fr)))


def be32(v):
    return int(v).to_bytes(32, "big")


def running_instance(ctx, pp, key, rng, l, x_run):
    """-> (blob, d_w, d_e, d_z): a relaxed instance with a random witness and the error vector that makes it hold"""
    M, half = 1 << l, 1 << (l - 1)
    w_bytes = random_fr_bytes(rng, half)
    d_w = hl.MultilinearPolynomial(ctx, ctx.upload(w_bytes), l - 1)
    z = ctx.upload(bytes(32 * M))
    z.write(w_bytes, 0)
    z.write(hl.frs_to_bytes(x_run), 32 * half)
    mz = [ctx.alloc(32 * M) for _ in range(3)]
    hl._check(ctx.lib.lh_debug_spartan_spmv(ctx.h, key.h, 0, fr_ptr(z), fr_pp(mz)))
    zero = ctx.upload(bytes(32 * M))
    d_e = hl.MultilinearPolynomial(ctx, ctx.alloc(32 * M), l)
    bad = (C.c_size_t * 2)()
    # T = a1 b2 + a2 b1 - u1 c2 - u2 c1 with (a2, b2, c2) = (0, Bz', 0) and u2 = x'[0]: Az' Bz' - x'[0] Cz'
    hl._check(ctx.lib.lh_debug_nova_cross_term(ctx.h, l, fr_pp(mz), fr_pp([zero, mz[1], zero]), None, None, hl._fr_array([1]),
                                               hl._fr_array([x_run[0]]), fr_ptr(d_e), bad))
    cw, ce = hl.MultilinearKzg.commit(pp, d_w), hl.MultilinearKzg.commit(pp, d_e)
    blob = be32(0) + b"".join(be32(c) for pt in (cw, ce) for c in pt) + b"".join(be32(v) for v in x_run)
    for b in mz + [zero]:
        b.free()
    return blob, d_w, d_e, z


def timed(ctx, fn):
    ctx.sync()
    t = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t) * 1e3, out


def profiled(ctx, fn):
    hl.profile_enable(ctx, True)
    try:
        fn()
        return hl.profile_read(ctx)
    finally:
        hl.profile_enable(ctx, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20:16", "20:20", "24:20"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nova_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=1000, help="seconds for the whole run: the process ends there")
    args = ap.parse_args()

    def expired(signum, frame):
        sys.stderr.write("exceeded the %d s limit\n" % args.limit)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)

    ctx = hl.Context(0)
    med = lambda v: round(statistics.median(v), 4)
    spread = lambda v: round(max(v) - min(v), 4)
    for text in args.shapes:
        n, l = [int(v) for v in text.split(":")]
        M, half = 1 << l, 1 << (l - 1)
        rng = np.random.default_rng(1000 * n + 10 * l)
        ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
        pp = hl.MultilinearKzg.setup(ctx, ss)
        vp = hl.MultilinearKzgVerifierParams.setup(ss)
        x = [1] + [int(v) for v in rng.integers(1, 1 << 62, size=PUBLIC - 1)]
        x_run = [int(v) for v in rng.integers(1, 1 << 62, size=PUBLIC)]
        for skewed in (False, True):
            mats, d_w = instance(ctx, pp, rng, n, l, skewed, x)
            key = hl.r1cs_commit(ctx, pp, mats, l)
            fresh = hl.nova_instance(ctx, pp, key, d_w, x)
            run_blob, run_w, run_e, z1 = running_instance(ctx, pp, key, rng, l, x_run)
            w_out = hl.MultilinearPolynomial(ctx, ctx.alloc(32 * half), l - 1)
            e_out = hl.MultilinearPolynomial(ctx, ctx.alloc(32 * M), l)
            step = lambda: hl.nova_fold(ctx, pp, key, run_blob, run_w, run_e, fresh, d_w, None, w_out, e_out)

            # ---- the fold step: one untimed, --reps timed, each verified on the host
            fold_ms, fold_verify_ms = [], []
            for rep in range(args.reps + 1):
                dt, (folded, proof) = timed(ctx, step)
                t = time.perf_counter()
                assert hl.nova_fold_verify(n, l, key.commitment, run_blob, fresh, proof) == folded
                if rep:
                    fold_ms.append(round(dt, 3))
                    fold_verify_ms.append((time.perf_counter() - t) * 1e3)
            kernels = by_name(profiled(ctx, step))

            # ---- the relaxed proof of the folded instance, and the plain proof of the same key
            relaxed_ms, relaxed_verify_ms, plain_ms, sizes = [], [], [], set()
            for rep in range(args.reps + 1):
                dt, rproof = timed(ctx, lambda: hl.spartan_prove_relaxed(ctx, pp, key, folded, w_out, e_out))
                t = time.perf_counter()
                hl.spartan_verify_relaxed(vp, n, l, key.commitment, folded, PUBLIC, rproof)  # (raises unless valid)
                dv = (time.perf_counter() - t) * 1e3
                dp, _ = timed(ctx, lambda: hl.spartan_prove(ctx, pp, key, d_w, x))
                sizes.add(len(rproof))
                if rep:
                    relaxed_ms.append(round(dt, 3)), relaxed_verify_ms.append(dv), plain_ms.append(round(dp, 3))

            # ---- the yardstick of nova_spmv2: one launch set over (z1, z2) against two of spartan_spmv, profiled, alternating
            z2 = ctx.upload(bytes(32 * M))
            z2.write(d_w.buf.read(32 * half), 0)
            z2.write(hl.frs_to_bytes(x), 32 * half)
            outs = [ctx.alloc(32 * M) for _ in range(6)]
            one = lambda: hl._check(ctx.lib.lh_debug_nova_spmv2(ctx.h, key.h, 0, fr_ptr(z1), fr_ptr(z2), fr_pp(outs[:3]), fr_pp(outs[3:])))

            def two():
                hl._check(ctx.lib.lh_debug_spartan_spmv(ctx.h, key.h, 0, fr_ptr(z1), fr_pp(outs[:3])))
                hl._check(ctx.lib.lh_debug_spartan_spmv(ctx.h, key.h, 0, fr_ptr(z2), fr_pp(outs[3:])))
            one(), two()  # (untimed)
            spmv2_ms, two_ms = [], []
            for rep in range(args.reps):
                spmv2_ms.append(sum(r["ms"] for r in profiled(ctx, one) if r["name"] == "nova_spmv2"))
                two_ms.append(sum(r["ms"] for r in profiled(ctx, two) if r["name"] == "spartan_spmv"))

            rec = dict(shape=dict(num_vars=n, dim_vars=l, num_public=PUBLIC), positions="skewed" if skewed else "uniform", pcs="mkzg",
                       reps=args.reps, fold_ms=fold_ms, fold_ms_median=med(fold_ms), fold_spread_ms=spread(fold_ms),
                       fold_proof_bytes=len(proof), fold_profiled_split_ms=split(kernels), fold_kernels=kernels,
                       host_fold_verify_ms_median=round(statistics.median(fold_verify_ms), 2),
                       relaxed_ms=relaxed_ms, relaxed_ms_median=med(relaxed_ms), relaxed_spread_ms=spread(relaxed_ms),
                       relaxed_proof_bytes=sorted(sizes), host_relaxed_verify_ms_median=round(statistics.median(relaxed_verify_ms), 1),
                       spartan_prove_ms=plain_ms, spartan_prove_ms_median=med(plain_ms),
                       step_over_proof=round(statistics.median(fold_ms) / statistics.median(plain_ms), 4),
                       nova_spmv2_ms=[round(v, 4) for v in spmv2_ms], nova_spmv2_ms_median=med(spmv2_ms),
                       two_spartan_spmv_ms=[round(v, 4) for v in two_ms], two_spartan_spmv_ms_median=med(two_ms),
                       two_spartan_spmv_spread_ms=spread(two_ms),
                       nova_spmv2_within_yardstick=bool(statistics.median(spmv2_ms) <= statistics.median(two_ms) + (max(two_ms) - min(two_ms))))
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            for b in outs + [z1, z2]:
                b.free()
            key.free()
            del mats, d_w, run_w, run_e, w_out, e_out
        pp.free()


if __name__ == "__main__":
    main()
