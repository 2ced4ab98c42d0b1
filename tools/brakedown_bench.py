"""Timing of the Brakedown PCS on one GPU (development aid, outside bench.py): for each num_vars one JSON line with the
commit split into encode / column hash / Merkle (per-launch HIP events, a separate synchronised pass), the commit and
open wall times, the proof size, and the multilinear KZG commit of the same polynomial beside it.

    timeout -k 10 600 python tools/brakedown_bench.py [--spec 6] [--reps 3] 20 22 24
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import halo2_lasso_amd as hl  # noqa: E402
import numpy as np  # noqa: E402

STAGES = {"bd_gather": "encode", "bd_reed_solomon": "encode", "bd_hash_columns": "hash", "bd_merkle_level": "merkle"}


def wall(ctx, fn, reps):
    best = None
    for _ in range(reps):
        ctx.sync()
        t = time.perf_counter()
        out = fn()
        ctx.sync()
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("num_vars", type=int, nargs="*", default=[20, 22, 24])
    ap.add_argument("--spec", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    ctx = hl.Context(0)
    seed = bytes(range(32))
    for nv in args.num_vars:
        t = time.perf_counter()
        pp = hl.Brakedown.setup(ctx, nv, args.spec, seed)
        setup_s = time.perf_counter() - t
        limbs = np.random.default_rng(nv).integers(0, 1 << 63, size=(1 << nv, 4), dtype=np.uint64)
        limbs[:, 3] %= np.uint64(0x30644E72E131A029)
        poly = hl.MultilinearPolynomial(ctx, ctx.upload(limbs.astype("<u8").tobytes()), nv)
        hl.Brakedown.commit(pp, poly).free()  # warm-up
        commit_ms, comm = wall(ctx, lambda: hl.Brakedown.commit(pp, poly), args.reps)
        hl.profile_enable(ctx, 1)
        hl.Brakedown.commit(pp, poly).free()
        split = {"encode": 0.0, "hash": 0.0, "merkle": 0.0}
        for rec in hl.profile_read(ctx):
            if rec["name"] in STAGES:
                split[STAGES[rec["name"]]] += rec["ms"]
        hl.profile_enable(ctx, 0)
        rng = random.Random(nv)
        point = [rng.randrange(hl.R_MOD) for _ in range(nv)]
        proofs = []

        def do_open():
            tr = hl.Keccak256Transcript()
            hl.Brakedown.open(pp, poly, comm, point, tr)
            proofs.append(tr.into_proof())

        open_ms, _ = wall(ctx, do_open, args.reps)
        kzg_pp = hl.MultilinearKzg.setup(ctx, [rng.randrange(1, hl.R_MOD) for _ in range(nv)])
        hl.MultilinearKzg.commit(kzg_pp, poly)
        kzg_ms, _ = wall(ctx, lambda: hl.MultilinearKzg.commit(kzg_pp, poly), args.reps)
        print(json.dumps({
            "num_vars": nv, "spec": args.spec, "row_len": pp.row_len, "num_rows": pp.num_rows,
            "codeword_len": pp.codeword_len, "setup_s": round(setup_s, 3),
            "commit_ms": round(commit_ms, 3), "encode_ms": round(split["encode"], 3),
            "column_hash_ms": round(split["hash"], 3), "merkle_ms": round(split["merkle"], 3),
            "open_ms": round(open_ms, 3), "proof_bytes": len(proofs[-1]), "mkzg_commit_ms": round(kzg_ms, 3),
        }), flush=True)
        comm.free()


if __name__ == "__main__":
    main()
