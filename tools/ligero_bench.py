"""Timing of the Ligero PCS on one GPU beside Brakedown Spec6 in the same process (development aid, outside bench.py): for
each num_vars one JSON line per scheme - Ligero at each log_inv_rate, then Brakedown - with the commit split into encode /
column hash / Merkle (per-launch HIP events, a separate synchronised pass), the commit and open wall times (the open also
over the staged matrix), the proof size and the device bytes of the commitment's rows.

    timeout -k 10 900 python tools/ligero_bench.py [--rates 1 2] [--reps 3] [--out profiles/ligero_bench.jsonl] 20 22 24
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

STAGES = {"bd_gather": "encode", "bd_reed_solomon": "encode", "bd_rs_encode": "encode", "bd_hash_columns": "hash",
          "bd_merkle_level": "merkle"}


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


def measure(ctx, pp, poly, nv, reps, label):
    hl.Brakedown.commit(pp, poly).free()  # warm-up
    commit_ms, comm = wall(ctx, lambda: hl.Brakedown.commit(pp, poly), reps)
    hl.profile_enable(ctx, 1)
    hl.Brakedown.commit(pp, poly).free()
    split = {"encode": 0.0, "hash": 0.0, "merkle": 0.0}
    for rec in hl.profile_read(ctx):
        if rec["name"] in STAGES:
            split[STAGES[rec["name"]]] += rec["ms"]
    hl.profile_enable(ctx, 0)
    rng = random.Random(nv)
    point = [rng.randrange(hl.R_MOD) for _ in range(nv)]
    value = hl.evaluate_polys(ctx, [poly], point)[0]
    proofs = []

    def do_open():
        tr = hl.Keccak256Transcript()
        hl.Brakedown.open(pp, poly, comm, point, tr)
        proofs.append(tr.into_proof())

    def do_staged_open():
        tr = hl.Keccak256Transcript()
        hl.Brakedown.batch_open(pp, nv, [poly], [comm], [point], [hl.Evaluation(0, 0, value)], tr)
        proofs.append(tr.into_proof())

    open_ms, _ = wall(ctx, do_open, reps)
    old = hl.get_option(ctx, "brakedown_staged_open")
    hl.set_option(ctx, "brakedown_staged_open", 1)
    try:
        staged_ms, _ = wall(ctx, do_staged_open, reps)
    finally:
        hl.set_option(ctx, "brakedown_staged_open", old)
    assert all(p == proofs[0] for p in proofs)
    t = time.perf_counter()
    hl.Brakedown.verify(pp, comm.root, point, value, hl.Keccak256Transcript.from_proof(proofs[0]))
    verify_ms = (time.perf_counter() - t) * 1e3
    comm.free()
    rec = dict(label)
    rec.update({"num_vars": nv, "row_len": pp.row_len, "num_rows": pp.num_rows, "codeword_len": pp.codeword_len,
                "num_column_opening": pp.num_column_opening, "rows_bytes": 32 * pp.num_rows * pp.codeword_len,
                "commit_ms": round(commit_ms, 3), "encode_ms": round(split["encode"], 3),
                "column_hash_ms": round(split["hash"], 3), "merkle_ms": round(split["merkle"], 3),
                "open_ms": round(open_ms, 3), "staged_open_ms": round(staged_ms, 3), "host_verify_ms": round(verify_ms, 1),
                "proof_bytes": len(proofs[0])})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("num_vars", type=int, nargs="*", default=[20, 22, 24])
    ap.add_argument("--rates", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    args = ap.parse_args()
    ctx = hl.Context(0)
    seed = bytes(range(32))
    for nv in args.num_vars:
        limbs = np.random.default_rng(nv).integers(0, 1 << 63, size=(1 << nv, 4), dtype=np.uint64)
        limbs[:, 3] %= np.uint64(0x30644E72E131A029)
        poly = hl.MultilinearPolynomial(ctx, ctx.upload(limbs.astype("<u8").tobytes()), nv)
        runs = [({"scheme": "ligero", "log_inv_rate": b}, lambda b=b: hl.Ligero.setup(ctx, nv, b)) for b in args.rates]
        runs.append(({"scheme": "brakedown", "spec": 6}, lambda: hl.Brakedown.setup(ctx, nv, 6, seed)))
        for label, make in runs:
            t = time.perf_counter()
            pp = make()
            setup_s = time.perf_counter() - t
            rec = measure(ctx, pp, poly, nv, args.reps, label)
            rec["setup_s"] = round(setup_s, 3)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            pp.free()
        poly.buf.free()


if __name__ == "__main__":
    main()
