"""One batch proof against one proof per table (development aid, outside bench.py): K tables with 2^num_vars lookups each
over multilinear KZG, in ONE process on one ctx -
  (a) K lh_lasso_prove calls in sequence, one transcript each,
  (b) one lh_lasso_prove_batch of the same tables and columns.
Batches:
  two_ranges        two range(2, 16), columns of their own
  and_xor_shared    bitwise(AND, 4, 16) + bitwise(XOR, 4, 16) over the SAME four chunk columns (counted and committed once)
  and_xor_distinct  the same two tables over columns of their own (32 product trees either way: the small GKR layers of the
                    batch run launched, gkr_resident takes 16 trees)

One untimed pass of each side, then --alternations rounds of (a), (b).  A side's time is the host's wall clock around its
proves with the stream drained before and after; the phase split is lh_lasso_last_timing (for (a): summed over the K proves).
The host verifier checks every proof once.  One JSON line per batch and size is appended to --out
(profiles/lasso_batch_bench.jsonl).

    timeout -k 10 600 python tools/lasso_batch_bench.py [--num-vars 16 20 24] [--batches two_ranges ...] [--alternations 5]
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

L = 16


def batches(ctx, rng, n):
    col = lambda: ctx.upload(rng.integers(0, 1 << L, size=1 << n, dtype=np.uint32).tobytes())
    rng16 = hl.LassoTable.range(2, L)
    and4, xor4 = hl.LassoTable.bitwise(hl.SUBTABLE_AND, 4, L), hl.LassoTable.bitwise(hl.SUBTABLE_XOR, 4, L)
    shared = [col() for _ in range(4)]
    return {
        "two_ranges": lambda: ([rng16, rng16], [[col(), col()], [col(), col()]]),
        "and_xor_shared": lambda: ([and4, xor4], [shared, shared]),
        "and_xor_distinct": lambda: ([and4, xor4], [shared, [col() for _ in range(4)]]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-vars", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--batches", nargs="+", default=["two_ranges", "and_xor_shared", "and_xor_distinct"])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lasso_batch_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=500, help="seconds for the whole run: the process ends there")
    args = ap.parse_args()

    def expired(signum, frame):
        sys.stderr.write("exceeded the %d s limit\n" % args.limit)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)

    ctx = hl.Context(0)
    for n in args.num_vars:
        rng = np.random.default_rng(n)
        ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, L))]
        pp = hl.MultilinearKzg.setup(ctx, ss)
        vp = hl.MultilinearKzgVerifierParams.setup(ss)
        makers = batches(ctx, rng, n)
        for name in args.batches:
            tables, cols = makers[name]()
            ms = {"singles": [], "batch": []}
            phases = {"singles": [], "batch": []}
            proofs, route = {}, {}
            for rep in range(args.alternations + 1):
                for side in ("singles", "batch"):
                    trs = [hl.Keccak256Transcript() for _ in (tables if side == "singles" else [0])]
                    ph = {}
                    ctx.sync()
                    t = time.perf_counter()
                    if side == "singles":
                        for table, c, tr in zip(tables, cols, trs):
                            hl.lasso_prove(pp, table, n, c, tr)
                            if rep:  # (resolving the phase events drains the stream: part of the K-proofs side as it is used)
                                for k, v in hl.lasso_last_timing(ctx).items():
                                    ph[k] = ph.get(k, 0.0) + float(v)
                    else:
                        hl.lasso_prove_batch(pp, tables, n, cols, trs[0])
                    ctx.sync()
                    dt = (time.perf_counter() - t) * 1e3
                    if side == "batch":
                        ph = {k: float(v) for k, v in hl.lasso_last_timing(ctx).items()}
                        route = hl.lasso_last_route(ctx)
                    if rep:  # (the first pass of each side is untimed)
                        ms[side].append(round(dt, 3))
                        phases[side].append(ph)
                    proofs.setdefault(side, [tr.into_proof() for tr in trs])
            t = time.perf_counter()
            reader = hl.Keccak256Transcript.from_proof(proofs["batch"][0])
            hl.lasso_verify_batch(vp, tables, n, reader)  # (raises unless the proof is valid)
            assert reader.remaining() == 0
            verify_batch_ms = round((time.perf_counter() - t) * 1e3, 1)
            t = time.perf_counter()
            for table, proof in zip(tables, proofs["singles"]):
                hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(proof))
            verify_singles_ms = round((time.perf_counter() - t) * 1e3, 1)
            rec = dict(batch=name, num_vars=n, pcs="mkzg", alternations=args.alternations,
                       proof_bytes={"singles": [len(p) for p in proofs["singles"]], "batch": len(proofs["batch"][0])},
                       host_verify_ms={"singles": verify_singles_ms, "batch": verify_batch_ms},
                       batch_resident_layers=route.get("resident_layers"), batch_derived_commitments=route.get("derived_commitments"),
                       batch_packed_ts_pairs=route.get("packed_ts_pairs"))
            for side in ("singles", "batch"):
                rec[side + "_ms"] = ms[side]
                rec[side + "_ms_median"] = round(statistics.median(ms[side]), 3)
                rec[side + "_spread_ms"] = round(max(ms[side]) - min(ms[side]), 3)
                rec[side + "_phases_ms_median"] = {k: round(statistics.median(p[k] for p in phases[side]), 3) for k in phases[side][0]}
            rec["batch_over_singles"] = round(rec["batch_ms_median"] / rec["singles_ms_median"], 3)
            lost = {k: round(rec["batch_phases_ms_median"][k] - rec["singles_phases_ms_median"][k], 3)
                    for k in rec["batch_phases_ms_median"] if k != "total"}
            rec["phase_delta_ms"] = lost  # (batch minus singles, per phase: the largest positive entry is the phase that lost)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            del tables, cols
        pp.free()


if __name__ == "__main__":
    main()
