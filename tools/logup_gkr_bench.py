"""LogUp-GKR proofs with the fused leaf kernel against leaves + frac_up (development aid, outside bench.py): shapes
(num_vars, table_vars, widths) over multilinear KZG, in ONE process on one ctx.  One untimed pass, then --alternations
rounds of the two values of the route option logup_fused_leaves; a proof's time is the host's wall clock around
lh_logup_gkr_prove with the stream drained before and after, and EVERY timed proof is verified on the host.  A profiled
pass per value follows (per-kernel records, summed by name).  For a shape of width 1 whose table holds 32-bit values the
same lookups are also proved as a c = 1 Lasso proof into a registered subtable of those values - for a reader who has to
pick an argument, not a pass mark.  One JSON line per shape is appended to --out (profiles/logup_gkr_bench.jsonl).

    timeout -k 10 900 python tools/logup_gkr_bench.py [--shapes 20:16:1 24:16:2] [--alternations 5]
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


def shape_of(text):
    n, l, widths = text.split(":")
    return int(n), int(l), [int(w) for w in widths.split(",")]


def make_lookups(ctx, rng, n, l, widths):
    """-> (lookups, rows, tables): a width-1 table holds 32-bit values (the Lasso comparison registers them), a tuple's
    columns hold field elements; inputs are table rows gathered on the host in Montgomery form"""
    lookups, all_rows, tables = [], [], []
    for w in widths:
        if w == 1:
            table = [[int(v) for v in rng.integers(0, 1 << 32, size=1 << l, dtype=np.uint64)]]
        else:
            table = [[int.from_bytes(rng.bytes(31), "little") for _ in range(1 << l)] for _ in range(w)]
        rows = rng.integers(0, 1 << l, size=1 << n, dtype=np.uint32)
        ins = []
        for col in table:
            mont = np.frombuffer(hl.frs_to_bytes(col), dtype=np.uint8).reshape(1 << l, 32)
            ins.append(hl.MultilinearPolynomial(ctx, ctx.upload(mont[rows].tobytes()), n))
        lookups.append(hl.LogupLookup(ins, table))
        all_rows.append(rows)
        tables.append(table)
    return lookups, all_rows, tables


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
    ap.add_argument("--shapes", nargs="+", default=["20:16:1", "24:16:2"])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logup_gkr_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=800, help="seconds for the whole run: the process ends there")
    args = ap.parse_args()

    def expired(signum, frame):
        sys.stderr.write("exceeded the %d s limit\n" % args.limit)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)

    ctx = hl.Context(0)
    default_fused = hl.get_option(ctx, "logup_fused_leaves")
    for text in args.shapes:
        n, l, widths = shape_of(text)
        rng = np.random.default_rng(1000 * n + l)
        ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
        pp = hl.MultilinearKzg.setup(ctx, ss)
        vp = hl.MultilinearKzgVerifierParams.setup(ss)
        lookups, rows, tables = make_lookups(ctx, rng, n, l, widths)

        def prove(fused):
            hl.set_option(ctx, "logup_fused_leaves", fused)
            tr = hl.Keccak256Transcript()
            ctx.sync()
            t = time.perf_counter()
            hl.logup_gkr_prove(pp, lookups, tr)
            ctx.sync()
            return (time.perf_counter() - t) * 1e3, tr.into_proof()

        def verify(proof):
            t = time.perf_counter()
            reader = hl.Keccak256Transcript.from_proof(proof)
            hl.logup_gkr_verify(vp, lookups, n, reader)  # (raises unless the proof is valid)
            assert reader.remaining() == 0
            return (time.perf_counter() - t) * 1e3

        ms = {0: [], 1: []}
        verify_ms, proofs = [], set()
        for rep in range(args.alternations + 1):
            for fused in (1, 0):
                dt, proof = prove(fused)
                proofs.add(proof)
                if rep:  # (the first pass of each value is untimed)
                    ms[fused].append(round(dt, 3))
                    verify_ms.append(verify(proof))
        assert len(proofs) == 1, "the two routes wrote different bytes"
        kernels = {}
        for fused in (1, 0):
            hl.profile_enable(ctx, True)
            try:
                prove(fused)
                kernels[fused] = by_name(hl.profile_read(ctx))
            finally:
                hl.profile_enable(ctx, False)
        hl.set_option(ctx, "logup_fused_leaves", default_fused)
        rec = dict(shape=dict(num_vars=n, table_vars=l, widths=widths), pcs="mkzg", alternations=args.alternations,
                   proof_bytes=len(next(iter(proofs))), host_verify_ms_median=round(statistics.median(verify_ms), 1))
        for fused, side in ((1, "fused"), (0, "unfused")):
            rec[side + "_ms"] = ms[fused]
            rec[side + "_ms_median"] = round(statistics.median(ms[fused]), 3)
            rec[side + "_spread_ms"] = round(max(ms[fused]) - min(ms[fused]), 3)
            rec[side + "_kernels"] = kernels[fused]
        rec["fused_minus_unfused_ms"] = round(rec["fused_ms_median"] - rec["unfused_ms_median"], 3)
        rec["fused_is_default_by_rule"] = rec["fused_minus_unfused_ms"] <= max(rec["fused_spread_ms"], rec["unfused_spread_ms"])

        if widths == [1] and l <= 20:  # the same lookups as a c = 1 Lasso proof into a registered subtable of the table's values
            with hl.Subtable.register(tables[0][0]) as sub:
                table = hl.LassoTable(1, l, [(0, sub)], [(1, [0])])
                dims = [ctx.upload(rows[0].tobytes())]
                lasso_ms, proof = [], b""
                for rep in range(args.alternations + 1):
                    tr = hl.Keccak256Transcript()
                    ctx.sync()
                    t = time.perf_counter()
                    hl.lasso_prove(pp, table, n, dims, tr)
                    ctx.sync()
                    if rep:
                        lasso_ms.append(round((time.perf_counter() - t) * 1e3, 3))
                    proof = tr.into_proof()
                hl.lasso_verify(vp, table, n, hl.Keccak256Transcript.from_proof(proof))
            rec["lasso_c1_registered"] = dict(ms=lasso_ms, ms_median=round(statistics.median(lasso_ms), 3),
                                              spread_ms=round(max(lasso_ms) - min(lasso_ms), 3), proof_bytes=len(proof))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del lookups
        pp.free()


if __name__ == "__main__":
    main()
