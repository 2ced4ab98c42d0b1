"""LogUp-GKR proofs from 32-bit input columns (hl.U32Column, lh_logup_gkr_prove_columns) against the same 32-bit values
uploaded as field elements (the existing entry) - development aid, outside bench.py, in the manner of
tools/logup_gkr_bench.py: shapes (num_vars, table_vars, widths) over multilinear KZG, in ONE process on one ctx.  One
untimed pass, then --alternations rounds of the two routes; a proof's time is the host's wall clock around
hl.logup_gkr_prove with the stream drained before and after, EVERY timed proof is verified on the host, and the two routes
must write the same bytes.  A profiled pass per route follows (per-kernel records, summed by name).  One JSON line per
shape is appended to --out (profiles/logup_gkr_bench.jsonl); `u32_gain_beyond_spread` says whether the u32 route's median
lies below the Fr route's by more than the larger of the two spreads.

    timeout -k 10 900 python tools/logup_gkr_u32_bench.py [--shapes 20:16:1 24:16:2] [--alternations 5]
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

ROUTES = ("fr", "u32")


def shape_of(text):
    n, l, widths = text.split(":")
    return int(n), int(l), [int(w) for w in widths.split(",")]


def make_lookups(ctx, rng, n, l, widths):
    """-> {route: lookups}: every table column holds 32-bit values; the inputs are table rows gathered on the host, once
    as uint32_t and once in Montgomery form"""
    out = {r: [] for r in ROUTES}
    for w in widths:
        table = [rng.integers(0, 1 << 32, size=1 << l, dtype=np.uint64) for _ in range(w)]
        rows = rng.integers(0, 1 << l, size=1 << n, dtype=np.uint32)
        ints = [[int(v) for v in col] for col in table]
        fr, u32 = [], []
        for col, col_ints in zip(table, ints):
            mont = np.frombuffer(hl.frs_to_bytes(col_ints), dtype=np.uint8).reshape(1 << l, 32)
            fr.append(hl.MultilinearPolynomial(ctx, ctx.upload(mont[rows].tobytes()), n))
            u32.append(hl.U32Column(ctx.upload(col.astype(np.uint32)[rows].tobytes()), n))
        out["fr"].append(hl.LogupLookup(fr, ints))
        out["u32"].append(hl.LogupLookup(u32, ints))
    return out


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
    for text in args.shapes:
        n, l, widths = shape_of(text)
        rng = np.random.default_rng(1000 * n + l + 32)
        ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
        pp = hl.MultilinearKzg.setup(ctx, ss)
        vp = hl.MultilinearKzgVerifierParams.setup(ss)
        lookups = make_lookups(ctx, rng, n, l, widths)
        statement = [hl.LogupLookup(None, lk.table) for lk in lookups["fr"]]

        def prove(route):
            tr = hl.Keccak256Transcript()
            ctx.sync()
            t = time.perf_counter()
            hl.logup_gkr_prove(pp, lookups[route], tr)
            ctx.sync()
            return (time.perf_counter() - t) * 1e3, tr.into_proof()

        def verify(proof):
            t = time.perf_counter()
            reader = hl.Keccak256Transcript.from_proof(proof)
            hl.logup_gkr_verify(vp, statement, n, reader)  # (raises unless the proof is valid)
            assert reader.remaining() == 0
            return (time.perf_counter() - t) * 1e3

        ms = {r: [] for r in ROUTES}
        verify_ms, proofs = [], set()
        for rep in range(args.alternations + 1):
            for route in ROUTES:
                dt, proof = prove(route)
                proofs.add(proof)
                if rep:  # (the first pass of each route is untimed)
                    ms[route].append(round(dt, 3))
                    verify_ms.append(verify(proof))
        assert len(proofs) == 1, "the two routes wrote different bytes"
        kernels, open_depth = {}, {}
        for route in ROUTES:
            hl.profile_enable(ctx, True)
            try:
                prove(route)
                kernels[route] = by_name(hl.profile_read(ctx))
                open_depth[route] = hl.lasso_last_route(ctx)["open_small_depth"]
            finally:
                hl.profile_enable(ctx, False)
        rec = dict(tool="logup_gkr_u32_bench", shape=dict(num_vars=n, table_vars=l, widths=widths), pcs="mkzg",
                   alternations=args.alternations, proof_bytes=len(next(iter(proofs))), proofs_equal=True,
                   host_verify_ms_median=round(statistics.median(verify_ms), 1))
        for route in ROUTES:
            rec[route + "_ms"] = ms[route]
            rec[route + "_ms_median"] = round(statistics.median(ms[route]), 3)
            rec[route + "_spread_ms"] = round(max(ms[route]) - min(ms[route]), 3)
            rec[route + "_kernel_ms"] = round(sum(e["ms"] for e in kernels[route].values()), 3)
            rec[route + "_open_small_depth"] = open_depth[route]
            rec[route + "_kernels"] = kernels[route]
        rec["u32_minus_fr_ms"] = round(rec["u32_ms_median"] - rec["fr_ms_median"], 3)
        rec["u32_gain_beyond_spread"] = -rec["u32_minus_fr_ms"] > max(rec["fr_spread_ms"], rec["u32_spread_ms"])
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del lookups
        pp.free()


if __name__ == "__main__":
    main()
