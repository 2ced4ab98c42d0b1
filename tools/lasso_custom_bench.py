"""The cost of a registered subtable on one GPU (development aid, outside bench.py): bitwise(AND, 4, 16) - the default
bench.py table - at 2^num_vars lookups over multilinear KZG, in ONE process, with the built-in AND kind against the same 2^16
entries registered through lh_subtable_register (hl.Subtable.register).  The only difference between the two proves is
where a subtable entry comes from: computed from the index (lasso_subtable_read_kernel, the init leaves), or gathered from the
device copy of the registered entries (lasso_subtable_gather_kernel: 12 B per lookup and memory where the built-in moves 8,
the 256 KiB table through the caches; the same for the init leaves, and one 256 KiB upload plus a host sort per prove).
Both take the derived commitments (T[0] = 0).

One untimed pass of each, then --alternations rounds of built-in and registered; the two proofs are compared byte for byte
and the host verifier checks the proof under both tables.  The prove time is the host's wall clock around lh_lasso_prove with
the stream drained; the phase split is lh_lasso_last_timing of every timed prove.  One JSON line is appended to --out
(profiles/lasso_custom_bench.jsonl).

    timeout -k 10 600 python tools/lasso_custom_bench.py [--num-vars 24] [--alternations 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-vars", type=int, default=24)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--chunk-bits", type=int, default=16)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lasso_custom_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=500, help="seconds for the whole run: the process ends there")
    args = ap.parse_args()

    def expired(signum, frame):
        sys.stderr.write("exceeded the %d s limit\n" % args.limit)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)

    n, c, l = args.num_vars, args.chunks, args.chunk_bits
    h = l // 2
    ctx = hl.Context(0)
    rng = np.random.default_rng(n)
    ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
    pp = hl.MultilinearKzg.setup(ctx, ss)
    m = np.arange(1 << l, dtype=np.uint32)
    registered = hl.Subtable.register(((m >> h) & (m & ((1 << h) - 1))).tolist())
    builtin = hl.LassoTable.bitwise(hl.SUBTABLE_AND, c, l)
    tables = {"builtin": builtin, "registered": hl.LassoTable(c, l, [(j, registered) for j in range(c)], builtin.g_terms)}
    d_dims = [ctx.upload(rng.integers(0, 1 << l, size=1 << n, dtype=np.uint32).tobytes()) for _ in range(c)]

    ms, phases, proofs, routes = {k: [] for k in tables}, {k: [] for k in tables}, {}, {}
    for rep in range(args.alternations + 1):
        for name, table in tables.items():
            tr = hl.Keccak256Transcript()
            ctx.sync()
            t = time.perf_counter()
            hl.lasso_prove(pp, table, n, d_dims, tr)
            ctx.sync()
            dt = (time.perf_counter() - t) * 1e3
            if rep:  # (the first pass of each is untimed)
                ms[name].append(round(dt, 3))
                phases[name].append({k: float(v) for k, v in hl.lasso_last_timing(ctx).items()})
            proofs.setdefault(name, tr.into_proof())
            routes[name] = hl.lasso_last_route(ctx)["derived_commitments"]
    assert proofs["builtin"] == proofs["registered"], "the registered AND entries give another proof"
    vp = hl.MultilinearKzgVerifierParams.setup(ss)
    verify_ms = {}
    for name, table in tables.items():
        t = time.perf_counter()
        reader = hl.Keccak256Transcript.from_proof(proofs[name])
        hl.lasso_verify(vp, table, n, reader)  # (raises unless the proof is valid)
        assert reader.remaining() == 0
        verify_ms[name] = round((time.perf_counter() - t) * 1e3, 1)
    rec = dict(workload="and_c%d_l%d" % (c, l), num_vars=n, pcs="mkzg", alternations=args.alternations,
               proof_bytes=len(proofs["builtin"]), same_bytes=True, host_verify_ms=verify_ms, derived_commitments=routes)
    for name in tables:
        rec[name + "_ms"] = ms[name]
        rec[name + "_ms_median"] = round(statistics.median(ms[name]), 3)
        rec[name + "_spread_ms"] = round(max(ms[name]) - min(ms[name]), 3)
        rec[name + "_phases_ms_median"] = {k: round(statistics.median(p[k] for p in phases[name]), 3) for k in phases[name][0]}
        rec[name + "_phases_ms_spread"] = {k: round(max(p[k] for p in phases[name]) - min(p[k] for p in phases[name]), 3)
                                           for k in phases[name][0]}
    registered.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
