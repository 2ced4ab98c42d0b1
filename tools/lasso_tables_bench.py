"""The comparison table on one GPU (development aid, outside bench.py): less_than(4, 16) - two 32-bit operands as four
chunks of 8 + 8 bits, seven memories, terms of up to four factors - at 2^num_vars lookups over multilinear KZG, in ONE
process, with the output column a = g(E) as a 32-bit column (LH_LASSO_PRODUCT_U32=1: lasso_output_small_prod, a u32 MSM, the
small-column opening) against the field-element column (0: lasso_output, a full-width MSM, a field-element table in the
opening).  One untimed pass of each value, then --alternations rounds of 0 and 1; the two routes' proofs are compared, and
the host verifier checks the proof (both routes share the derived commitments of the one-bit LTU columns at l = 16: equal
bytes alone would not show them right).

The knob is live (read at every prove), so the process flips it through its own environment.  The prove time is the host's
wall clock around lh_lasso_prove with the stream drained; the phase split is lh_lasso_last_timing of the last prove of each
route.  One JSON line is appended to profiles/lasso_tables_bench.jsonl.

    timeout -k 10 600 python tools/lasso_tables_bench.py [--num-vars 20] [--alternations 5]
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

OUT = os.path.join(ROOT, "profiles", "lasso_tables_bench.jsonl")
KNOB = "LH_LASSO_PRODUCT_U32"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-vars", type=int, default=20)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--chunk-bits", type=int, default=16)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--limit", type=int, default=500, help="seconds for the whole run: the process ends there")
    args = ap.parse_args()

    def expired(signum, frame):
        sys.stderr.write("exceeded the %d s limit\n" % args.limit)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)

    n, c, l = args.num_vars, args.chunks, args.chunk_bits
    ctx = hl.Context(0)
    rng = np.random.default_rng(n)
    ss = [int(v) for v in rng.integers(1, 1 << 62, size=max(n, l))]
    pp = hl.MultilinearKzg.setup(ctx, ss)
    table = hl.LassoTable.less_than(c, l)
    dims = [rng.integers(0, 1 << l, size=1 << n, dtype=np.uint32) for _ in range(c)]
    h = l // 2
    for j in range(1, c):  # equal high chunks in a quarter of the lookups, so that every chunk decides somewhere
        hit = rng.integers(0, 4, size=1 << n) < j
        dims[j] = np.where(hit, (dims[j] >> h) * ((1 << h) + 1), dims[j]).astype(np.uint32)
    d_dims = [ctx.upload(d.tobytes()) for d in dims]

    ms, phases, proofs = {0: [], 1: []}, {}, {}
    saved = os.environ.get(KNOB)
    try:
        for rep in range(args.alternations + 1):
            for route in (0, 1):
                os.environ[KNOB] = str(route)
                tr = hl.Keccak256Transcript()
                ctx.sync()
                t = time.perf_counter()
                hl.lasso_prove(pp, table, n, d_dims, tr)
                ctx.sync()
                dt = (time.perf_counter() - t) * 1e3
                if rep:  # (the first pass of each route is untimed)
                    ms[route].append(round(dt, 3))
                phases[route] = {k: round(float(v), 3) for k, v in hl.lasso_last_timing(ctx).items()}
                proofs.setdefault(route, tr.into_proof())
    finally:
        if saved is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = saved
    assert proofs[0] == proofs[1], "the two output routes disagree"
    t = time.perf_counter()
    reader = hl.Keccak256Transcript.from_proof(proofs[1])
    hl.lasso_verify(hl.MultilinearKzgVerifierParams.setup(ss), table, n, reader)  # (raises unless the proof is valid)
    assert reader.remaining() == 0
    verify_ms = (time.perf_counter() - t) * 1e3
    route = hl.lasso_last_route(ctx)
    med = {r: statistics.median(v) for r, v in ms.items()}
    spread = {r: max(v) - min(v) for r, v in ms.items()}
    rec = dict(workload="less_than_c%d_l%d" % (c, l), num_vars=n, pcs="mkzg", alternations=args.alternations,
               field_column_ms=ms[0], u32_column_ms=ms[1], field_column_ms_median=round(med[0], 3),
               u32_column_ms_median=round(med[1], 3), field_column_spread_ms=round(spread[0], 3),
               u32_column_spread_ms=round(spread[1], 3),
               u32_wins=bool(med[0] - med[1] > max(spread.values())),  # the rule for the knob's default
               phases_ms_field_column=phases[0], phases_ms_u32_column=phases[1], proof_bytes=len(proofs[1]),
               host_verified=True, host_verify_ms=round(verify_ms, 1), derived_commitments=route["derived_commitments"])
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
