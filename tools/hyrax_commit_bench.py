"""Hyrax batch_commit on both commit routes on one GPU (development aid, outside bench.py): the per-ctx option hyrax_rows 1
(the row kernels of csrc/kernels_hyrax.hip) against 0 (one msm_batch job per row), timed at the C entry
lh_hyrax_batch_commit over random tables, minimum and median of a few calls after a warm-up call (which also builds the
generators' window table), and the two routes' points compared.  One JSON line per (num_vars, polys in the batch).

    timeout -k 10 400 python tools/hyrax_commit_bench.py [12:1 16:1 20:1 20:4 22:1 24:1]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import halo2_lasso_amd as hl  # noqa: E402
import numpy as np  # noqa: E402


def poly(ctx, n, seed):
    rs = np.random.default_rng(seed)
    raw = rs.integers(0, 1 << 63, size=(1 << n, 4), dtype=np.uint64)
    raw[:, 3] >>= 4  # below 2^252 < r: every row is a valid residue
    return hl.MultilinearPolynomial(ctx, ctx.upload(raw.tobytes()), n)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(min(ts), 3), round(sorted(ts)[len(ts) // 2], 3)


def main():
    shapes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(12, 1), (16, 1), (20, 1), (20, 4), (22, 1), (24, 1)]
    ctx = hl.Context(0)
    for n, batch in shapes:
        pp = hl.Hyrax.trim(hl.Hyrax.setup(ctx, 1 << n, 1), 1 << n, 1)
        polys = [poly(ctx, n, 100 * n + i) for i in range(batch)]
        rec = {"num_vars": n, "polys": batch, "rows": pp.num_chunks, "row_len": 1 << pp.row_num_vars}
        points = {}
        for route in (1, 0):
            hl.set_option(ctx, "hyrax_rows", route)
            points[route] = hl.Hyrax.batch_commit(pp, polys)
            out = (hl._ffi.lh_g1 * (batch * pp.num_chunks))()
            ptrs = hl._ptr_array(polys)
            rec["hyrax_rows_%d_ms_min_median" % route] = timed(lambda: hl._check(pp.lib.lh_hyrax_batch_commit(
                pp.ctx.h, pp.params.h, pp.poly_size, pp.batch_size, ptrs, batch, n, out)), 5 if n <= 20 else 3)
        rec["same_points"] = points[0] == points[1]
        print(json.dumps(rec), flush=True)
        del polys
    hl.set_option(ctx, "hyrax_rows", 1)


if __name__ == "__main__":
    main()
