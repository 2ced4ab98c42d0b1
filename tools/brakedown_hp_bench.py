"""HyperPlonk over Brakedown on one GPU (development aid, outside bench.py).  At 2^num_vars, Spec6, in ONE process:

  batched commit   lh_brakedown_batch_commit of 8 polys as one batch (option brakedown_batch_commit 1) against the loop of
                   single commits (0), five alternations, medians;
  staged open      one poly opened at two points from the staged matrix (option brakedown_staged_open 1) against the column
                   round trips (0), five alternations, medians; the two routes' bytes are compared;
  the proof        vanilla_plonk_with_lookup (halo2_lasso_amd.synthetic) proved over Brakedown and over multilinear KZG, the
                   Brakedown proof checked by the host verifier, the arena's peak beside it.

With --lasso, instead (the Lasso prover over Brakedown): the 2^num_vars range check with c = 2, l = 16,
  column commit    lh_brakedown_commit_columns of its 9 columns (a | dim | read_ts | E | final_cts as u32) with the first
                   encoder stage from the 4-byte entries (option brakedown_u32_gather 1) against the generic gather on the
                   loaded message (0), five alternations, medians; the two routes' roots are compared;
  the proof        lh_lasso_prove_brakedown and lh_lasso_prove over multilinear KZG on the same lookups, the phase times
                   of the Brakedown proof (lh_lasso_last_timing) and the host verifier beside them.

Every step runs under a time limit of its own (--step-limit seconds: the process ends there, nothing is tried again), and the
whole under the caller's.  One JSON line per step is appended to profiles/brakedown_hp_bench.jsonl.

    timeout -k 10 900 python tools/brakedown_hp_bench.py [--num-vars 20] [--polys 8] [--alternations 5] [--lasso]
"""
import argparse
import json
import os
import random
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_lasso_amd as hl  # noqa: E402
import numpy as np  # noqa: E402
from halo2_lasso_amd import hyperplonk as hp, synthetic  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "brakedown_hp_bench.jsonl")


class Step:
    """a named step under its own time limit: when it runs out the process ends (exit status 124), nothing is retried"""

    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def __enter__(self):
        def expired(signum, frame):
            sys.stderr.write("step %r exceeded its %d s limit\n" % (self.name, self.limit))
            os._exit(124)
        signal.signal(signal.SIGALRM, expired)
        signal.alarm(self.limit)
        self.t = time.perf_counter()
        return self

    def __exit__(self, *exc):
        signal.alarm(0)
        print("[%s] %.1f s" % (self.name, time.perf_counter() - self.t), flush=True)
        return False


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def rand_poly(ctx, nv, seed):
    limbs = np.random.default_rng(seed).integers(0, 1 << 63, size=(1 << nv, 4), dtype=np.uint64)
    limbs[:, 3] %= np.uint64(0x30644E72E131A029)
    return hl.MultilinearPolynomial(ctx, ctx.upload(limbs.astype("<u8").tobytes()), nv)


def timed(ctx, fn):
    ctx.sync()
    t = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t) * 1e3, out


def alternate(ctx, option, run, alternations):
    """-> {route: [ms]}: route 1, route 0, route 1, ... in one process, after one untimed pass of each"""
    ms = {0: [], 1: []}
    default = hl.get_option(ctx, option)
    try:
        for rep in range(alternations + 1):
            for route in (1, 0):
                hl.set_option(ctx, option, route)
                dt, _ = timed(ctx, lambda: run(route))
                if rep:
                    ms[route].append(dt)
    finally:
        hl.set_option(ctx, option, default)
    return ms


def range_check_columns(n, l=16):
    """the witness columns of a 2^n range check with c = 2 chunks of l bits, as the prover makes them, on the host:
    -> (dims, [a, dim_0, dim_1, read_ts_0, read_ts_1, E_0, E_1, final_cts_0, final_cts_1]) as uint32 arrays"""
    rng = np.random.default_rng(2000 + n)
    dims = [rng.integers(0, 1 << l, size=1 << n, dtype=np.uint32) for _ in range(2)]
    rts, fcs = [], []
    for d in dims:
        order = np.argsort(d, kind="stable")
        sd = d[order]
        start = np.flatnonzero(np.r_[True, sd[1:] != sd[:-1]])
        rank = np.arange(len(d)) - np.repeat(start, np.diff(np.r_[start, len(d)]))
        r = np.empty(len(d), dtype=np.uint32)
        r[order] = rank  # read_ts[k] = earlier lookups of the same index
        rts.append(r)
        fcs.append(np.bincount(d, minlength=1 << l).astype(np.uint32))
    a = (dims[0].astype(np.uint64) + (dims[1].astype(np.uint64) << l)).astype(np.uint32)
    return dims, [a, dims[0], dims[1], rts[0], rts[1], dims[0].copy(), dims[1].copy(), fcs[0], fcs[1]]


def lasso_steps(ctx, args, base):
    nv, l = args.num_vars, 16
    assert nv >= l, "--lasso: the lookups must be at least as many as the subtable's entries"
    table = hl.LassoTable.range(2, l)
    with Step("setup", args.step_limit):
        pp = hl.Brakedown.setup(ctx, nv, args.spec, bytes(range(32)))
        base.update(row_len=pp.row_len, num_rows=pp.num_rows, codeword_len=pp.codeword_len)
        dims, cols = range_check_columns(nv, l)
        d_cols = [ctx.upload(c.tobytes()) for c in cols]
        d_dims = [ctx.upload(d.tobytes()) for d in dims]

    with Step("column commit", args.step_limit):
        roots = {}

        def commit(route):
            comms = hl.Brakedown.commit_columns(pp, [(b.ptr, "u32", len(c)) for b, c in zip(d_cols, cols)])
            roots[route] = [c.root for c in comms]
            for c in comms:
                c.free()
        ms = alternate(ctx, "brakedown_u32_gather", commit, args.alternations)
        assert roots[0] == roots[1], "the two gather routes disagree"
        emit(dict(base, step="commit_columns", workload="range_c2_l16", columns=len(cols), u32_gather_ms=ms[1],
                  generic_gather_ms=ms[0], u32_gather_ms_median=round(statistics.median(ms[1]), 3),
                  generic_gather_ms_median=round(statistics.median(ms[0]), 3),
                  ratio_generic_over_u32=round(statistics.median(ms[0]) / statistics.median(ms[1]), 3)))
    del d_cols

    with Step("lasso over brakedown", args.step_limit):
        ms, phases, proof = [], None, None
        for rep in range(4):
            tr = hl.Keccak256Transcript()
            dt, _ = timed(ctx, lambda: hl.lasso_prove(pp, table, nv, d_dims, tr))
            if rep:
                ms.append(dt)
            phases = hl.lasso_last_timing(ctx)
            if proof is None:
                proof = tr.into_proof()
        mem = hl.memory_stats(ctx)
        dt_v, _ = timed(ctx, lambda: hl.lasso_verify(pp, table, nv, hl.Keccak256Transcript.from_proof(proof)))
        emit(dict(base, step="lasso_brakedown", workload="range_c2_l16", prove_ms=ms,
                  prove_ms_median=round(statistics.median(ms), 3), phases_ms_last={k: round(float(v), 3) for k, v in phases.items()},
                  proof_bytes=len(proof), host_verify_ms=round(dt_v, 1), arena_high_water_bytes=mem["arena_high_water_bytes"]))
    with Step("lasso over multilinear kzg", args.step_limit):
        rng = np.random.default_rng(nv)
        kzg = hl.MultilinearKzg.setup(ctx, [int(v) for v in rng.integers(1, 1 << 62, size=nv)])
        ms = []
        for rep in range(4):
            tr = hl.Keccak256Transcript()
            dt, _ = timed(ctx, lambda: hl.lasso_prove(kzg, table, nv, d_dims, tr))
            if rep:
                ms.append(dt)
        emit(dict(base, step="lasso_mkzg", workload="range_c2_l16", prove_ms=ms,
                  prove_ms_median=round(statistics.median(ms), 3), proof_bytes=len(tr.into_proof())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-vars", type=int, default=20)
    ap.add_argument("--spec", type=int, default=6)
    ap.add_argument("--polys", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--lasso", action="store_true", help="the Lasso prover's steps instead of HyperPlonk's")
    args = ap.parse_args()
    nv, seed = args.num_vars, bytes(range(32))
    ctx = hl.Context(0)
    base = {"num_vars": nv, "spec": args.spec}
    if args.lasso:
        return lasso_steps(ctx, args, base)

    with Step("setup", args.step_limit):
        pp = hl.Brakedown.setup(ctx, nv, args.spec, seed)
        base.update(row_len=pp.row_len, num_rows=pp.num_rows, codeword_len=pp.codeword_len)
        polys = [rand_poly(ctx, nv, 100 + i) for i in range(args.polys)]

    with Step("batched commit", args.step_limit):
        roots = {}

        def commit(route):
            comms = hl.Brakedown.batch_commit(pp, polys)
            roots[route] = [c.root for c in comms]
            for c in comms:
                c.free()
        ms = alternate(ctx, "brakedown_batch_commit", commit, args.alternations)
        assert roots[0] == roots[1], "the two commit routes disagree"
        emit(dict(base, step="batch_commit", polys=args.polys, batched_ms=ms[1], per_poly_ms=ms[0],
                  batched_ms_median=round(statistics.median(ms[1]), 3), per_poly_ms_median=round(statistics.median(ms[0]), 3),
                  ratio_per_poly_over_batched=round(statistics.median(ms[0]) / statistics.median(ms[1]), 3)))

    with Step("staged open", args.step_limit):
        rng = random.Random(nv)
        poly = polys[0]
        comm = hl.Brakedown.commit(pp, poly)
        points = [[rng.randrange(hl.R_MOD) for _ in range(nv)] for _ in range(2)]
        evals = [hl.Evaluation(0, k, hl.evaluate_polys(ctx, [poly], pt)[0]) for k, pt in enumerate(points)]
        proofs = {}

        def open_(route):
            tr = hl.Keccak256Transcript()
            hl.Brakedown.batch_open(pp, nv, [poly], [comm], points, evals, tr)
            proofs[route] = tr.into_proof()
        ms = alternate(ctx, "brakedown_staged_open", open_, args.alternations)
        assert proofs[0] == proofs[1], "the two open routes disagree"
        emit(dict(base, step="open_two_points", proof_bytes=len(proofs[0]), staged_ms=ms[1], round_trips_ms=ms[0],
                  staged_ms_median=round(statistics.median(ms[1]), 3), round_trips_ms_median=round(statistics.median(ms[0]), 3),
                  ratio_round_trips_over_staged=round(statistics.median(ms[0]) / statistics.median(ms[1]), 3),
                  pinned_staging_bytes=32 * pp.num_rows * pp.codeword_len))
        comm.free()
    del polys
    if args.skip_proof:
        return

    with Step("circuit", args.step_limit):
        circ = synthetic.vanilla_plonk_with_lookup(ctx, nv)
    with Step("hyperplonk over brakedown", args.step_limit):
        g_pp, g_vp = synthetic.prover_param(pp, circ, pp)
        ms, proof = [], None
        for rep in range(4):
            tr = hl.Keccak256Transcript()
            dt, _ = timed(ctx, lambda: hp.HyperPlonk.prove(g_pp, circ.instances, circ.d_witness, tr))
            if rep:
                ms.append(dt)
            if proof is None:
                proof = tr.into_proof()
        mem = hl.memory_stats(ctx)
        dt_v, _ = timed(ctx, lambda: hp.HyperPlonk.verify(g_vp, circ.instances, hl.Keccak256Transcript.from_proof(proof)))
        emit(dict(base, step="hyperplonk_brakedown", workload="vanilla_plonk_with_lookup", prove_ms=ms,
                  prove_ms_median=round(statistics.median(ms), 3), proof_bytes=len(proof), host_verify_ms=round(dt_v, 1),
                  arena_high_water_bytes=mem["arena_high_water_bytes"]))
    with Step("hyperplonk over multilinear kzg", args.step_limit):
        rng = np.random.default_rng(nv)
        kzg = hl.MultilinearKzg.setup(ctx, [int(v) for v in rng.integers(1, 1 << 62, size=nv)])
        k_pp = synthetic.prover_param(kzg, circ)
        ms = []
        for rep in range(4):
            tr = hl.Keccak256Transcript()
            dt, _ = timed(ctx, lambda: hp.HyperPlonk.prove(k_pp, circ.instances, circ.d_witness, tr))
            if rep:
                ms.append(dt)
        emit(dict(base, step="hyperplonk_mkzg", workload="vanilla_plonk_with_lookup", prove_ms=ms,
                  prove_ms_median=round(statistics.median(ms), 3), proof_bytes=len(tr.into_proof())))


if __name__ == "__main__":
    main()
