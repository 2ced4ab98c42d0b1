"""Timing of a Gemini opening against a Zeromorph opening on one GPU (development aid, outside bench.py): same SRS, same
table, same point, the two alternated `--alt` times, medians; then one synchronised pass with per-launch HIP events that
splits the Gemini opening into its MSMs and its other kernels and counts its launches; and the arena's peak.
One JSON line per num_vars.

    timeout -k 10 900 python tools/gemini_bench.py [--alt 5] 20 22 24
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import halo2_lasso_amd as hl  # noqa: E402
import numpy as np  # noqa: E402


def timed(ctx, fn):
    ctx.sync()
    t = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("num_vars", type=int, nargs="*", default=[20, 22, 24])
    ap.add_argument("--alt", type=int, default=5)
    args = ap.parse_args()
    ctx = hl.Context(0)
    for nv in args.num_vars:
        rng = random.Random(nv)
        params = hl.Zeromorph.setup(ctx, rng.randrange(1, hl.R_MOD), 1 << nv)
        zpp, gpp = hl.Zeromorph.trim(params, 1 << nv), hl.Gemini.trim(params, 1 << nv)
        limbs = np.random.default_rng(nv).integers(0, 1 << 63, size=(1 << nv, 4), dtype=np.uint64)
        limbs[:, 3] %= np.uint64(0x30644E72E131A029)
        poly = hl.MultilinearPolynomial(ctx, ctx.upload(limbs.astype("<u8").tobytes()), nv)
        point = [rng.randrange(hl.R_MOD) for _ in range(nv)]
        sizes = {}

        def do_open(pcs, pp, key):
            tr = hl.Keccak256Transcript()
            pcs.open(pp, poly, point, tr)
            sizes[key] = len(tr.into_proof())

        do_open(hl.Zeromorph, zpp, "zeromorph"), do_open(hl.Gemini, gpp, "gemini")  # warm-up
        zm, gm = [], []
        for _ in range(args.alt):
            zm.append(timed(ctx, lambda: do_open(hl.Zeromorph, zpp, "zeromorph")))
            gm.append(timed(ctx, lambda: do_open(hl.Gemini, gpp, "gemini")))
        hl.profile_enable(ctx, 1)
        do_open(hl.Gemini, gpp, "gemini")
        split, launches = {}, 0
        for rec in hl.profile_read(ctx):
            launches += 1
            key = rec["name"] if rec["name"].startswith(("gm_", "fix_var")) else "msm_and_other"
            split[key] = split.get(key, 0.0) + rec["ms"]
        hl.profile_enable(ctx, 0)
        new_ms = sum(v for k, v in split.items() if k != "msm_and_other")
        print(json.dumps({
            "num_vars": nv, "alternations": args.alt,
            "zeromorph_open_ms": round(statistics.median(zm), 3), "gemini_open_ms": round(statistics.median(gm), 3),
            "gemini_over_zeromorph": round(statistics.median(gm) / statistics.median(zm), 3),
            "gemini_proof_bytes": sizes["gemini"], "zeromorph_proof_bytes": sizes["zeromorph"],
            "profiled_launch_records": launches, "profiled_new_kernels_ms": round(new_ms, 3),
            "profiled_msm_ms": round(split.get("msm_and_other", 0.0), 3),
            "profiled_split_ms": {k: round(v, 3) for k, v in sorted(split.items())},
            "memory_stats": [int(v) for v in hl.memory_stats(ctx)] if not isinstance(hl.memory_stats(ctx), dict) else hl.memory_stats(ctx),
        }), flush=True)
        params.free()


if __name__ == "__main__":
    main()
