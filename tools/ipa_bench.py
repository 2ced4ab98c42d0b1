"""Timing of the multilinear IPA and of Hyrax on one GPU (development aid, outside bench.py): setup (the device generators), commit,
open and proof size, beside the multilinear-KZG commit and open of the same table at the same point, the two alternated
`--alt` times, medians; then one synchronised pass with per-launch HIP events that splits an IPA opening into its MSMs, its
base folds, its inner products / axpys and the rest (host time = the opening's wall time minus every record).
One JSON line per num_vars; `--hyrax` lists the sizes measured for Hyrax (batch_size 1) the same way.

    timeout -k 10 900 python tools/ipa_bench.py [--alt 5] 16 18 20 --hyrax 20 22 24
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
    ap.add_argument("num_vars", type=int, nargs="*", default=[16, 18, 20])
    ap.add_argument("--alt", type=int, default=5)
    ap.add_argument("--hyrax", type=int, nargs="*", default=[])
    args = ap.parse_args()
    ctx = hl.Context(0)
    for scheme, nv in [("ipa", v) for v in args.num_vars] + [("hyrax", v) for v in args.hyrax]:
        pcs = hl.Ipa if scheme == "ipa" else hl.Hyrax
        sizes_of = (lambda: (1 << nv,)) if scheme == "ipa" else (lambda: (1 << nv, 1))
        rng = random.Random(nv)
        setup_ms = []
        for _ in range(3):
            t = time.perf_counter()
            params = pcs.setup(ctx, *sizes_of())
            setup_ms.append((time.perf_counter() - t) * 1e3)
            if len(setup_ms) < 3:
                params.free()
        ipp = pcs.trim(params, *sizes_of())
        kpp = hl.MultilinearKzg.setup(ctx, [rng.randrange(1, hl.R_MOD) for _ in range(nv)])
        limbs = np.random.default_rng(nv).integers(0, 1 << 63, size=(1 << nv, 4), dtype=np.uint64)
        limbs[:, 3] %= np.uint64(0x30644E72E131A029)
        poly = hl.MultilinearPolynomial(ctx, ctx.upload(limbs.astype("<u8").tobytes()), nv)
        point = [rng.randrange(hl.R_MOD) for _ in range(nv)]
        sizes = {}

        def ipa_open():
            tr = hl.Keccak256Transcript()
            pcs.open(ipp, poly, point, tr)
            sizes["ipa"] = len(tr.into_proof())

        def kzg_open():
            tr = hl.Keccak256Transcript()
            hl.MultilinearKzg.open(kpp, poly, point, tr)
            sizes["kzg"] = len(tr.into_proof())

        ipa_commit = lambda: pcs.commit(ipp, poly)  # noqa: E731
        kzg_commit = lambda: hl.MultilinearKzg.commit(kpp, poly)  # noqa: E731
        for fn in (ipa_commit, kzg_commit, ipa_open, kzg_open):  # warm-up
            fn()
        t = {"ipa_commit": [], "kzg_commit": [], "ipa_open": [], "kzg_open": []}
        for _ in range(args.alt):
            t["ipa_commit"].append(timed(ctx, ipa_commit)), t["kzg_commit"].append(timed(ctx, kzg_commit))
            t["ipa_open"].append(timed(ctx, ipa_open)), t["kzg_open"].append(timed(ctx, kzg_open))
        hl.profile_enable(ctx, 1)
        wall = timed(ctx, ipa_open)
        split, launches = {}, 0
        for rec in hl.profile_read(ctx):
            launches += 1
            name = rec["name"]
            key = "base_fold" if name == "ipa_base_fold" else "inner_products_axpys" if name in ("ipa_cross", "ipa_fold_fr") \
                else "eq_xy" if name == "eq_xy" else "row_combination" if name == "hyrax_combine" else "msm"
            split[key] = split.get(key, 0.0) + rec["ms"]
        hl.profile_enable(ctx, 0)
        split["host_and_gaps"] = wall - sum(split.values())
        print(json.dumps({
            "scheme": scheme, "num_vars": nv, "alternations": args.alt, "ipa_setup_ms": round(statistics.median(setup_ms), 3),
            **{k + "_ms": round(statistics.median(v), 3) for k, v in t.items()},
            "ipa_proof_bytes": sizes["ipa"], "kzg_proof_bytes": sizes["kzg"],
            "profiled_open_ms": round(wall, 3), "profiled_launch_records": launches,
            "profiled_split_ms": {k: round(v, 3) for k, v in sorted(split.items())},
        }), flush=True)
        params.free()


if __name__ == "__main__":
    main()
