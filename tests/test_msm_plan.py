"""The planning half of the batched MSM (csrc/msm.hip msm_chunk_prepare) through the host-only entry lh_debug_msm_plan.  No
GPU.  The batch comes in one call (msm_batch) or in two (msm_prepare, then msm_run: the helper ctx's staged precommit,
csrc/open_columns.cpp): both must plan the same sub-batches for the same jobs, a helper ctx never plans two halves, and
the numbers are the ones the window rule gives: a 32-bit column of n points and b significant bits gets windows of
c = min(max(floor(log2 n) - 4, 4), 17, b) bits (a packed pair: one window of b bits), W = ceil(b / c) of them, n W entries
and W 2^c buckets rounded up to whole key blocks."""
import ctypes as C

import pytest

LH_OK, LH_ERR_ARG = 0, -8
WORDS = ["jobs", "entries", "small_entries", "buckets", "segments", "windows", "groups", "shares", "k", "chunks", "seg_size",
         "plain_reduce"]

# job lists: (n, bits, kind) - kind 0 field elements, 1 a 32-bit column, >= 4 a packed pair with that shift
JOB_LISTS = {
    "one-small-u32": [(1000, 8, 1)],
    "one-fr": [(4097, 254, 0)],
    "range-2p17-precommit": [(1 << 16, 17, 1), (1 << 16, 17, 1), (1 << 16, 9, 1), (1 << 16, 9, 1)],
    "and-2p21-precommit": [(1 << 20, 9, 1)] * 4 + [(1 << 20, 17, 1)] * 2 + [(1 << 20, 18, 9), (1 << 20, 18, 9)],
    "and-2p24-precommit": [(1 << 23, 9, 1)] * 4 + [(1 << 23, 17, 1)] * 2 + [(1 << 23, 20, 10), (1 << 23, 20, 10)],
    "and-2p24-commit": [(1 << 24, 16, 1)] * 4 + [(1 << 24, 20, 10), (1 << 24, 20, 10)] + [(1 << 16, 14, 1)] * 4,
    "mixed": [(1 << 18, 254, 0), (1 << 18, 32, 1), (77, 1, 1), (1 << 12, 12, 4)],
    "forty-eight": [(1 << 10, 5 + (j % 20), 1) for j in range(48)],
}


@pytest.fixture(scope="module")
def plan(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()

    def plan(jobs, helper, via_prepare):
        k = len(jobs)
        n = (C.c_size_t * k)(*[j[0] for j in jobs])
        bits = (C.c_uint32 * k)(*[j[1] for j in jobs])
        kinds = (C.c_uint32 * k)(*[j[2] for j in jobs])
        out, subs = (C.c_uint64 * 24)(), C.c_size_t()
        st = lib.lh_debug_msm_plan(k, n, bits, kinds, int(helper), int(via_prepare), out, C.byref(subs))
        assert st == LH_OK, (jobs, st)
        return [dict(zip(WORDS, list(out)[12 * s:12 * s + 12])) for s in range(subs.value)]

    return plan


def window(n, bits, kind):
    """(window bits, windows) of a 32-bit column by the rule in the module's docstring"""
    if kind >= 4:
        return max(bits, 4), 1
    c = min(max(n.bit_length() - 1 - 4, 4), 17, bits)
    return c, -(-bits // c)


@pytest.mark.parametrize("name", list(JOB_LISTS))
@pytest.mark.parametrize("helper", [0, 1])
def test_two_calls_plan_what_one_call_plans(plan, name, helper):
    jobs = JOB_LISTS[name]
    one, two = plan(jobs, helper, 0), plan(jobs, helper, 1)
    assert one == two, (name, helper)
    assert sum(s["jobs"] for s in one) == len(jobs)
    if helper:
        assert len(one) == 1, "a helper ctx never splits a batch into halves"


@pytest.mark.parametrize("name", [k for k, v in JOB_LISTS.items() if all(j[2] for j in v)])
def test_entries_and_buckets_follow_the_window_rule(plan, name):
    jobs = JOB_LISTS[name]
    subs = plan(jobs, 1, 1)
    assert len(subs) == 1
    s = subs[0]
    shapes = [window(*j) for j in jobs]
    assert s["entries"] == sum(j[0] * w for j, (c, w) in zip(jobs, shapes)), (name, s)
    assert s["windows"] == sum(2 if j[2] >= 4 else w for j, (c, w) in zip(jobs, shapes)), (name, s)
    # (a job's key range starts at a multiple of 2^10 - of its 2^c buckets when it sorts slab by slab -, and a window's
    # buckets are rounded up to whole segments of at most 16)
    floor = sum(w << c for c, w in shapes)
    slack = sum(max(1 << 10, 1 << c) + 16 * w for c, w in shapes)
    assert floor <= s["buckets"] <= floor + slack, (name, s, floor)
    assert s["chunks"] == -(-s["entries"] // s["k"]) and s["small_entries"] <= s["entries"]
    assert s["seg_size"] in (4, 8, 16) and s["shares"] >= s["windows"]


def test_the_headline_commit_batch_runs_as_two_halves_on_an_owner_only(plan):
    jobs = JOB_LISTS["and-2p24-commit"]
    owner, helper = plan(jobs, 0, 1), plan(jobs, 1, 1)
    assert len(owner) == 2 and len(helper) == 1
    assert sum(s["entries"] for s in owner) == helper[0]["entries"]
    # (a half keeps the batch's forms: segment size, reduction kernels, entries per accumulate thread)
    for word in ("k", "seg_size", "plain_reduce"):
        assert owner[0][word] == owner[1][word] == helper[0][word], word


def test_plan_argument_errors(hl):
    from halo2_lasso_amd import _ffi
    lib = _ffi.load()
    n, bits, kinds = (C.c_size_t * 1)(16), (C.c_uint32 * 1)(8), (C.c_uint32 * 1)(1)
    out, subs = (C.c_uint64 * 24)(), C.c_size_t()
    assert lib.lh_debug_msm_plan(0, n, bits, kinds, 0, 0, out, C.byref(subs)) == LH_ERR_ARG
    assert lib.lh_debug_msm_plan(1, n, bits, kinds, 0, 0, None, C.byref(subs)) == LH_ERR_ARG
    bits[0] = 33  # wider than a 32-bit column
    assert lib.lh_debug_msm_plan(1, n, bits, kinds, 0, 0, out, C.byref(subs)) == LH_ERR_ARG
