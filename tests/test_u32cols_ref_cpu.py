"""The reference of the 32-bit column kernels (tests/u32cols_ref.py) on its own, no GPU: its numpy dot product against the
plain one, its eq tables against the definition, what its quad sums and bind2 results MEAN - the first three round messages
of an eq-factored sum-check, assembled the way csrc/sumcheck.cpp assembles them, against a textbook computation over the
expanded field-element tables - and that the GPU suite's own input cases tell every listed wrong kernel from a right one."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import u32cols_ref as ur  # noqa: E402

R = ur.R_MOD


def test_dot_and_eq_tables_against_their_definitions():
    for n in (0, 1, 2, 255, (1 << 16) + 3):
        t = ur.fr_random(n, ("dot", n))
        for pattern in ur.PATTERNS:
            col = ur.column(pattern, n, n, ("dot", n))
            assert ur.dot(t, col) == ur.dot_plain(t.ints(), col), (n, pattern)
        assert all(v < R for v in t.ints())
    assert ur.dot(ur.fr_random(9, 1), ur.column("ones", 4, 4, 1)[0:4:2]) == ur.dot_plain(ur.fr_random(9, 1).ints()[:2], [0xFFFFFFFF] * 2)
    y = ur.fr_random(5, "y", False).ints()
    assert ur.eq_table(y) == [ur.eq_at(y, i) for i in range(32)]
    assert ur.eq_table(y, 19) == [ur.eq_at(y, i) for i in range(19)] and sum(ur.eq_table(y)) % R == 1
    assert ur.eq_table([]) == [1]
    # the stored forms the edge weights stand for
    assert [v * ur.MONT % R for v in ur.STORED_EDGES] == [0, ur.MONT, R - 1]
    assert [ur.num_vars_for(e) for e in (1, 2, 3, 257, 1 << 18, (1 << 18) + 1)] == [0, 1, 2, 9, 18, 19]


def test_closed_form_case_is_the_plain_sum():
    c, want = ur.closed_form_heavy(1000)
    assert want["sums"] == ur.reference(c)["sums"] == [ur.dot_plain(c.weights.ints(), c.cols[0])]
    # a lane of the capped 1024 x 256 grid adds 8 terms at n = 8 * 2^18: above 2^288, into limb 9 of its accumulator
    assert 8 * (R - 1) * 0xFFFFFFFF >= 1 << 288


# ------------------------------------------------------------------ what the sums mean: an eq-factored sum-check
def textbook_round(tables_w, y, rs, j, n):
    """round j of the eq-factored sum-check of sum_x eq(y, x) T(x) over the multilinear T = sum of w * table, after the
    challenges rs[0 .. j): (q_j(0), q_j(1)) with q_j(e) = sum_b eq(y[j+1 ..], b) T(rs, e, b) - T's multilinear extension
    evaluated from the definition, nothing folded"""
    T = [sum(w * t[i] for w, t in tables_w) % R for i in range(1 << n)]
    out = []
    for e in (0, 1):
        q = 0
        for b in range(1 << (n - j - 1)):
            at = sum(ur.eq_at(rs[:j], x) * T[x + (e << j) + (b << (j + 1))] for x in range(1 << j))
            q += ur.eq_at(y[j + 1:], b) * at
        out.append(q % R)
    return out


def expanded(col, ln, n):
    return [int(v) for v in col[:ln]] + [0] * ((1 << n) - ln)


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_surge_shape_rounds_0_to_2_from_one_column(n):
    """sum-check over ONE table that still is a column (sumcheck.cpp, u32_rounds): round 0 sends the odd half of the quad
    sums against E_0, round 1 (1 - r0) S2 + r0 S3, round 2 is sc_round_u32_bind2 against E_2"""
    for pattern in ur.PATTERNS:
        y = ur.fr_random(n, ("surge", n, pattern), False).ints()
        r0, r1 = ur.fr_random(2, ("surge r", n, pattern), False).ints()
        col = ur.column(pattern, 1 << n, 1 << n, ("surge", n))
        levels = [ur.eq_table(y[j + 1:]) for j in range(3)]  # E_j = eq(y[j+1 ..], .)
        quads = ur.reference(ur.Case("inner_products_small_quads", "", 1 << (n - 2), [col], [1 << n], ur.FrTable.from_ints(levels[0])))["sums"]
        bind = ur.reference(ur.Case("sc_round_u32_bind2", "", 1 << (n - 3), [col], [1 << n], ur.FrTable.from_ints(levels[2]), r0=r0, r1=r1))
        T = [(1, expanded(col, 1 << n, n))]
        assert quads[:2] == textbook_round(T, y, [], 0, n)  # the claim's halves; the round sends q(1) = odd
        assert ((1 - r0) * quads[2] + r0 * quads[3]) % R == textbook_round(T, y, [r0], 1, n)[1]
        assert bind["sums"] == [textbook_round(T, y, [r0, r1], 2, n)[1]]
        # ... and the table it leaves is T bound with (r0, r1)
        want = [sum(ur.eq_at([r0, r1], x) * T[0][1][x + 4 * i] for x in range(4)) % R for i in range(1 << (n - 2))]
        assert bind["table"] == want
        assert ur.quads_identity(ur.Case("inner_products_small_quads", "", 1 << (n - 2), [col], [1 << n], None, y=y), quads) == []


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_opening_shape_rounds_0_to_2_from_weighted_columns(n):
    """the batch opening's per-term shape (sumcheck.cpp, u32t_rounds): term m is eq(y_m, .) * merged_m with merged_m = sum_k
    w_k col_k.  Round 0 from the columns' quad sums against E_1 combined with y_1, round 1 from the same sums with r0,
    round 2 is lincomb_bind2 against E_2"""
    N = 1 << n
    r0, r1 = ur.fr_random(2, ("open r", n), False).ints()
    for m, lens in enumerate(([N, N - 4, 4, 0], [N], [N - 4, N, 2 * N])):
        y = ur.fr_random(n, ("open y", n, m), False).ints()
        w = ur.fr_random(len(lens), ("open w", n, m)).ints()
        cols = [ur.column(ur.PATTERNS[(k + m) % 4], ln, max(ln, N), ("open", n, m, k)) for k, ln in enumerate(lens)]
        levels = [ur.eq_table(y[j + 1:]) for j in range(3)]
        s = ur.reference(ur.Case("inner_products_quads", "", N // 4, cols, lens, ur.FrTable.from_ints(levels[1])))["table"]
        t4 = [sum(w[k] * s[4 * k + t] for k in range(len(lens))) % R for t in range(4)]
        bind = ur.reference(ur.Case("lincomb_bind2", "", N // 8, cols, lens, ur.FrTable.from_ints(levels[2]), w, r0=r0, r1=r1))
        T = [(w[k], expanded(cols[k], min(lens[k], N), n)) for k in range(len(lens))]
        y1 = y[1]
        assert [((1 - y1) * t4[0] + y1 * t4[2]) % R, ((1 - y1) * t4[1] + y1 * t4[3]) % R] == textbook_round(T, y, [], 0, n)
        assert [((1 - r0) * t4[0] + r0 * t4[1]) % R, ((1 - r0) * t4[2] + r0 * t4[3]) % R] == textbook_round(T, y, [r0], 1, n)
        assert bind["sums"] == textbook_round(T, y, [r0, r1], 2, n)
        # the fold of an opening's first step and the plain combination are the same polynomial's
        mixed = ur.reference(ur.Case("lincomb_mixed", "", N, cols, lens, None, w))["table"]
        assert mixed == [sum(wk * t[i] for wk, t in T) % R for i in range(N)]
        x = y[0]
        fold = ur.reference(ur.Case("lincomb_fold_small", "", N // 2, cols, [min(ln, N) for ln in lens], None, w, r0=x))["table"]
        assert fold == [((1 - x) * mixed[i] + x * mixed[i + N // 2]) % R for i in range(N // 2)]


def test_half_table_reference_is_the_full_inner_product():
    for kw in ur.cases("inner_products_small_half"):
        if kw["half"] > 300:
            continue
        c = ur.build("inner_products_small_half", **kw)
        want = [sum(ur.eq_at(c.y, i) * int(col[i]) for i in range(2 * c.n)) % R for col in c.cols]
        assert ur.reference(c)["sums"] == want, c.what()
        assert c.weights.ints() == [ur.eq_at(c.y[1:], b) for b in range(c.n)]


# ------------------------------------------------------------------ the GPU suite's inputs tell wrong kernels from right ones
def test_case_lists_hold_the_shapes_every_branch_needs():
    sizes = lambda op: sorted({ur.size_of(op, kw) for kw in ur.cases(op, cus=256)})  # noqa: E731
    assert sizes("inner_products_small") == [1, 63, 64, 65, 255, 256, 257, 1 << 18, (1 << 18) + 1, 3 * (1 << 18) + 77]
    assert sizes("inner_products_small_half") == [1, 2, 64, 257, (1 << 18) + 1]
    assert sizes("inner_products_small_quads") == [1, 2, 63, 64, 65, 256, 257, 1 << 18, (1 << 18) + 1, (1 << 19) + 5]
    assert sizes("inner_products_quads") == [1, 64, 65, 257, (1 << 18) + 1]
    assert sizes("lincomb_mixed") == [1, 255, 257, (1 << 20) + 1]
    assert sizes("lincomb_fold_small") == [1, 2, 255, 257, (1 << 20) + 1]
    for op in ("lincomb_bind2", "sc_round_u32_bind2"):
        assert sizes(op) == [1, 2, 64, 127, 128, 129, (1 << 18) + 257]
        assert ur.cases(op, cus=304, size="stride")[0]["size"] == 4 * 256 * 304 + 257
    assert {kw["count"] for kw in ur.cases("inner_products_small")} == {1, 2, 3, 4, 5, 9}
    assert {kw["count"] for kw in ur.cases("inner_products_small") if kw["n"] >= 1 << 18} == {1, 2, 3, 4, 5}
    assert {kw["count"] for kw in ur.cases("inner_products_small_half")} == {1, 2, 3, 5}
    assert {len(kw["lens"]) for kw in ur.cases("inner_products_quads")} == {1, 2, 3, 5}
    assert {(kw["num_fr"], kw["num_sm"]) for kw in ur.cases("lincomb_mixed")} == {(0, 0), (0, 1), (1, 0), (1, 2), (8, 24)}
    assert {(kw["num_fr"], kw["num_sm"]) for kw in ur.cases("lincomb_mixed", size=(1 << 20) + 1)} == {(1, 2)}
    assert {kw["count"] for kw in ur.cases("lincomb_fold_small")} == {1, 2, 24}
    assert {kw["count"] for kw in ur.cases("lincomb_fold_small", size=(1 << 20) + 1)} == {2}
    assert {kw["count"] for kw in ur.cases("lincomb_bind2")} == {1, 2, 3, 24}
    assert {kw["count"] for kw in ur.cases("lincomb_bind2", size="stride")} <= {1, 2, 3}
    # every length of the issue's lists occurs, per operation
    seen = {op: set() for op in ur.OPS}
    for op in ("lincomb_mixed", "lincomb_fold_small", "lincomb_bind2"):
        for kw in ur.cases(op):
            if ur.size_of(op, kw) == 257 or (op == "lincomb_bind2" and kw["size"] == 129):
                seen[op].update(ur.build(op, **kw).lens)
    assert seen["lincomb_mixed"] == {0, 1, 256, 257, 262}
    assert seen["lincomb_fold_small"] == {0, 1, 256, 257, 258, 513, 514}
    assert seen["lincomb_bind2"] == {0, 4 * 129, 4 * 258, 8 * 258}
    # the quads' launch groups: both short, short with full, a lone tail
    five = [kw["lens"] for kw in ur.cases("inner_products_quads") if len(kw["lens"]) == 5][0]
    assert five[:2] == ("short", "zero") and five[2:4] == ("four", "full") and five[4:] == ("long",)


@pytest.mark.parametrize("name", sorted(ur.MUTANTS))
def test_some_case_tells_the_mutant_from_the_reference(name):
    op, mutant = ur.MUTANTS[name]
    for kw in ur.cases(op):
        if ur.size_of(op, kw) > 300:
            continue
        c = ur.build(op, **kw)
        want, got = ur.reference(c), mutant(c)
        if (want["sums"], want["table"]) != (got["sums"], got["table"]):
            return
    pytest.fail("no case of %s up to size 300 tells the mutant %s (%s) from the reference" % (op, name, mutant.__doc__))


def test_every_value_pattern_reaches_every_operation():
    for op in ur.OPS:
        seen = set()
        for kw in ur.cases(op):
            if ur.size_of(op, kw) <= 300:
                c = ur.build(op, **kw)
                for col, ln in zip(c.cols, c.lens):
                    body = col[:ln]
                    if ln >= 64:
                        seen.add("ones" if (body == 0xFFFFFFFF).all() else "zero" if not body.any() else
                                 "sparse" if body.max() == 1 else "uniform")
        assert seen == set(ur.PATTERNS), (op, seen)


def test_failure_lines_name_operation_shape_column_and_index():
    def got_of(want, table=None, sums=None):
        return {"sums": sums if sums is not None else want["sums"], "taken": True, "untouched": False,
                "table": ur.FrTable.from_ints(table if table is not None else want["table"]) if want["table"] is not None else None}

    c = ur.build("inner_products_quads", quads=64, lens=("full", "long", "short"))
    want = ur.reference(c)
    assert ur.compare(c, got_of(want), want) == []
    wrong = list(want["table"])
    wrong[6] = (wrong[6] + 1) % R
    wrong[9] = (wrong[9] + 5) % R
    (line,) = ur.compare(c, got_of(want, table=wrong), want)
    assert line.startswith("inner_products_quads (quads=64, lens full/long/short") and "2 of 12 entries" in line
    assert "first column 1 (length 512), S_2: got 0x%x, want 0x%x" % (wrong[6], want["table"][6]) in line
    c = ur.build("lincomb_bind2", size=129, count=3)
    want = ur.reference(c)
    wrong = list(want["table"])
    wrong[200] ^= 1
    lines = ur.compare(c, got_of(want, table=wrong, sums=want["sums"][::-1]), want)
    assert len(lines) == 2 and "size=129, count=3" in lines[0] and "first q(0)" in lines[0] and "first entry 200:" in lines[1]
    c = ur.build("inner_products_small", n=65, count=5)
    want = ur.reference(c)
    (line,) = ur.compare(c, got_of(want, sums=want["sums"][:4] + [0]), want)
    assert "n=65, count=5" in line and "1 of 5 sums differ, first column 4" in line
    c = ur.build("lincomb_fold_small", half=64, count=25)
    want = ur.reference(c)
    assert not want["taken"]
    assert ur.compare(c, {"sums": None, "table": None, "taken": True, "untouched": True}, want) == [c.what() + ": taken = True, want False"]
    assert ur.compare(c, {"sums": None, "table": None, "taken": False, "untouched": False}, want) == [c.what() + ": not taken, but d_out was written"]
    assert ur.compare(c, {"sums": None, "table": None, "taken": False, "untouched": True}, want) == []
