"""CPU: the numpy restatement of the capturable two-stage inference link (tests/cascade_plan_ref.py) against what it replaces --
its candidate table against the numpy of TwoStageDetector.detect (the keep lists flattened groups ascending, row // L2 the frustum,
the frustum's frame and group looked up) on hand-worked keep lists, and its plan against the plan of tests/refine_plan_ref.py with
the counts as the positives, where the two overlap (everything but the two status bits that differ by design)."""
import numpy as np

import cascade_plan_ref as ref
import refine_plan_ref

STRIDES = (0.1, 0.2, 0.4, 0.8)
BIG = (1 << 20,) * 4


def _detect_numpy(keep_h, cnt_h, L2, frustum_frame, unit_group):
    """TwoStageDetector.detect's own lines, verbatim in their arithmetic."""
    rows = [keep_h[g, :c] for g, c in enumerate(cnt_h) if c > 0]
    rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros((0,), dtype=np.int64)
    unit = rows // L2
    frame = np.asarray(frustum_frame, dtype=np.int64).reshape(-1)[unit]
    return rows, frame, np.asarray(unit_group)[unit]


def _table(B1=4, L2=5, seed=0):
    rs = np.random.RandomState(seed)
    dets = rs.uniform(-1, 1, (B1 * L2, 8)).astype(np.float32)
    return dets, np.asarray([0, 0, 1, 1]), np.asarray([2, 0, 1, 1]), np.asarray([0, 0, 1, 2])


def test_candidates_by_hand():
    dets, uframe, uclass, ugroup = _table()
    keep = np.asarray([[7, 3, 9, -1, -1, -1], [12, -1, -1, -1, -1, -1], [19, 15, 16, 17, 18, 10]])
    cnt = np.asarray([3, 1, 6])
    out, n, st = ref.candidates(keep, cnt, 5, uframe, uclass, ugroup, dets, 12)
    assert n == 10 and st == 0
    assert out["cand_row"].tolist() == [7, 3, 9, 12, 19, 15, 16, 17, 18, 10, -1, -1]
    assert out["cand_frame"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, -1, -1]
    assert out["cand_class"].tolist() == [0, 2, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    assert out["cand_group"].tolist() == [0, 0, 0, 1, 2, 2, 2, 2, 2, 1, 3, 3]
    assert np.array_equal(out["cand_score"][:10], dets[out["cand_row"][:10], 7]) and not out["cand_score"][10:].any()
    assert all(out[k].dtype == np.int32 for k in ("cand_row", "cand_frame", "cand_class", "cand_group")) and out["cand_score"].dtype == np.float32


def test_candidates_equal_the_numpy_of_detect():
    dets, uframe, uclass, ugroup = _table()
    rs = np.random.RandomState(3)
    for trial in range(50):
        G, top_k = int(rs.randint(1, 6)), int(rs.randint(1, 7))
        cnt = rs.randint(0, top_k + 1, G)
        if trial % 5 == 0:
            cnt[:] = 0                                                       # the first stage keeps nothing
        keep = np.full((G, top_k), -1, dtype=np.int32)
        for g in range(G):
            keep[g, :cnt[g]] = rs.choice(len(dets), cnt[g], replace=False)
        rows, frame, group = _detect_numpy(keep, cnt, 5, uframe, ugroup)
        for D in (max(1, len(rows)), len(rows) + 3):
            out, n, st = ref.candidates(keep, cnt, 5, uframe, uclass, ugroup, dets, D)
            assert n == len(rows) and st == 0
            assert np.array_equal(out["cand_row"][:n], rows) and np.array_equal(out["cand_frame"][:n], frame)
            assert np.array_equal(out["cand_group"][:n], group) and np.array_equal(out["cand_class"][:n], uclass[rows // 5])
            assert (out["cand_row"][n:] == -1).all() and (out["cand_frame"][n:] == -1).all() and (out["cand_group"][n:] == G).all()
        if len(rows) > 1:                                                    # one candidate short: the first D rows, bit 7
            out, n, st = ref.candidates(keep, cnt, 5, uframe, uclass, ugroup, dets, len(rows) - 1)
            assert n == len(rows) - 1 and st == ref.ST_ROWS and np.array_equal(out["cand_row"], rows[:-1])


def test_candidates_that_are_never_dereferenced():
    dets, uframe, uclass, ugroup = _table()
    keep = np.asarray([[7, 3, 9], [12, 1, 2], [19, 15, 16]])
    # an overflowed group and a count beyond top_k: passed on to nobody, bit 9
    out, n, st = ref.candidates(keep, np.asarray([2, -1, 1]), 5, uframe, uclass, ugroup, dets, 8)
    assert st == ref.ST_GROUP and out["cand_row"][:n].tolist() == [7, 3, 19]
    out, n, st = ref.candidates(keep, np.asarray([2, 4, 1]), 5, uframe, uclass, ugroup, dets, 8)
    assert st == ref.ST_GROUP and out["cand_row"][:n].tolist() == [7, 3, 19]
    # entries outside dets, and entries of dets rows that belong to no frustum of the batch: skipped, no bit
    bad = keep.copy()
    bad[0, 1], bad[1, 0], bad[2, 2] = 20, -1, -2 ** 31
    out, n, st = ref.candidates(bad, np.asarray([3, 3, 3]), 5, uframe, uclass, ugroup, dets, 8)
    assert st == 0 and out["cand_row"][:n].tolist() == [7, 9, 1, 2, 19, 15]
    out, n, st = ref.candidates(keep, np.asarray([3, 3, 3]), 5, uframe[:3], uclass[:3], ugroup[:3], dets, 8)      # B1 = 3: rows >= 15 are out
    assert st == 0 and out["cand_row"][:n].tolist() == [7, 3, 9, 12, 1, 2]


def test_plan_equals_the_training_plan_where_they_overlap():
    rs = np.random.RandomState(5)
    for trial in range(60):
        D, S = int(rs.randint(1, 9)), int(rs.randint(1, 4))
        cnt = rs.randint(0, 30, (D, S)) * (rs.uniform(size=(D, 1)) < 0.7)
        psz = np.stack([rs.uniform(3, 5, D), rs.uniform(0.5, 2.5, D), rs.uniform(1, 2, D)], 1)
        if trial % 4 == 0:
            psz[rs.randint(D), 1] = [0.0, -1.0, np.nan, np.inf][trial // 4 % 4]
        lpad = BIG if trial % 3 else (16, 8, 4, 2)
        B = int(rs.randint(1, D + 1))
        cap = int(rs.choice([0, 7, int(cnt.sum()) // 2, int(cnt.sum()), 1 << 40]))
        got = ref.plan(cnt, psz, STRIDES, lpad, B, cap)
        want = refine_plan_ref.plan(cnt, cnt, psz, STRIDES, lpad, B, cap)
        for a, b in zip(got[:5], want[:5]):
            assert np.array_equal(a, b), trial
        shared = ref.ST_TRUNC | ref.ST_WIDE | ref.ST_WIDTH
        assert got[5] & shared == want[5] & shared and not got[5] & refine_plan_ref.ST_FEW
        survivors = sum(1 for d in range(D) if cnt[d].sum() > 0 and psz[d, 1] > 0 and np.isfinite(psz[d, 1])
                        and all(refine_plan_ref.windows(psz[d, 1], s) <= lp for s, lp in zip(STRIDES, lpad)))
        assert bool(got[5] & ref.ST_MANY) == (survivors > B) and bool(want[5] & refine_plan_ref.ST_FEW) == (survivors < B)


def test_plan_cases_by_hand():
    cnt = np.asarray([[5, 0, 2], [0, 0, 0], [3, 3, 3], [4, 1, 0]])
    psz = np.asarray([[4.0, 1.6, 1.5]] * 4)
    su, n, so, off, counts, st = ref.plan(cnt, psz, STRIDES, BIG, 4, 100)       # candidate 1 holds no row: no slot, no bit
    assert su.tolist() == [0, 2, 3, 4] and n == 3 and st == 0 and off.tolist() == [0, 7, 16, 100, 21] and counts.tolist() == [7, 9, 5, 0]
    assert so.tolist() == [0, 5, 5, 7, 7, 7, 7, 10, 13, 16, 20, 21, 21]
    su, n, so, off, counts, st = ref.plan(cnt, psz, STRIDES, BIG, 2, 100)       # more survivors than slots: bit 8
    assert su.tolist() == [0, 2] and n == 2 and st == ref.ST_MANY and off.tolist() == [0, 7, 16]
    su, n, so, off, counts, st = ref.plan(cnt, psz, STRIDES, BIG, 3, 20)        # one row short: bit 2
    assert st == ref.ST_TRUNC and counts.tolist() == [7, 9, 4] and off.tolist() == [0, 7, 16, 20]
    su, n, so, off, counts, st = ref.plan(cnt * 0, psz, STRIDES, BIG, 2, 20)    # nobody: no bit at all
    assert su.tolist() == [4, 4] and n == 0 and st == 0 and off.tolist() == [20, 20, 0] and not so.any()
