// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the capturable
// two-stage inference link -- fcn_cascade_candidates, fcn_refine_detect_count / _plan / _fill, csrc/cascade_plan.h compiled for the
// host against tests/host_harness/hip_emu -- with exactly sized buffers: the candidate table at one group, at its 65536 groups and
// its 2048 candidates, with overflowed groups, counts beyond top_k, keep entries out of range and more kept rows than candidates;
// the plan with more and fewer survivors than slots, none at all, the capacity met, one row short and 0, D = S = B = 1, the
// largest plan and widths that are no width; candidates -> count -> plan -> fill on frames of one segment and of three, with the
// filler candidates of the table and out-of-range lists, into a point buffer of exactly capacity + 1 rows; argument handling.
// Built with -fsanitize=address,undefined by tests/test_cascade_plan_sanitizer.py, so a read or write past any buffer is a
// report, not luck.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <vector>
#include "include/fcn_hip.h"
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
static double unit() { return rand() / (RAND_MAX + 1.0); }
static const double STRIDE[4] = {0.1, 0.2, 0.4, 0.8};
static const int32_t BIG[4] = {1 << 20, 1 << 20, 1 << 20, 1 << 20};

struct Cands {
    std::vector<int32_t> row, frame, cls, group;
    std::vector<float> score;
    int32_t n = -9, status = 0;
    explicit Cands(int D) : row(D, -9), frame(D, -9), cls(D, -9), group(D, -9), score(D, -9.f) {}
};

// the table as the contract states it, sequentially
static void cand_ref(const std::vector<int32_t> &keep, const std::vector<int32_t> &cnt, int G, int top_k, int L2, const std::vector<int32_t> &uf,
                     const std::vector<int32_t> &uc, const std::vector<int32_t> &ug, const std::vector<float> &dets, int D, Cands &w)
{
    const int B1 = (int)uf.size(), R = (int)dets.size() / 8;
    int64_t total = 0;
    w.status = 0;
    for (int g = 0; g < G; ++g) {
        if (cnt[g] < 0 || cnt[g] > top_k) { w.status |= 512; continue; }
        for (int k = 0; k < cnt[g]; ++k) {
            const int r = keep[(size_t)g * top_k + k];
            if (r < 0 || r >= R || r / L2 >= B1) continue;
            if (total < D) {
                w.row[total] = r; w.frame[total] = uf[r / L2]; w.cls[total] = uc[r / L2]; w.group[total] = ug[r / L2];
                w.score[total] = dets[(size_t)r * 8 + 7];
            }
            ++total;
        }
    }
    w.n = total < D ? (int)total : D;
    for (int i = w.n; i < D; ++i) { w.row[i] = -1; w.frame[i] = -1; w.cls[i] = 0; w.group[i] = G; w.score[i] = 0.f; }
    if (total > D) w.status |= 128;
}

static void cand_case(const std::vector<int32_t> &keep, const std::vector<int32_t> &cnt, int G, int top_k, int L2, const std::vector<int32_t> &uf,
                      const std::vector<int32_t> &uc, const std::vector<int32_t> &ug, const std::vector<float> &dets, int D, int want_status,
                      int want_n)
{
    Cands got(D), want(D);
    cand_ref(keep, cnt, G, top_k, L2, uf, uc, ug, dets, D, want);
    const int rc = fcn_cascade_candidates(keep.data(), cnt.data(), G, top_k, L2, uf.data(), uc.data(), ug.data(), (int)uf.size(), dets.data(),
                                          (int)dets.size() / 8, D, got.row.data(), got.frame.data(), got.cls.data(), got.group.data(),
                                          got.score.data(), &got.n, &got.status, nullptr);
    EXPECT(rc == 0);
    EXPECT(got.row == want.row && got.frame == want.frame && got.cls == want.cls && got.group == want.group && got.score == want.score);
    EXPECT(got.n == want.n && got.status == want.status && got.status == want_status && (want_n < 0 || got.n == want_n));
}

// the plan as the contract states it, sequentially
static void plan_ref(const std::vector<int32_t> &cnt, const std::vector<double> &psz, const int32_t *lpad, int D, int S, int B, int64_t cap,
                     std::vector<int32_t> &slot_unit, std::vector<int64_t> &soff, std::vector<int64_t> &off, std::vector<int64_t> &counts,
                     int &n, int &status)
{
    slot_unit.assign(B, D); soff.assign((size_t)D * S + 1, 0); off.assign(B + 1, cap); counts.assign(B, 0);
    n = 0; status = 0;
    int survivors = 0;
    int64_t run = 0;
    for (int d = 0; d < D; ++d) {
        int64_t p = 0;
        for (int s = 0; s < S; ++s) p += cnt[(size_t)d * S + s];
        bool keep = p > 0;
        if (keep) {
            const double w = psz[3 * (size_t)d + 1];
            if (!(w > 0.0 && std::isfinite(w))) { status |= 64; keep = false; }
            else {
                for (int s = 0; s < 4; ++s)
                    if (std::ceil((w / 2.0 - (-w / 2.0)) / STRIDE[s]) > (double)lpad[s]) keep = false;
                if (!keep) status |= 32;
            }
        }
        const bool slot = keep && survivors < B;
        if (keep) ++survivors;
        const int64_t lo = run < cap ? run : cap;
        for (int s = 0; s < S; ++s) {
            soff[(size_t)d * S + s] = run < cap ? run : cap;
            if (slot && cnt[(size_t)d * S + s] > 0) run += cnt[(size_t)d * S + s];
        }
        if (slot) { slot_unit[n] = d; off[n] = lo; counts[n] = (run < cap ? run : cap) - lo; ++n; }
    }
    soff[(size_t)D * S] = run < cap ? run : cap;
    off[B] = soff[(size_t)D * S];
    status |= (survivors > B ? 256 : 0) | (run > cap ? 4 : 0);
}

static void plan_case(const std::vector<int32_t> &cnt, const std::vector<double> &psz, const int32_t *lpad, int D, int S, int B, int64_t cap,
                      int want_status)
{
    std::vector<int32_t> slot_unit(B, -1), wsu;
    std::vector<int64_t> soff((size_t)D * S + 1, -1), off(B + 1, -1), counts(B, -1), wso, woff, wc;
    int32_t n_kept = -1, status = 0;
    int wn, wst;
    plan_ref(cnt, psz, lpad, D, S, B, cap, wsu, wso, woff, wc, wn, wst);
    const int rc = fcn_refine_detect_plan(cnt.data(), psz.data(), STRIDE, lpad, D, S, B, cap, slot_unit.data(), &n_kept, soff.data(),
                                          off.data(), counts.data(), &status, nullptr);
    EXPECT(rc == 0);
    EXPECT(slot_unit == wsu && soff == wso && off == woff && counts == wc && n_kept == wn && status == wst);
    EXPECT(status == want_status);
}

int main()
{
    // ---- the candidate table: exactly sized keep lists, tables and outputs
    {
        const int L2 = 5;
        std::vector<float> dets(20 * 8);
        srand(3);
        for (auto &v : dets) v = (float)(2.0 * unit() - 1.0);
        const std::vector<int32_t> uf = {0, 0, 1, 1}, uc = {2, 0, 1, 1}, ug = {0, 0, 1, 2};
        const std::vector<int32_t> keep = {7, 3, 9, 4, 0, 1, 12, 11, 10, 13, 14, 2, 19, 15, 16, 17, 18, 5};
        cand_case({7, 3, 9, 4, 0, 1}, {4}, 1, 6, L2, uf, uc, ug, dets, 6, 0, 4);           // G = 1
        cand_case(keep, {2, 0, 3}, 3, 6, L2, uf, uc, ug, dets, 8, 0, 5);                  // an empty group
        cand_case(keep, {2, -1, 3}, 3, 6, L2, uf, uc, ug, dets, 8, 512, 5);               // an overflowed one
        cand_case(keep, {2, 7, 3}, 3, 6, L2, uf, uc, ug, dets, 8, 512, 5);                // a count beyond top_k: keep is never read there
        cand_case(keep, {INT32_MAX, 1, INT32_MIN}, 3, 6, L2, uf, uc, ug, dets, 8, 512, 1);
        cand_case(keep, {6, 6, 0}, 3, 6, L2, uf, uc, ug, dets, 12, 0, 12);                // exactly D rows
        cand_case(keep, {6, 6, 0}, 3, 6, L2, uf, uc, ug, dets, 11, 128, 11);              // D + 1 rows
        cand_case(keep, {0, 3, 1}, 3, 6, L2, uf, uc, ug, dets, 1, 128, 1);                // D = 1
        cand_case(keep, {0, 0, 0}, 3, 6, L2, uf, uc, ug, dets, 1, 0, 0);
        {
            std::vector<int32_t> bad(keep);
            bad[1] = 20; bad[6] = -1; bad[14] = INT32_MIN; bad[15] = INT32_MAX;           // entries that are no row of dets
            cand_case(bad, {3, 3, 4}, 3, 6, L2, uf, uc, ug, dets, 8, 0, 6);
            cand_case(keep, {3, 3, 3}, 3, 6, L2, {0, 0, 1}, {2, 0, 1}, {0, 0, 1}, dets, 8, 0, 6);       // B1 = 3: rows >= 15 are nobody's
        }
        for (const int G : {700, 65536}) {                                                // more groups than threads; the largest call
            const int top_k = G == 700 ? 3 : 2, R = 4000, B1 = 790;
            std::vector<float> d2((size_t)R * 8);
            for (auto &v : d2) v = (float)unit();
            std::vector<int32_t> k2((size_t)G * top_k), c2(G), f2(B1), s2(B1), g2(B1);
            for (auto &v : k2) v = rand() % 4006 - 3;
            for (auto &v : c2) v = unit() < (G == 700 ? 0.9 : 0.02) ? rand() % (top_k + 3) - 1 : 0;
            for (int u = 0; u < B1; ++u) { f2[u] = rand() % 9; s2[u] = rand() % 3; g2[u] = rand() % G; }
            cand_case(k2, c2, G, top_k, 5, f2, s2, g2, d2, 2048, 512, -1);
            cand_case(k2, c2, G, top_k, 5, f2, s2, g2, d2, 100, 512 | 128, 100);
        }
        // argument handling: nothing written
        Cands o(8);
        const std::vector<int32_t> cnt = {2, 1, 3};
#define CAND(k_, c_, G_, t_, L_, f_, B_, d_, R_, D_, r_, n_, s_) fcn_cascade_candidates(k_, c_, G_, t_, L_, f_, uc.data(), ug.data(), B_, d_, R_, D_, r_, o.frame.data(), o.cls.data(), o.group.data(), o.score.data(), n_, s_, nullptr)
        EXPECT(CAND(nullptr, cnt.data(), 3, 6, L2, uf.data(), 4, dets.data(), 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), nullptr, 3, 6, L2, uf.data(), 4, dets.data(), 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, nullptr, 4, dets.data(), 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, uf.data(), 4, nullptr, 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, uf.data(), 4, dets.data(), 20, 8, nullptr, &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, uf.data(), 4, dets.data(), 20, 8, o.row.data(), nullptr, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, uf.data(), 4, dets.data(), 20, 8, o.row.data(), &o.n, nullptr) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 0, 6, L2, uf.data(), 4, dets.data(), 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 0, L2, uf.data(), 4, dets.data(), 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, 0, uf.data(), 4, dets.data(), 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, uf.data(), 0, dets.data(), 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, uf.data(), 4, dets.data(), 0, 8, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, uf.data(), 4, dets.data(), 20, 0, o.row.data(), &o.n, &o.status) == FCN_E_BADARG);
        EXPECT(CAND(keep.data(), cnt.data(), 65537, 6, L2, uf.data(), 4, dets.data(), 20, 8, o.row.data(), &o.n, &o.status) == FCN_E_LIMIT);
        EXPECT(CAND(keep.data(), cnt.data(), 3, 6, L2, uf.data(), 4, dets.data(), 20, 2049, o.row.data(), &o.n, &o.status) == FCN_E_LIMIT);
#undef CAND
        EXPECT(o.row[0] == -9 && o.frame[7] == -9 && o.score[0] == -9.f && o.n == -9 && o.status == 0);
    }
    // ---- the plan: exactly sized inputs and outputs
    {
        const int D = 12, S = 3;
        std::vector<int32_t> cnt((size_t)D * S);
        std::vector<double> psz((size_t)D * 3);
        srand(9);
        for (int i = 0; i < D * S; ++i) cnt[i] = 6 + rand() % 900;
        for (int d = 0; d < D; ++d) { psz[3 * d] = 4.0; psz[3 * d + 1] = 0.5 + 2.0 * unit(); psz[3 * d + 2] = 1.5; }
        for (int s = 0; s < S; ++s) { cnt[1 * S + s] = 0; cnt[6 * S + s] = 0; }          // no row between candidates with rows
        int64_t first = 0, total4 = 0, total10 = 0;
        int seen = 0;
        for (int d = 0; d < D; ++d) {
            if (d == 1 || d == 6) continue;
            for (int s = 0; s < S; ++s) { if (seen == 0) first += cnt[d * S + s]; if (seen < 4) total4 += cnt[d * S + s]; total10 += cnt[d * S + s]; }
            ++seen;
        }
        plan_case(cnt, psz, BIG, D, S, 4, 1ll << 40, 256);                    // more survivors than slots: bit 8
        plan_case(cnt, psz, BIG, D, S, 10, 1ll << 40, 0);                     // as many
        plan_case(cnt, psz, BIG, D, S, 12, 1ll << 40, 0);                     // fewer: the normal case, no bit
        plan_case(cnt, psz, BIG, D, S, 4, total4, 256);                       // exactly enough room
        plan_case(cnt, psz, BIG, D, S, 4, total4 - 1, 256 | 4);               // one row short
        plan_case(cnt, psz, BIG, D, S, 10, total10, 0);
        plan_case(cnt, psz, BIG, D, S, 10, total10 - 1, 4);
        plan_case(cnt, psz, BIG, D, S, 4, first + 5, 256 | 4);                // inside the second candidate's first segment
        plan_case(cnt, psz, BIG, D, S, 4, first, 256 | 4);                    // at the boundary behind the first candidate
        plan_case(cnt, psz, BIG, D, S, 12, total10 / 5, 4);
        plan_case(cnt, psz, BIG, D, S, 4, 0, 256 | 4);                        // no room at all
        plan_case(std::vector<int32_t>((size_t)D * S, 0), psz, BIG, D, S, 4, 1000, 0);       // none survives: no bit
        plan_case({7}, {4.0, 1.6, 1.5}, BIG, 1, 1, 1, 100, 0);                // D = S = B = 1
        plan_case({0}, {4.0, 1.6, 1.5}, BIG, 1, 1, 1, 100, 0);
        for (const double w : {0.0, -1.5, (double)NAN, (double)INFINITY}) {   // widths that are no width
            std::vector<double> loud(psz), quiet(psz);
            loud[3 * 4 + 1] = w; quiet[3 * 1 + 1] = w; quiet[3 * 6 + 1] = w;
            plan_case(cnt, psz, BIG, D, S, 10, 1ll << 40, 0);
            plan_case(cnt, loud, BIG, D, S, 10, 1ll << 40, 64);
            plan_case(cnt, quiet, BIG, D, S, 10, 1ll << 40, 0);
        }
        for (int s = 0; s < 4; ++s)                                           // on a window count and one step beyond it
            for (const int k : {1, 3, 8}) {
                double on = k * STRIDE[s];
                while (std::ceil((on / 2.0 - (-on / 2.0)) / STRIDE[s]) > k) on = std::nextafter(on, 0.0);
                for (;;) {
                    const double up = std::nextafter(on, 100.0);
                    if (std::ceil((up / 2.0 - (-up / 2.0)) / STRIDE[s]) > k) break;
                    on = up;
                }
                int32_t lpad[4] = {1 << 20, 1 << 20, 1 << 20, 1 << 20};
                lpad[s] = k;
                plan_case({3, 4}, {4.0, on, 1.5}, lpad, 1, 2, 1, 100, 0);
                plan_case({3, 4}, {4.0, std::nextafter(on, 100.0), 1.5}, lpad, 1, 2, 1, 100, 32);
            }
        {                                                                     // the largest plan, sums beyond 2^31
            int max_u = 0, max_segs = 0;
            EXPECT(fcn_refine_train_plan_limits(&max_u, &max_segs) == 0 && max_u == 2048 && max_segs == 65536);
            const int D2 = max_u, S2 = max_segs / max_u;
            std::vector<int32_t> c2((size_t)D2 * S2);
            std::vector<double> z2((size_t)D2 * 3, 1.6);
            for (int i = 0; i < D2 * S2; ++i) c2[i] = (i / S2) % 3 ? 2000000000 - (rand() % 1000) : 0;
            plan_case(c2, z2, BIG, D2, S2, D2, 1ll << 60, 0);
            plan_case(c2, z2, BIG, D2, S2, 100, 1000, 256 | 4);
        }
        std::vector<int32_t> slot_unit(4, -1);
        std::vector<int64_t> soff((size_t)D * S + 1, -1), off(5, -1), counts(4, -1);
        int32_t n_kept = -1, status = 0;
        const double zero_stride[4] = {0.1, 0.0, 0.4, 0.8};
        const int32_t zero_lpad[4] = {64, 32, 0, 8};
#define PLAN(...) fcn_refine_detect_plan(__VA_ARGS__, nullptr)
#define OUTS slot_unit.data(), &n_kept, soff.data(), off.data(), counts.data(), &status
        EXPECT(PLAN(nullptr, psz.data(), STRIDE, BIG, D, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), nullptr, STRIDE, BIG, D, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), nullptr, BIG, D, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, nullptr, D, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, D, S, 4, 100, nullptr, &n_kept, soff.data(), off.data(), counts.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, D, S, 4, 100, slot_unit.data(), &n_kept, soff.data(), off.data(), counts.data(), nullptr) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, -1, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, D, 0, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, D, S, 0, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, D, S, 4, -1, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), zero_stride, BIG, D, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, zero_lpad, D, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, 2049, S, 4, 100, OUTS) == FCN_E_LIMIT);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, D, S, 2049, 100, OUTS) == FCN_E_LIMIT);
        EXPECT(PLAN(cnt.data(), psz.data(), STRIDE, BIG, D, 5462, 4, 100, OUTS) == FCN_E_LIMIT);
#undef PLAN
#undef OUTS
        EXPECT(slot_unit[0] == -1 && soff[0] == -1 && off[4] == -1 && counts[0] == -1 && n_kept == -1 && status == 0);
    }
    // ---- candidates -> count -> plan -> fill on frames, into point buffers of exactly capacity + 1 rows
    const int seg = fcn_frustum_select_seg();
    for (int ps = 4; ps <= 5; ++ps) {
        const int F = 3, S = 3, B1 = 3, L2 = 2, R = B1 * L2, G = 2, top_k = 4, D = 8;
        const int64_t len[F] = {700, 1, 2 * (int64_t)seg + 100};
        std::vector<int64_t> off(F + 1, 0);
        for (int f = 0; f < F; ++f) off[f + 1] = off[f] + len[f];
        const int64_t n = off[F];
        std::vector<float> pts((size_t)n * ps);
        srand(11);
        for (int64_t i = 0; i < n; ++i) {
            pts[i * ps] = (float)(-4.0 + 8.0 * unit()); pts[i * ps + 1] = (float)(0.0 + 2.0 * unit()); pts[i * ps + 2] = (float)(16.0 + 8.0 * unit());
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = 0.5f;
        }
        const float detv[R][8] = {{0.1f, 1.8f, 20.1f, 6.2f, 3.9f, 1.6f, 0.32f, 0.9f}, {1.4f, 1.7f, 19.1f, 4.1f, 3.0f, 1.5f, 3.1f, 0.8f},
                                  {0.f, 1.8f, 20.f, 9.f, 9.f, 3.f, 0.f, 0.7f}, {30.f, 1.8f, 60.f, 4.f, 2.f, 1.5f, 1.f, 0.5f},
                                  {1.5f, 1.7f, 19.f, 4.f, 3.f, 1.5f, -2.9f, 0.4f}, {0.f, 1.f, 20.f, 30.f, 30.f, 9.f, 0.5f, 0.3f}};
        std::vector<float> dets(R * 8);
        for (int r = 0; r < R; ++r) for (int k = 0; k < 8; ++k) dets[r * 8 + k] = detv[r][k];
        // frustums 0, 1, 2 of frames 0, 1, 2: rows 0, 1 search frame 0, rows 2, 3 the one-row frame, rows 4, 5 the three-segment one
        const std::vector<int32_t> uf = {0, 1, 2}, uc = {0, 1, 2}, ug = {0, 0, 1};
        const std::vector<int32_t> keep = {1, 0, 3, R, 5, 4, -1, -1}, kcnt = {4, 2};       // (R: no row of dets -- skipped)
        Cands c(D);
        EXPECT(fcn_cascade_candidates(keep.data(), kcnt.data(), G, top_k, L2, uf.data(), uc.data(), ug.data(), B1, dets.data(), R, D,
                                      c.row.data(), c.frame.data(), c.cls.data(), c.group.data(), c.score.data(), &c.n, &c.status, nullptr) == 0);
        EXPECT(c.n == 5 && c.status == 0 && c.row == std::vector<int32_t>({1, 0, 3, 5, 4, -1, -1, -1}));
        EXPECT(c.frame == std::vector<int32_t>({0, 0, 1, 2, 2, -1, -1, -1}) && c.group == std::vector<int32_t>({0, 0, 0, 1, 1, 2, 2, 2}));
        // the table as it stands -- three filler candidates -- and two more out-of-range lists
        std::vector<int32_t> scnt((size_t)D * S, -1);
        std::vector<double> pc((size_t)D * 24, -7.0), pa(D, -7.0), psz((size_t)D * 3, -7.0);
#define DCOUNT(p0, cr_, cf_, S_) fcn_refine_detect_count(p0, off.data(), F, ps, dets.data(), R, cr_, cf_, D, 1.2, S_, scnt.data(), pc.data(), pa.data(), psz.data(), nullptr)
#define DFILL(cr_, cf_, so_, o_) fcn_refine_detect_fill(pts.data(), off.data(), F, ps, dets.data(), R, cr_, cf_, D, 1.2, S, so_, o_, nullptr)
        EXPECT(DCOUNT(pts.data(), c.row.data(), c.frame.data(), S) == 0);
        for (int d = 5; d < D; ++d) {
            for (int s = 0; s < S; ++s) EXPECT(scnt[d * S + s] == 0);
            EXPECT(psz[3 * d + 1] == -7.0 && pa[d] == -7.0 && pc[(size_t)d * 24] == -7.0);
        }
        EXPECT(scnt[0 * S] > 10 && scnt[1 * S] > 10 && scnt[0 * S + 1] == 0 && scnt[2 * S] == 0);      // (row 3 is far away: no point)
        for (int s = 0; s < S; ++s) EXPECT(scnt[3 * S + s] > 50 && scnt[4 * S + s] > 0);
        EXPECT(psz[3 * 0 + 1] == 3.0f * 1.2 && psz[3 * 3 + 1] == 30.0 * 1.2);
        {                                                                     // the reading selection counts the same rows
            std::vector<int32_t> whole(5, -1);
            std::vector<double> pc2(5 * 24), pa2(5), ps2(5 * 3);
            EXPECT(fcn_refine_select_count(pts.data(), off.data(), F, ps, dets.data(), R, c.row.data(), c.frame.data(), 5, 1.2, pc2.data(),
                                           pa2.data(), ps2.data(), whole.data(), nullptr) == 0);
            for (int d = 0; d < 5; ++d) EXPECT(whole[d] == scnt[d * S] + scnt[d * S + 1] + scnt[d * S + 2]);
            EXPECT(memcmp(pc2.data(), pc.data(), 5 * 24 * 8) == 0 && memcmp(ps2.data(), psz.data(), 5 * 3 * 8) == 0 && memcmp(pa2.data(), pa.data(), 5 * 8) == 0);
        }
        {
            std::vector<int32_t> brow(c.row), bframe(c.frame), keepc(scnt);
            brow[0] = R; brow[3] = INT32_MIN; bframe[1] = F; bframe[4] = -5;
            EXPECT(DCOUNT(pts.data(), brow.data(), bframe.data(), S) == 0);
            for (int i = 0; i < D * S; ++i) EXPECT(scnt[i] == 0);
            EXPECT(DCOUNT(pts.data(), c.row.data(), c.frame.data(), S) == 0 && scnt == keepc);
        }
        int64_t full[D];
        int64_t all = 0;
        for (int d = 0; d < D; ++d) { full[d] = 0; for (int s = 0; s < S; ++s) full[d] += scnt[d * S + s]; all += full[d]; }
        const int32_t lpad[4] = {1 << 20, 1 << 20, 1 << 20, 1 << 20};
        const struct { int B; int64_t cap; int status; int n; } cases[] = {{2, full[0] + full[1], 256, 2}, {4, all, 0, 4}, {4, all - 1, 4, 4},
            {3, full[0] + 10, 256 | 4, 3}, {8, all + 7, 0, 4}, {4, 1, 4, 4}, {1, full[0], 256, 1}, {8, all / 2, 4, 4}};
        for (const auto &k : cases) {
            std::vector<int32_t> slot_unit(k.B, -1);
            std::vector<int64_t> soff((size_t)D * S + 1, -1), poff(k.B + 1, -1), counts(k.B, -1);
            int32_t n_kept = -1, status = 0;
            EXPECT(fcn_refine_detect_plan(scnt.data(), psz.data(), STRIDE, lpad, D, S, k.B, k.cap, slot_unit.data(), &n_kept, soff.data(),
                                          poff.data(), counts.data(), &status, nullptr) == 0);
            EXPECT(status == k.status && n_kept == k.n && slot_unit[0] == 0 && soff[(size_t)D * S] <= k.cap && poff[k.B] == soff[(size_t)D * S]);
            int64_t stored = 0;
            for (int i = 0; i < k.B; ++i) {
                if (i >= n_kept) EXPECT(slot_unit[i] == D && poff[i] == k.cap && counts[i] == 0);
                else EXPECT(poff[i] + counts[i] <= k.cap && slot_unit[i] != 2);
                stored += counts[i];
            }
            EXPECT(stored == soff[(size_t)D * S]);
            std::vector<float> out((size_t)(k.cap + 1) * ps, -7.f);           // exactly capacity + 1 rows
            EXPECT(DFILL(c.row.data(), c.frame.data(), soff.data(), out.data()) == 0);
            const int64_t end = soff[(size_t)D * S];
            for (int64_t i = 0; i < end; ++i) EXPECT(out[i * ps + 2] >= 15.f && out[i * ps + 2] <= 25.f);
            for (int64_t i = end; i <= k.cap; ++i) EXPECT(out[i * ps] == -7.f);
        }
        // a window count the first candidate's width does not fit: dropped, bit 5
        {
            int32_t lp[4] = {64, 32, 16, 4};                                  // 3 * 1.2 / 0.8: 5 windows
            std::vector<int32_t> slot_unit(4, -1);
            std::vector<int64_t> soff((size_t)D * S + 1, -1), poff(5, -1), counts(4, -1);
            int32_t n_kept = -1, status = 0;
            EXPECT(fcn_refine_detect_plan(scnt.data(), psz.data(), STRIDE, lp, D, S, 4, 1 << 20, slot_unit.data(), &n_kept, soff.data(),
                                          poff.data(), counts.data(), &status, nullptr) == 0);
            EXPECT(status == 32 && n_kept == 0);
        }
        // fewer segments than a frame needs is the caller's duty (no refusal, S segments searched); argument handling
        std::vector<int32_t> keepc(scnt);
        scnt.assign((size_t)D * (S - 1), -1);
        EXPECT(DCOUNT(pts.data(), c.row.data(), c.frame.data(), S - 1) == 0 && scnt[3 * (S - 1)] == keepc[3 * S] && scnt[3 * (S - 1) + 1] == keepc[3 * S + 1]);
        scnt.assign((size_t)D * S, -1);
        EXPECT(DCOUNT(nullptr, c.row.data(), c.frame.data(), S) == FCN_E_BADARG && DCOUNT(pts.data(), nullptr, c.frame.data(), S) == FCN_E_BADARG);
        EXPECT(DCOUNT(pts.data(), c.row.data(), nullptr, S) == FCN_E_BADARG && DCOUNT(pts.data(), c.row.data(), c.frame.data(), 0) == FCN_E_BADARG && scnt[0] == -1);
        std::vector<int64_t> soff((size_t)D * S + 1, 0);
        std::vector<float> out(ps, -7.f);
        EXPECT(DFILL(c.row.data(), c.frame.data(), nullptr, out.data()) == FCN_E_BADARG && DFILL(c.row.data(), c.frame.data(), soff.data(), nullptr) == FCN_E_BADARG);
        EXPECT(DFILL(c.row.data(), c.frame.data(), soff.data(), out.data()) == 0 && out[0] == -7.f);         // every slice empty
#undef DCOUNT
#undef DFILL
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
