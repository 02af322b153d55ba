// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the capturable
// refine-stage training input -- fcn_box3d_jitter_draw, fcn_refine_train_match / _count / _plan / _fill, csrc/refine_plan.h compiled
// for the host against tests/host_harness/hip_emu -- with exactly sized buffers: the jitter draw at one unit, at 64 copies and at
// its 65535 units; the plan with more and fewer survivors than slots, none at all, a capacity inside a segment, at a unit boundary
// and 0, U = S = B = 1, the largest plan, widths that are no width and widths on and one step beyond a window count on each
// stride; count -> plan -> fill on a small scene with out-of-range candidates and a binding capacity (the fill then writes into a
// buffer of exactly capacity + 1 rows); argument handling.  Built with -fsanitize=address,undefined by
// tests/test_refine_plan_sanitizer.py, so a read or write past any buffer is a report, not luck.
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

// the plan as the contract states it, sequentially
static void plan_ref(const std::vector<int32_t> &cnt, const std::vector<int32_t> &pos, const std::vector<double> &psz, const int32_t *lpad,
                     int U, int S, int B, int64_t cap, std::vector<int32_t> &slot_unit, std::vector<int64_t> &soff,
                     std::vector<int64_t> &off, std::vector<int64_t> &counts, int &n, int &status)
{
    slot_unit.assign(B, U); soff.assign((size_t)U * S + 1, 0); off.assign(B + 1, cap); counts.assign(B, 0);
    n = 0; status = 0;
    int survivors = 0;
    int64_t run = 0;
    for (int u = 0; u < U; ++u) {
        int64_t p = 0;
        for (int s = 0; s < S; ++s) p += pos[(size_t)u * S + s];
        bool keep = p > 0;
        if (keep) {
            const double w = psz[3 * (size_t)u + 1];
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
            soff[(size_t)u * S + s] = run < cap ? run : cap;
            if (slot && cnt[(size_t)u * S + s] > 0) run += cnt[(size_t)u * S + s];
        }
        if (slot) { slot_unit[n] = u; off[n] = lo; counts[n] = (run < cap ? run : cap) - lo; ++n; }
    }
    soff[(size_t)U * S] = run < cap ? run : cap;
    off[B] = soff[(size_t)U * S];
    status |= (survivors < B ? 2 : 0) | (run > cap ? 4 : 0);
}

static void plan_case(const std::vector<int32_t> &cnt, const std::vector<int32_t> &pos, const std::vector<double> &psz, const int32_t *lpad,
                      int U, int S, int B, int64_t cap, int want_status)
{
    std::vector<int32_t> slot_unit(B, -1), wsu;
    std::vector<int64_t> soff((size_t)U * S + 1, -1), off(B + 1, -1), counts(B, -1), wso, woff, wc;
    int32_t n_kept = -1, status = 0;
    int wn, wst;
    plan_ref(cnt, pos, psz, lpad, U, S, B, cap, wsu, wso, woff, wc, wn, wst);
    const int rc = fcn_refine_train_plan(cnt.data(), pos.data(), psz.data(), STRIDE, lpad, U, S, B, cap, slot_unit.data(), &n_kept,
                                         soff.data(), off.data(), counts.data(), &status, nullptr);
    EXPECT(rc == 0);
    EXPECT(slot_unit == wsu && soff == wso && off == woff && counts == wc && n_kept == wn && status == wst);
    EXPECT(status == want_status);
}

int main()
{
    // ---- the jitter draw: exactly sized tables
    {
        const struct { int D, A; } shapes[] = {{1, 1}, {1, 64}, {300, 3}, {65535, 1}, {1023, 64}};
        for (const auto &sh : shapes) {
            const size_t n = (size_t)sh.D * sh.A * 7;
            std::vector<double> a(n, -7.0), b(n, -7.0);
            int64_t state = (1ll << 32) + 5;
            EXPECT(fcn_box3d_jitter_draw(sh.D, sh.A, 99, &state, 1, a.data(), nullptr) == 0 && state == (1ll << 32) + 6);
            state = (1ll << 32) + 5;
            EXPECT(fcn_box3d_jitter_draw(sh.D, sh.A, 99, &state, 0, b.data(), nullptr) == 0 && state == (1ll << 32) + 5 && a == b);
            bool in = true;
            for (size_t i = 0; i < n; ++i) in = in && a[i] >= 0.0 && a[i] < 1.0;
            EXPECT(in);
            state = 6;
            EXPECT(fcn_box3d_jitter_draw(sh.D, sh.A, 99, &state, 0, b.data(), nullptr) == 0 && a != b);       // another step
            // the first unit of a larger table is the unit of the smallest one
            std::vector<double> one(7, -7.0);
            EXPECT(fcn_box3d_jitter_draw(1, 1, 99, &state, 0, one.data(), nullptr) == 0 && memcmp(one.data(), b.data(), 56) == 0);
        }
        std::vector<double> t(5 * 3 * 7, -7.0);
        int64_t state = 0;
        EXPECT(fcn_box3d_jitter_draw(0, 3, 99, &state, 1, t.data(), nullptr) == 0 && state == 1 && t[0] == -7.0);
        EXPECT(fcn_box3d_jitter_draw(5, 3, 99, nullptr, 1, t.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box3d_jitter_draw(5, 3, 99, &state, 1, nullptr, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box3d_jitter_draw(-1, 3, 99, &state, 1, t.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box3d_jitter_draw(5, 0, 99, &state, 1, t.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box3d_jitter_draw(5, 65, 99, &state, 1, t.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box3d_jitter_draw(65536, 1, 99, &state, 1, t.data(), nullptr) == FCN_E_LIMIT);
        EXPECT(fcn_box3d_jitter_draw(1024, 64, 99, &state, 1, t.data(), nullptr) == FCN_E_LIMIT);
        EXPECT(state == 1 && t[0] == -7.0);
    }
    // ---- the plan: exactly sized inputs and outputs
    {
        const int U = 12, S = 3;
        std::vector<int32_t> cnt((size_t)U * S), pos((size_t)U * S);
        std::vector<double> psz((size_t)U * 3);
        srand(9);
        for (int i = 0; i < U * S; ++i) { cnt[i] = 6 + rand() % 900; pos[i] = 1 + rand() % 5; }
        for (int u = 0; u < U; ++u) { psz[3 * u] = 4.0; psz[3 * u + 1] = 0.5 + 2.0 * unit(); psz[3 * u + 2] = 1.5; }
        for (int s = 0; s < S; ++s) { pos[1 * S + s] = 0; pos[6 * S + s] = 0; }
        int64_t first = 0, total4 = 0, total10 = 0;
        int seen = 0;
        for (int u = 0; u < U; ++u) {
            if (u == 1 || u == 6) continue;
            for (int s = 0; s < S; ++s) { if (seen == 0) first += cnt[u * S + s]; if (seen < 4) total4 += cnt[u * S + s]; total10 += cnt[u * S + s]; }
            ++seen;
        }
        plan_case(cnt, pos, psz, BIG, U, S, 4, 1ll << 40, 0);                 // more survivors than slots
        plan_case(cnt, pos, psz, BIG, U, S, 10, 1ll << 40, 0);                // as many
        plan_case(cnt, pos, psz, BIG, U, S, 12, 1ll << 40, 2);                // fewer
        plan_case(cnt, pos, psz, BIG, U, S, 4, total4, 0);                    // exactly enough room
        plan_case(cnt, pos, psz, BIG, U, S, 4, total4 - 1, 4);                // one row short
        plan_case(cnt, pos, psz, BIG, U, S, 4, first + 5, 4);                 // inside the second unit's first segment
        plan_case(cnt, pos, psz, BIG, U, S, 4, first, 4);                     // at the boundary behind the first unit
        plan_case(cnt, pos, psz, BIG, U, S, 12, total10 / 5, 6);              // far short and too few
        plan_case(cnt, pos, psz, BIG, U, S, 4, 0, 4);                         // no room at all
        {
            std::vector<int32_t> none((size_t)U * S, 0);
            plan_case(cnt, none, psz, BIG, U, S, 4, 1000, 2);                 // none survives
        }
        plan_case({7}, {2}, {4.0, 1.6, 1.5}, BIG, 1, 1, 1, 100, 0);           // U = S = B = 1
        plan_case({7}, {0}, {4.0, 1.6, 1.5}, BIG, 1, 1, 1, 100, 2);
        // widths that are no width: on units with positives bit 6, on units without none
        for (const double w : {0.0, -1.5, (double)NAN, (double)INFINITY}) {
            std::vector<double> loud(psz), quiet(psz);
            loud[3 * 4 + 1] = w; quiet[3 * 1 + 1] = w; quiet[3 * 6 + 1] = w;
            plan_case(cnt, pos, loud, BIG, U, S, 4, 1ll << 40, 64);
            plan_case(cnt, pos, quiet, BIG, U, S, 4, 1ll << 40, 0);
        }
        {
            std::vector<double> huge(psz);
            huge[3 * 4 + 1] = 1e300;                                          // compared in fp64: no conversion to int
            plan_case(cnt, pos, huge, BIG, U, S, 4, 1ll << 40, 32);
        }
        // on a window count and one step beyond it, on each stride alone
        for (int s = 0; s < 4; ++s)
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
                plan_case({3, 4}, {0, 1}, {4.0, on, 1.5}, lpad, 1, 2, 1, 100, 0);
                plan_case({3, 4}, {0, 1}, {4.0, std::nextafter(on, 100.0), 1.5}, lpad, 1, 2, 1, 100, 32 | 2);
            }
        {                                                                     // 777 units of 5 segments, sums beyond 2^31
            const int U2 = 777, S2 = 5;
            std::vector<int32_t> c2((size_t)U2 * S2), p2((size_t)U2 * S2);
            std::vector<double> z2((size_t)U2 * 3, 1.6);
            for (int i = 0; i < U2 * S2; ++i) { c2[i] = 2000000000 - (rand() % 1000); p2[i] = (i / S2) % 3 ? rand() % 2 : 0; }
            plan_case(c2, p2, z2, BIG, U2, S2, 200, 1ll << 50, 0);
            plan_case(c2, p2, z2, BIG, U2, S2, 777, 1ll << 36, 6);
        }
        {                                                                     // the largest plan
            int max_u = 0, max_segs = 0;
            EXPECT(fcn_refine_train_plan_limits(&max_u, &max_segs) == 0 && max_u == 2048 && max_segs == 65536);
            EXPECT(fcn_refine_train_plan_limits(nullptr, &max_segs) == FCN_E_BADARG);
            const int U2 = max_u, S2 = max_segs / max_u;
            std::vector<int32_t> c2((size_t)U2 * S2), p2((size_t)U2 * S2);
            std::vector<double> z2((size_t)U2 * 3, 1.6);
            for (int i = 0; i < U2 * S2; ++i) { c2[i] = rand() % 50; p2[i] = rand() % 40 == 0; }
            plan_case(c2, p2, z2, BIG, U2, S2, U2, 1ll << 40, 2);
            plan_case(c2, p2, z2, BIG, U2, S2, 100, 1000, 4);
        }
        // argument handling: nothing written
        std::vector<int32_t> slot_unit(4, -1);
        std::vector<int64_t> soff((size_t)U * S + 1, -1), off(5, -1), counts(4, -1);
        int32_t n_kept = -1, status = 0;
        const double zero_stride[4] = {0.1, 0.0, 0.4, 0.8}, nan_stride[4] = {0.1, 0.2, NAN, 0.8};
        const int32_t zero_lpad[4] = {64, 32, 0, 8};
#define PLAN(...) fcn_refine_train_plan(__VA_ARGS__, nullptr)
#define GOOD cnt.data(), pos.data(), psz.data(), STRIDE, BIG
#define OUTS slot_unit.data(), &n_kept, soff.data(), off.data(), counts.data(), &status
        EXPECT(PLAN(nullptr, pos.data(), psz.data(), STRIDE, BIG, U, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), nullptr, psz.data(), STRIDE, BIG, U, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), nullptr, STRIDE, BIG, U, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), psz.data(), nullptr, BIG, U, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), psz.data(), STRIDE, nullptr, U, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, S, 4, 100, nullptr, &n_kept, soff.data(), off.data(), counts.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, S, 4, 100, slot_unit.data(), nullptr, soff.data(), off.data(), counts.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, S, 4, 100, slot_unit.data(), &n_kept, nullptr, off.data(), counts.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, S, 4, 100, slot_unit.data(), &n_kept, soff.data(), nullptr, counts.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, S, 4, 100, slot_unit.data(), &n_kept, soff.data(), off.data(), nullptr, &status) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, S, 4, 100, slot_unit.data(), &n_kept, soff.data(), off.data(), counts.data(), nullptr) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, -1, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, 0, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, S, 0, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, U, S, 4, -1, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), psz.data(), zero_stride, BIG, U, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), psz.data(), nan_stride, BIG, U, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), psz.data(), STRIDE, zero_lpad, U, S, 4, 100, OUTS) == FCN_E_BADARG);
        EXPECT(PLAN(GOOD, 2049, S, 4, 100, OUTS) == FCN_E_LIMIT);
        EXPECT(PLAN(GOOD, U, S, 2049, 100, OUTS) == FCN_E_LIMIT);
        EXPECT(PLAN(GOOD, U, 5462, 4, 100, OUTS) == FCN_E_LIMIT);
#undef PLAN
#undef GOOD
#undef OUTS
        EXPECT(slot_unit[0] == -1 && soff[0] == -1 && off[4] == -1 && counts[0] == -1 && n_kept == -1 && status == 0);
    }
    // ---- match -> jitter draw -> count -> plan -> fill on frames, into buffers of exactly capacity + 1 rows
    const int seg = fcn_frustum_select_seg();
    for (int ps = 4; ps <= 5; ++ps) {
        const int F = 3, S = 3, A = 3, R = 5, G = 3, D = 7, U = D * A;
        const int64_t len[F] = {700, 0, 2 * (int64_t)seg + 100};
        std::vector<int64_t> off(F + 1, 0);
        for (int f = 0; f < F; ++f) off[f + 1] = off[f] + len[f];
        const int64_t n = off[F];
        std::vector<float> pts((size_t)n * ps);
        srand(11);
        for (int64_t i = 0; i < n; ++i) {
            pts[i * ps] = (float)(-4.0 + 8.0 * unit()); pts[i * ps + 1] = (float)(0.0 + 2.0 * unit()); pts[i * ps + 2] = (float)(16.0 + 8.0 * unit());
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = 0.5f;
        }
        const double gtv[G][7] = {{0, 1.8, 20, 6, 4, 1.6, 0.3}, {1.5, 1.7, 19, 4, 3, 1.5, -2.9}, {30, 1.8, 60, 4, 2, 1.5, 1.0}};
        std::vector<double> gt(G * 7);
        for (int j = 0; j < G; ++j) for (int k = 0; k < 7; ++k) gt[j * 7 + k] = gtv[j][k];
        const std::vector<int64_t> goff = {0, 1, 1, 3};                       // frame 0: label 0; frame 2: labels 1, 2
        const float detv[R][8] = {{0.1f, 1.8f, 20.1f, 6.2f, 3.9f, 1.6f, 0.32f, 0.9f}, {1.4f, 1.7f, 19.1f, 4.1f, 3.0f, 1.5f, 3.1f, 0.8f},
                                  {9.f, 1.8f, 30.f, 4.f, 2.f, 1.5f, 0.f, 0.7f}, {30.f, 1.8f, 60.f, 4.f, 2.f, 1.5f, 1.f, 0.5f},
                                  {1.5f, 1.7f, 19.f, 4.f, 3.f, 1.5f, -2.9f, 0.4f}};
        std::vector<float> dets(R * 8);
        for (int r = 0; r < R; ++r) for (int k = 0; k < 8; ++k) dets[r * 8 + k] = detv[r][k];
        // candidates: 0 (frame 0, matches label 0), 1 (frame 2, label 1), 2 (matches nothing), 3 (label 2: far away, no point),
        // 4 (frame 2, label 1), 5: row out of range, 6: frame out of range -- skipped, not reported, never dereferenced
        const std::vector<int32_t> crow = {0, 1, 2, 3, 4, R, 0}, cframe = {0, 2, 2, 2, 2, 0, F};
        std::vector<int32_t> gidx(D, -9);
        std::vector<float> best(D, -9.f);
        EXPECT(fcn_refine_train_match(dets.data(), R, crow.data(), cframe.data(), D, gt.data(), G, goff.data(), F, 0.5, gidx.data(), best.data(), nullptr) == 0);
        EXPECT(gidx[0] == 0 && gidx[1] == 1 && gidx[2] == -1 && gidx[3] == 2 && gidx[4] == 1 && gidx[5] == -1 && gidx[6] == -1 && best[5] == 0.f);
        {                                                                     // the reading entry reports what the no-read one skips
            std::vector<int32_t> g2(D, -9);
            std::vector<float> b2(D, -9.f);
            EXPECT(fcn_refine_match(dets.data(), R, crow.data(), cframe.data(), D, gt.data(), G, goff.data(), F, 0.5, g2.data(), b2.data(), nullptr) == FCN_E_BADARG);
            EXPECT(g2 == gidx && b2 == best);
        }
        std::vector<double> jit((size_t)U * 7, -7.0);
        int64_t state = 4;
        EXPECT(fcn_box3d_jitter_draw(D, A, 17, &state, 1, jit.data(), nullptr) == 0 && state == 5);
        std::vector<int32_t> scnt((size_t)U * S, -1), spos((size_t)U * S, -1);
        std::vector<double> pc((size_t)U * 24, -7.0), pa(U, -7.0), psz((size_t)U * 3, -7.0), gc((size_t)U * 24), gh(U), gs((size_t)U * 3);
#define TCOUNT(p0, cg_, S_) fcn_refine_train_count(p0, off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2, cg_, gt.data(), G, A, jit.data(), 0.05, S_, scnt.data(), spos.data(), pc.data(), pa.data(), psz.data(), gc.data(), gh.data(), gs.data(), nullptr)
#define TFILL(cg_, so_, o_) fcn_refine_train_fill(pts.data(), off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2, cg_, gt.data(), G, A, jit.data(), 0.05, S, so_, o_, nullptr)
        std::vector<int32_t> cgt(gidx);
        cgt[5] = 0; cgt[6] = 0;                                               // a label for the two bad candidates: still skipped
        EXPECT(TCOUNT(pts.data(), cgt.data(), S) == 0);
        for (int u = 5 * A; u < U; ++u) for (int s = 0; s < S; ++s) EXPECT(scnt[u * S + s] == 0 && spos[u * S + s] == 0);
        for (int u = 5 * A; u < U; ++u) EXPECT(psz[3 * u + 1] == -7.0 && pa[u] == -7.0);
        for (int a = 0; a < A; ++a) EXPECT(scnt[a * S] > 10 && spos[a * S] > 5 && psz[3 * a + 1] > 4.0 && psz[3 * (2 * A + a) + 1] == -7.0);
        for (int a = 0; a < A; ++a) for (int s = 0; s < S; ++s) EXPECT(scnt[((1 * A + a) * S) + s] > 0 && spos[((4 * A + a) * S) + s] > 0 && scnt[((3 * A + a) * S) + s] == 0);
        {
            std::vector<int32_t> high(cgt);
            high[4] = G;                                                      // a label row out of range: skipped too
            std::vector<int32_t> keep(scnt);
            EXPECT(TCOUNT(pts.data(), high.data(), S) == 0);
            for (int a = 0; a < A; ++a) for (int s = 0; s < S; ++s) EXPECT(scnt[((4 * A + a) * S) + s] == 0);
            EXPECT(TCOUNT(pts.data(), cgt.data(), S) == 0 && scnt == keep);
        }
        int64_t full[3] = {0, 0, 0};                                          // rows of the first three survivors: units 0, 1, 2
        for (int a = 0; a < 3; ++a) for (int s = 0; s < S; ++s) full[a] += scnt[a * S + s];
        int64_t all = 0;                                                      // the 9 survivors: candidates 0, 1, 4
        for (int u = 0; u < U; ++u) { int64_t p = 0, c = 0; for (int s = 0; s < S; ++s) { p += spos[u * S + s]; c += scnt[u * S + s]; } if (p > 0) all += c; }
        const int32_t lpad[4] = {64, 32, 16, 8};
        const struct { int B; int64_t cap; int status; int n; } cases[] = {{2, full[0] + full[1], 0, 2}, {9, all, 0, 9}, {9, all - 1, 4, 9},
            {3, full[0] + 10, 4, 3}, {12, all + 7, 2, 9}, {4, 1, 4, 4}, {1, full[0], 0, 1}, {12, all / 2, 6, 9}};
        for (const auto &c : cases) {
            std::vector<int32_t> slot_unit(c.B, -1);
            std::vector<int64_t> soff((size_t)U * S + 1, -1), poff(c.B + 1, -1), counts(c.B, -1);
            int32_t n_kept = -1, status = 0;
            EXPECT(fcn_refine_train_plan(scnt.data(), spos.data(), psz.data(), STRIDE, lpad, U, S, c.B, c.cap, slot_unit.data(), &n_kept,
                                         soff.data(), poff.data(), counts.data(), &status, nullptr) == 0);
            EXPECT(status == c.status && n_kept == c.n && slot_unit[0] == 0 && soff[(size_t)U * S] <= c.cap && poff[c.B] == soff[(size_t)U * S]);
            int64_t stored = 0;
            for (int i = 0; i < c.B; ++i) {
                if (i >= n_kept) EXPECT(slot_unit[i] == U && poff[i] == c.cap && counts[i] == 0);
                else EXPECT(poff[i] + counts[i] <= c.cap);
                stored += counts[i];
            }
            EXPECT(stored == soff[(size_t)U * S]);
            std::vector<float> out((size_t)(c.cap + 1) * ps, -7.f);           // exactly capacity + 1 rows
            EXPECT(TFILL(cgt.data(), soff.data(), out.data()) == 0);
            const int64_t end = soff[(size_t)U * S];
            for (int64_t i = 0; i < end; ++i) EXPECT(out[i * ps + 2] >= 15.f && out[i * ps + 2] <= 25.f);
            for (int64_t i = end; i <= c.cap; ++i) EXPECT(out[i * ps] == -7.f);
        }
        // a window count the first candidate's width (6.2 * 1.2 and its jitter) does not fit: its units are dropped, bit 5
        {
            const int32_t tight[4] = {64, 32, 16, 8};
            const double wide_stride[4] = {0.1, 0.2, 0.4, 0.8};
            int32_t lp[4] = {tight[0], tight[1], tight[2], tight[3]};
            lp[3] = 5;                                                        // 4.68 .. 5.2 / 0.8: 6 or 7 windows
            std::vector<int32_t> slot_unit(4, -1);
            std::vector<int64_t> soff((size_t)U * S + 1, -1), poff(5, -1), counts(4, -1);
            int32_t n_kept = -1, status = 0;
            EXPECT(fcn_refine_train_plan(scnt.data(), spos.data(), psz.data(), wide_stride, lp, U, S, 4, 1 << 20, slot_unit.data(), &n_kept,
                                         soff.data(), poff.data(), counts.data(), &status, nullptr) == 0);
            EXPECT(status == 32 && n_kept == 4 && slot_unit[0] == 1 * A);
        }
        // fewer segments than a frame needs is the caller's duty (no refusal, S segments searched); argument handling as the
        // reading entries have it
        std::vector<int32_t> keep(scnt);
        scnt.assign((size_t)U * (S - 1), -1); spos.assign((size_t)U * (S - 1), -1);
        EXPECT(TCOUNT(pts.data(), cgt.data(), S - 1) == 0 && scnt[(1 * A) * (S - 1)] == keep[(1 * A) * S] && scnt[(1 * A) * (S - 1) + 1] == keep[(1 * A) * S + 1]);
        scnt.assign((size_t)U * S, -1); spos.assign((size_t)U * S, -1);
        EXPECT(TCOUNT(nullptr, cgt.data(), S) == FCN_E_BADARG && TCOUNT(pts.data(), nullptr, S) == FCN_E_BADARG && TCOUNT(pts.data(), cgt.data(), 0) == FCN_E_BADARG && scnt[0] == -1);
        std::vector<int64_t> soff((size_t)U * S + 1, 0);
        std::vector<float> out(ps, -7.f);
        EXPECT(TFILL(cgt.data(), nullptr, out.data()) == FCN_E_BADARG && TFILL(cgt.data(), soff.data(), nullptr) == FCN_E_BADARG);
        EXPECT(TFILL(cgt.data(), soff.data(), out.data()) == 0 && out[0] == -7.f);       // every slice empty
        EXPECT(fcn_refine_train_match(nullptr, R, crow.data(), cframe.data(), D, gt.data(), G, goff.data(), F, 0.5, gidx.data(), best.data(), nullptr) == FCN_E_BADARG);
#undef TCOUNT
#undef TFILL
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
