// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the capturable
// inference front -- fcn_frustum_detect_count / _plan / _fill and fcn_frustum_fov_plan, csrc/frustum_detect_plan.h compiled for the
// host against tests/host_harness/hip_emu -- with exactly sized buffers, on the cases that sit on a boundary: n_boxes at, beyond and
// below the table, box frames out of range, more and fewer survivors than slots, the capacity met, one row short (the cut inside a
// segment) and 0, D = S = B1 = 1 and the largest plan; count -> plan -> fill on frames of 4096, 4097 and 0 rows into a point buffer of
// exactly capacity + 1 rows (the spare row stays as it was) against the reading selection; the whole-image plan; argument handling.
// Built with -fsanitize=address,undefined by tests/test_frustum_detect_sanitizer.py, so a read or write past any buffer is a report,
// not luck.
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

// the plan as the contract states it, sequentially
static void plan_ref(const std::vector<int32_t> &cnt, const std::vector<double> &box, const std::vector<int32_t> &frame, int nb, double hthr,
                     double pthr, int D, int S, int B, int64_t cap, int F, std::vector<int32_t> &slot_box, std::vector<int64_t> &soff,
                     std::vector<int64_t> &off, std::vector<int64_t> &counts, int &n, int &status)
{
    slot_box.assign(B, D); soff.assign((size_t)D * S + 1, 0); off.assign(B + 1, cap); counts.assign(B, 0);
    n = 0; status = 0;
    if (nb < 0 || nb > D) { status |= 1024; nb = nb < 0 ? 0 : D; }
    int survivors = 0;
    int64_t run = 0;
    for (int d = 0; d < D; ++d) {
        bool keep = d < nb;
        if (keep && (frame[d] < 0 || frame[d] >= F)) { status |= 1024; keep = false; }
        if (keep) {
            int64_t p = 0;
            for (int s = 0; s < S; ++s) p += cnt[(size_t)d * S + s] > 0 ? cnt[(size_t)d * S + s] : 0;
            const double *q = &box[(size_t)d * 4];
            keep = !(q[3] - q[1] < hthr) && !(q[2] - q[0] < 1.0) && !((double)p < pthr) && p > 0;
        }
        const bool slot = keep && survivors < B;
        if (keep) ++survivors;
        const int64_t lo = run < cap ? run : cap;
        for (int s = 0; s < S; ++s) {
            soff[(size_t)d * S + s] = run < cap ? run : cap;
            if (slot && cnt[(size_t)d * S + s] > 0) run += cnt[(size_t)d * S + s];
        }
        if (slot) { slot_box[n] = d; off[n] = lo; counts[n] = (run < cap ? run : cap) - lo; ++n; }
    }
    soff[(size_t)D * S] = run < cap ? run : cap;
    off[B] = soff[(size_t)D * S];
    status |= (survivors > B ? 256 : 0) | (run > cap ? 4 : 0);
}

static int plan_case(const std::vector<int32_t> &cnt, const std::vector<double> &box, const std::vector<int32_t> &frame, int nb, int D, int S,
                     int B, int64_t cap, int F, int want_status, double hthr = 5.0, double pthr = 1.0)
{
    std::vector<int32_t> slot_box(B, -1), wsb;
    std::vector<int64_t> soff((size_t)D * S + 1, -1), off(B + 1, -1), counts(B, -1), wso, woff, wc;
    std::vector<int32_t> nbv(1, nb);
    int32_t n_kept = -1, status = 0;
    int wn, wst;
    plan_ref(cnt, box, frame, nb, hthr, pthr, D, S, B, cap, F, wsb, wso, woff, wc, wn, wst);
    const int rc = fcn_frustum_detect_plan(cnt.data(), box.data(), frame.data(), nbv.data(), hthr, pthr, D, S, B, cap, F, slot_box.data(),
                                           &n_kept, soff.data(), off.data(), counts.data(), &status, nullptr);
    EXPECT(rc == 0);
    EXPECT(slot_box == wsb && soff == wso && off == woff && counts == wc && n_kept == wn && status == wst);
    EXPECT(status == want_status);
    return n_kept;
}

int main()
{
    // ---- the plan on its boundaries: exactly sized counts, boxes, frames and outputs
    {
        const int D = 6, S = 2, F = 2;
        const std::vector<int32_t> cnt = {3, 0, 0, 0, 2, 5, 4, 4, 1, 1, 9, 9};
        std::vector<double> box;
        for (int d = 0; d < D; ++d) { box.push_back(10.0); box.push_back(20.0); box.push_back(110.0); box.push_back(d == 3 ? 24.0 : 90.0); }
        const std::vector<int32_t> frame = {0, 1, 1, 0, 1, 0};
        EXPECT(plan_case(cnt, box, frame, D, D, S, 6, 100, F, 0) == 4);                   // boxes 1 (no row) and 3 (4 px) are out
        EXPECT(plan_case(cnt, box, frame, D, D, S, 4, 100, F, 0) == 4);                   // exactly B1 survivors
        EXPECT(plan_case(cnt, box, frame, D, D, S, 3, 100, F, 256) == 3);                 // B1 + 1
        EXPECT(plan_case(cnt, box, frame, 0, D, S, 3, 100, F, 0) == 0);                   // n_boxes = 0: every slot at the spare row
        EXPECT(plan_case(cnt, box, frame, D + 1, D, S, 6, 100, F, 1024) == 4);            // beyond the table: row D is never read
        EXPECT(plan_case(cnt, box, frame, INT32_MAX, D, S, 6, 100, F, 1024) == 4);
        EXPECT(plan_case(cnt, box, frame, -1, D, S, 6, 100, F, 1024) == 0);
        EXPECT(plan_case(cnt, box, frame, INT32_MIN, D, S, 6, 100, F, 1024) == 0);
        EXPECT(plan_case(cnt, box, frame, 3, D, S, 6, 100, F, 0) == 2);
        for (int32_t f : {-1, 2, INT32_MIN, INT32_MAX}) {
            std::vector<int32_t> bad(frame);
            bad[2] = f;
            EXPECT(plan_case(cnt, box, bad, D, D, S, 6, 100, F, 1024) == 3);
            EXPECT(plan_case(cnt, box, bad, 2, D, S, 6, 100, F, 0) == 1);                 // beyond n_boxes it is nobody's business
        }
        EXPECT(plan_case(cnt, box, frame, D, D, S, 6, 30, F, 0) == 4);                    // 3 + 7 + 2 + 18 = 30: exactly met
        EXPECT(plan_case(cnt, box, frame, D, D, S, 6, 29, F, 4) == 4);                    // one row short
        EXPECT(plan_case(cnt, box, frame, D, D, S, 6, 4, F, 4) == 4);                     // the cut inside box 2's first segment
        EXPECT(plan_case(cnt, box, frame, D, D, S, 6, 0, F, 4) == 4);
        EXPECT(plan_case({7}, {0.0, 0.0, 9.0, 5.0}, {0}, 1, 1, 1, 1, 100, 1, 0) == 1);    // D = S = B1 = 1, height == threshold
        EXPECT(plan_case({7}, {0.0, 0.0, 9.0, std::nextafter(5.0, 0.0)}, {0}, 1, 1, 1, 1, 100, 1, 0) == 0);
        EXPECT(plan_case({7}, {0.0, 0.0, 1.0, 9.0}, {0}, 1, 1, 1, 1, 100, 1, 0) == 1);    // width exactly 1
        EXPECT(plan_case({7}, {0.0, 0.0, 9.0, 9.0}, {0}, 1, 1, 1, 1, 100, 1, 0, 5.0, 7.0) == 1);
        EXPECT(plan_case({6}, {0.0, 0.0, 9.0, 9.0}, {0}, 1, 1, 1, 1, 100, 1, 0, 5.0, 7.0) == 0);
        EXPECT(plan_case({0}, {0.0, 0.0, 9.0, 9.0}, {0}, 1, 1, 1, 1, 100, 1, 0, 5.0, 0.0) == 0);
    }
    {
        int max_d = 0, max_segs = 0;
        EXPECT(fcn_frustum_detect_plan_limits(&max_d, &max_segs) == 0 && max_d == 2048 && max_segs == 65536);
        EXPECT(fcn_frustum_detect_plan_limits(nullptr, &max_segs) == 10001);
        const int D = max_d, S = max_segs / max_d;
        srand(5);
        std::vector<int32_t> cnt((size_t)D * S), frame(D);
        std::vector<double> box;
        for (int d = 0; d < D; ++d) {
            const bool rows = unit() < 0.6;
            for (int s = 0; s < S; ++s) cnt[(size_t)d * S + s] = rows ? (int)(unit() * 50) : 0;
            frame[d] = (int)(unit() * 11) - 1;                                              // -1 .. 9 of F = 9
            box.push_back(0.0); box.push_back(0.0); box.push_back(50.0); box.push_back(d % 7 ? 40.0 : 2.0);
        }
        plan_case(cnt, box, frame, D, D, S, D, (int64_t)1 << 40, 9, 1024);
        plan_case(cnt, box, frame, D - 3, D, S, 300, 9000, 9, 1024 | 256 | 4);
    }
    // ---- count -> plan -> fill on frames of 4096, 4097 and 0 rows: V2C = R0 = identity, a pinhole P
    {
        const int F = 3, ps = 4, S = 2, D = 7;
        const int64_t len[3] = {4096, 4097, 0};
        const std::vector<int64_t> foff = {0, 4096, 8193, 8193};
        std::vector<float> pts((size_t)8193 * ps);
        srand(9);
        for (size_t i = 0; i < pts.size() / ps; ++i) {                                     // velodyne x is the clip distance's axis
            pts[i * ps] = (float)(3.0 + 40.0 * unit()); pts[i * ps + 1] = (float)(-8.0 + 16.0 * unit());
            pts[i * ps + 2] = (float)(5.0 + 40.0 * unit()); pts[i * ps + 3] = (float)unit();
        }
        (void)len;
        std::vector<double> P, V2C, R0, wh;
        for (int f = 0; f < F; ++f) {
            const double p[12] = {700, 0, 600, 40, 0, 700, 180, 2, 0, 0, 1, 0.003}, v[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            const double r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            P.insert(P.end(), p, p + 12); V2C.insert(V2C.end(), v, v + 12); R0.insert(R0.end(), r, r + 9);
            wh.push_back(1242.0); wh.push_back(375.0);
        }
        // whole image and an inner box per frame, and a seventh that the table's n_boxes = 6 leaves out
        std::vector<double> boxes;
        for (int d = 0; d < D; ++d) {
            const double whole[4] = {-50, -50, 1300, 430}, inner[4] = {600.25, 100.5, 1000.75, 300.0};
            boxes.insert(boxes.end(), d % 2 ? inner : whole, (d % 2 ? inner : whole) + 4);
        }
        const std::vector<int32_t> bframe = {0, 0, 1, 1, 2, 2, 0};
        // the reading selection over all seven boxes
        std::vector<double> wbox(D * 4, -9.0), wang(D, -9.0);
        std::vector<int32_t> wcnt((size_t)D * S, -9);
        EXPECT(fcn_frustum_select_count(pts.data(), foff.data(), F, ps, P.data(), V2C.data(), R0.data(), wh.data(), boxes.data(), bframe.data(),
                                        D, S, 1, 2.0, wbox.data(), wang.data(), wcnt.data(), nullptr) == 0);
        EXPECT(wcnt[0] > 300 && wcnt[1] == 0 && wcnt[4] > 300 && wcnt[5] <= 1 && wcnt[8] == 0 && wcnt[12] == wcnt[0]);
        for (int32_t nb : {6, 7, 9, 0, -4}) {
            for (int bad = 0; bad < 3; ++bad) {                                            // box 2's frame: as it is, F, -1
                std::vector<int32_t> bf(bframe);
                if (bad) bf[2] = bad == 1 ? F : -1;
                const std::vector<int32_t> nbv(1, nb);
                std::vector<double> box2d(D * 4, -9.0), ang(D, -9.0);
                std::vector<int32_t> cnt((size_t)D * S, -9);
                EXPECT(fcn_frustum_detect_count(pts.data(), foff.data(), F, ps, P.data(), V2C.data(), R0.data(), wh.data(), boxes.data(),
                                                bf.data(), D, S, 1, 2.0, nbv.data(), box2d.data(), ang.data(), cnt.data(), nullptr) == 0);
                for (int d = 0; d < D; ++d) {
                    const bool dead = d >= nb || (bad && d == 2);
                    for (int s = 0; s < S; ++s) EXPECT(cnt[(size_t)d * S + s] == (dead ? 0 : wcnt[(size_t)d * S + s]));
                    EXPECT(dead ? (box2d[d * 4] == -9.0 && ang[d] == -9.0)
                                : (memcmp(&box2d[d * 4], &wbox[d * 4], 32) == 0 && memcmp(&ang[d], &wang[d], 8) == 0));
                }
                int64_t total = 0;
                for (int d = 0; d < D; ++d) total += cnt[(size_t)d * S] + cnt[(size_t)d * S + 1];
                for (int64_t cap : {total, total - 1, total / 2, (int64_t)0}) {
                    if (cap < 0) continue;
                    const int B = 5;
                    std::vector<int32_t> slot_box(B, -1);
                    std::vector<int64_t> soff((size_t)D * S + 1, -1), off(B + 1, -1), counts(B, -1);
                    int32_t n_kept = -1, status = 0;
                    EXPECT(fcn_frustum_detect_plan(cnt.data(), box2d.data(), bf.data(), nbv.data(), 5.0, 1.0, D, S, B, cap, F, slot_box.data(),
                                                   &n_kept, soff.data(), off.data(), counts.data(), &status, nullptr) == 0);
                    const int want_bits = ((nb > D || nb < 0) ? 1024 : 0) | ((bad && nb > 2) ? 1024 : 0) | (cap < total ? 4 : 0);
                    EXPECT(status == want_bits && soff[(size_t)D * S] == cap && off[B] == cap);
                    // exactly capacity + 1 rows: the spare row behind the buffer is read by an empty slot, never written
                    std::vector<float> out((size_t)(cap + 1) * ps, -9.f);
                    EXPECT(fcn_frustum_detect_fill(pts.data(), foff.data(), F, ps, P.data(), V2C.data(), R0.data(), wh.data(), boxes.data(),
                                                   bf.data(), D, S, 1, 2.0, nbv.data(), soff.data(), out.data(), nullptr) == 0);
                    for (int k = 0; k < ps; ++k) EXPECT(out[(size_t)cap * ps + k] == -9.f);
                    int64_t stored = 0;
                    for (int b = 0; b < B; ++b) {
                        stored += counts[b];
                        EXPECT(b < n_kept ? (slot_box[b] < D && off[b] + counts[b] <= cap) : (slot_box[b] == D && off[b] == cap && counts[b] == 0));
                    }
                    EXPECT(stored == cap);
                    for (int64_t i = 0; i < cap * ps; ++i)
                        if (out[i] == -9.f) { EXPECT(out[i] != -9.f); break; }             // every granted row is written
                }
            }
        }
        // ---- the whole-image plan: one box per frame, every frame live, no clipping
        {
            std::vector<double> fb;
            for (int f = 0; f < F; ++f) { fb.push_back(0.0); fb.push_back(0.0); fb.push_back(1242.0); fb.push_back(375.0); }
            const std::vector<int32_t> ff = {0, 1, 2}, nf(1, F);
            std::vector<double> box2d(F * 4, -9.0), ang(F, -9.0);
            std::vector<int32_t> cnt((size_t)F * S, -9);
            EXPECT(fcn_frustum_detect_count(pts.data(), foff.data(), F, ps, P.data(), V2C.data(), R0.data(), wh.data(), fb.data(), ff.data(), F,
                                            S, 0, 2.0, nf.data(), box2d.data(), ang.data(), cnt.data(), nullptr) == 0);
            std::vector<int64_t> soff((size_t)F * S + 1, -1), fo(F + 1, -1);
            const int64_t rows = 8193;
            EXPECT(fcn_frustum_fov_plan(cnt.data(), F, S, rows, soff.data(), fo.data(), nullptr) == 0);
            int64_t run = 0;
            for (int i = 0; i < F * S; ++i) { EXPECT(soff[i] == run); if (i % S == 0) EXPECT(fo[i / S] == run); run += cnt[i]; }
            EXPECT(soff[(size_t)F * S] == run && fo[F] == run && run <= rows && run > 600 && fo[2] == fo[3]);
            std::vector<float> out((size_t)run * ps, -9.f);                                // exactly the subset's rows
            EXPECT(fcn_frustum_detect_fill(pts.data(), foff.data(), F, ps, P.data(), V2C.data(), R0.data(), wh.data(), fb.data(), ff.data(), F,
                                           S, 0, 2.0, nf.data(), soff.data(), out.data(), nullptr) == 0);
            EXPECT(fcn_frustum_fov_plan(cnt.data(), F, S, 10, soff.data(), fo.data(), nullptr) == 0 && soff[(size_t)F * S] == 10 && fo[1] == 10);
            EXPECT(fcn_frustum_fov_plan(nullptr, F, S, rows, soff.data(), fo.data(), nullptr) == 10001);
            EXPECT(fcn_frustum_fov_plan(cnt.data(), F, 0, rows, soff.data(), fo.data(), nullptr) == 10001);
            EXPECT(fcn_frustum_fov_plan(cnt.data(), 65536, 2, rows, soff.data(), fo.data(), nullptr) == 10002);
        }
        // ---- argument handling
        {
            const std::vector<int32_t> nbv(1, D);
            std::vector<int32_t> cnt((size_t)D * S, -9), slot_box(4, -9);
            std::vector<int64_t> soff((size_t)D * S + 1, 0), off(5, -9), counts(4, -9);
            int32_t n_kept = -9, status = -9;
            EXPECT(fcn_frustum_detect_count(pts.data(), foff.data(), F, ps, P.data(), V2C.data(), R0.data(), wh.data(), boxes.data(), bframe.data(),
                                            D, S, 1, 2.0, nullptr, wbox.data(), wang.data(), cnt.data(), nullptr) == 10001);
            EXPECT(fcn_frustum_detect_fill(pts.data(), foff.data(), F, ps, P.data(), V2C.data(), R0.data(), wh.data(), boxes.data(), bframe.data(),
                                           D, S, 1, 2.0, nullptr, soff.data(), pts.data(), nullptr) == 10001);
            EXPECT(fcn_frustum_detect_count(pts.data(), foff.data(), F, 2, P.data(), V2C.data(), R0.data(), wh.data(), boxes.data(), bframe.data(),
                                            D, S, 1, 2.0, nbv.data(), wbox.data(), wang.data(), cnt.data(), nullptr) == 10001);
            EXPECT(fcn_frustum_detect_plan(cnt.data(), wbox.data(), bframe.data(), nullptr, 5.0, 1.0, D, S, 4, 100, F, slot_box.data(), &n_kept,
                                           soff.data(), off.data(), counts.data(), &status, nullptr) == 10001);
            EXPECT(fcn_frustum_detect_plan(cnt.data(), wbox.data(), bframe.data(), nbv.data(), 5.0, 1.0, 2049, S, 4, 100, F, slot_box.data(),
                                           &n_kept, soff.data(), off.data(), counts.data(), &status, nullptr) == 10002);
            EXPECT(fcn_frustum_detect_plan(cnt.data(), wbox.data(), bframe.data(), nbv.data(), NAN, 1.0, D, S, 4, 100, F, slot_box.data(), &n_kept,
                                           soff.data(), off.data(), counts.data(), &status, nullptr) == 10001);
            EXPECT(cnt[0] == -9 && slot_box[0] == -9 && n_kept == -9 && status == -9 && off[0] == -9);
        }
    }
    if (!fails) printf("all ok\n");
    return fails ? 1 : 0;
}
