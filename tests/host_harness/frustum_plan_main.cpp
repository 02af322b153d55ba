// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the capturable
// first-stage training input -- fcn_box2d_perturb, fcn_frustum_train_count / _plan / _fill, csrc/frustum_plan.h compiled for the
// host against tests/host_harness/hip_emu -- with exactly sized buffers: more boxes than one workgroup's lanes, a box beyond the
// image and frames out of range, the plan with more and fewer survivors than slots, none at all, a capacity one row and far
// short (the fill then writes into a buffer of exactly capacity + 1 rows), B = D = 1, the largest plan, argument handling.
// Built with -fsanitize=address,undefined by tests/test_frustum_plan_sanitizer.py, so a read or write past any buffer is a
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

// the plan as the contract states it, sequentially
static void plan_ref(const std::vector<int32_t> &cnt, const std::vector<int32_t> &pos, const std::vector<double> &gt2d, double min_h,
                     int D, int S, int B, int64_t cap, std::vector<int32_t> &slot_box, std::vector<int64_t> &soff,
                     std::vector<int64_t> &off, int &n, int &status)
{
    slot_box.assign(B, 0); soff.assign((size_t)D * S + 1, 0); off.assign(B + 1, 0);
    n = 0;
    int survivors = 0;
    int64_t run = 0;
    for (int d = 0; d < D; ++d) {
        int64_t p = 0;
        for (int s = 0; s < S; ++s) p += pos[(size_t)d * S + s];
        const bool keep = !(gt2d[4 * d + 3] - gt2d[4 * d + 1] < min_h) && p > 0;
        const bool slot = keep && survivors < B;
        if (keep) ++survivors;
        if (slot) { slot_box[n] = d; off[n] = run < cap ? run : cap; ++n; }
        for (int s = 0; s < S; ++s) {
            soff[(size_t)d * S + s] = run < cap ? run : cap;
            if (slot && cnt[(size_t)d * S + s] > 0) run += cnt[(size_t)d * S + s];
        }
    }
    soff[(size_t)D * S] = run < cap ? run : cap;
    for (int i = n; i <= B; ++i) off[i] = soff[(size_t)D * S];
    status = (survivors < B ? 2 : 0) | (run > cap ? 4 : 0);
}

static void plan_case(const std::vector<int32_t> &cnt, const std::vector<int32_t> &pos, const std::vector<double> &gt2d, double min_h,
                      int D, int S, int B, int64_t cap, int want_status)
{
    std::vector<int32_t> slot_box(B, -1), wsb;
    std::vector<int64_t> soff((size_t)D * S + 1, -1), off(B + 1, -1), wso, woff;
    int32_t n_kept = -1, status = 0;
    int wn, wst;
    plan_ref(cnt, pos, gt2d, min_h, D, S, B, cap, wsb, wso, woff, wn, wst);
    const int rc = fcn_frustum_train_plan(cnt.data(), pos.data(), gt2d.data(), min_h, D, S, B, cap, slot_box.data(), soff.data(),
                                          off.data(), &n_kept, &status, nullptr);
    EXPECT(rc == 0);
    EXPECT(slot_box == wsb && soff == wso && off == woff && n_kept == wn && status == wst);
    EXPECT(status == want_status);
}

int main()
{
    // ---- perturb: 300 boxes (two workgroups), exactly sized; box 4 beyond the image, boxes 2 and 7 with frames out of range
    {
        int T = 0;
        EXPECT(fcn_box2d_perturb_limits(&T) == 0 && T == 32);
        EXPECT(fcn_box2d_perturb_limits(nullptr) == FCN_E_BADARG);
        const int D = 300, F = 2;
        std::vector<double> boxes((size_t)D * 4), out((size_t)D * 4, -7.0), wh = {1242, 375, 1224, 370};
        std::vector<int32_t> bframe(D);
        srand(5);
        for (int d = 0; d < D; ++d) {
            const double x0 = 1000.0 * rand() / RAND_MAX, y0 = 250.0 * rand() / RAND_MAX;
            boxes[4 * d] = x0; boxes[4 * d + 1] = y0; boxes[4 * d + 2] = x0 + 5 + 180.0 * rand() / RAND_MAX; boxes[4 * d + 3] = y0 + 5 + 100.0 * rand() / RAND_MAX;
            bframe[d] = d % 2;
        }
        boxes[16] = 1300; boxes[17] = 100; boxes[18] = 1400; boxes[19] = 200;
        bframe[2] = -1; bframe[7] = F;
        int64_t state = 3;
        int32_t status = 0;
        int rc = fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), D, F, 0.1, 99, &state, 1, out.data(), &status, nullptr);
        EXPECT(rc == 0 && state == 4 && status == 16);
        for (int d = 0; d < D; ++d) {
            const bool failed = d == 2 || d == 4 || d == 7;
            const double W = wh[2 * (d % 2)], H = wh[2 * (d % 2) + 1];
            if (failed) EXPECT(memcmp(&out[4 * d], &boxes[4 * d], 32) == 0);
            else EXPECT(out[4 * d] < out[4 * d + 2] && out[4 * d + 1] < out[4 * d + 3] && out[4 * d] >= 0 && out[4 * d + 2] <= W - 1 &&
                        out[4 * d + 1] >= 0 && out[4 * d + 3] <= H - 1 && memcmp(&out[4 * d], &boxes[4 * d], 32) != 0);
        }
        std::vector<double> again((size_t)D * 4, -7.0);
        state = 3; status = 0;
        rc = fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), D, F, 0.1, 99, &state, 0, again.data(), &status, nullptr);
        EXPECT(rc == 0 && state == 3 && again == out);                        // the same step, the same boxes; no advance
        state = (1ll << 32) + 5;
        rc = fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), 1, F, 0.1, 99, &state, 1, again.data(), &status, nullptr);
        EXPECT(rc == 0 && state == (1ll << 32) + 6 && again[0] != out[0] && again[4] == out[4]);       // D = 1: one row written
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), 0, F, 0.1, 99, &state, 1, again.data(), &status, nullptr) == 0);
        EXPECT(state == (1ll << 32) + 7);
        EXPECT(fcn_box2d_perturb(nullptr, bframe.data(), wh.data(), D, F, 0.1, 99, &state, 1, out.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), nullptr, wh.data(), D, F, 0.1, 99, &state, 1, out.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), nullptr, D, F, 0.1, 99, &state, 1, out.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), D, F, 0.1, 99, nullptr, 1, out.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), D, F, 0.1, 99, &state, 1, nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), D, F, 0.1, 99, &state, 1, out.data(), nullptr, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), -1, F, 0.1, 99, &state, 1, out.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), D, F, 1.0, 99, &state, 1, out.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), D, F, -0.5, 99, &state, 1, out.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb(boxes.data(), bframe.data(), wh.data(), D, F, NAN, 99, &state, 1, out.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(state == (1ll << 32) + 7);
    }
    // ---- plan: exactly sized inputs and outputs
    {
        const int D = 12, S = 3;
        std::vector<int32_t> cnt((size_t)D * S), pos((size_t)D * S);
        std::vector<double> gt2d((size_t)D * 4);
        srand(9);
        for (int i = 0; i < D * S; ++i) { cnt[i] = rand() % 900; pos[i] = cnt[i] < 30 ? cnt[i] : rand() % 30; }
        for (int d = 0; d < D; ++d) { gt2d[4 * d] = 0; gt2d[4 * d + 1] = 10; gt2d[4 * d + 2] = 50; gt2d[4 * d + 3] = 10 + 30 + d; }
        for (int s = 0; s < S; ++s) { pos[1 * S + s] = 0; pos[6 * S + s] = 0; }
        pos[4 * S] = 3; gt2d[4 * 4 + 3] = 10 + 24.5;                          // fails the height rule alone
        int64_t total4 = 0, total9 = 0;
        int seen = 0;
        for (int d = 0; d < D; ++d) {
            if (d == 1 || d == 4 || d == 6) continue;
            for (int s = 0; s < S; ++s) { if (seen < 4) total4 += cnt[d * S + s]; total9 += cnt[d * S + s]; }
            ++seen;
        }
        plan_case(cnt, pos, gt2d, 25.0, D, S, 4, 1ll << 40, 0);               // more survivors than slots
        plan_case(cnt, pos, gt2d, 25.0, D, S, 12, 1ll << 40, 2);              // fewer
        plan_case(cnt, pos, gt2d, 25.0, D, S, 4, total4, 0);                  // exactly enough room
        plan_case(cnt, pos, gt2d, 25.0, D, S, 4, total4 - 1, 4);              // one row short
        plan_case(cnt, pos, gt2d, 25.0, D, S, 12, total9 / 5, 6);             // far short and too few
        plan_case(cnt, pos, gt2d, 25.0, D, S, 4, 0, 4);                       // no room at all
        plan_case(cnt, pos, gt2d, 1000.0, D, S, 4, 1ll << 40, 2);             // none survives
        plan_case(cnt, pos, gt2d, 24.0, D, S, 12, 1ll << 40, 2);              // box 4 passes the height rule now
        plan_case({7}, {2}, {0, 0, 10, 40}, 25.0, 1, 1, 1, 100, 0);           // B = D = 1
        plan_case({7}, {0}, {0, 0, 10, 40}, 25.0, 1, 1, 1, 100, 2);
        {                                                                     // 777 boxes of 5 segments, sums beyond 2^31
            const int D2 = 777, S2 = 5;
            std::vector<int32_t> c2((size_t)D2 * S2), p2((size_t)D2 * S2);
            std::vector<double> g2((size_t)D2 * 4);
            for (int i = 0; i < D2 * S2; ++i) { c2[i] = 2000000000 - (rand() % 1000); p2[i] = (i / S2) % 3 ? rand() % 2 : 0; }
            for (int d = 0; d < D2; ++d) { g2[4 * d] = 0; g2[4 * d + 1] = 0; g2[4 * d + 2] = 9; g2[4 * d + 3] = 10 + rand() % 60; }
            plan_case(c2, p2, g2, 25.0, D2, S2, 200, 1ll << 50, 0);
            plan_case(c2, p2, g2, 25.0, D2, S2, 777, 1ll << 36, 6);
        }
        {                                                                     // the largest plan
            int max_d = 0, max_segs = 0;
            EXPECT(fcn_frustum_train_plan_limits(&max_d, &max_segs) == 0 && max_d == 2048 && max_segs == 65536);
            EXPECT(fcn_frustum_train_plan_limits(nullptr, &max_segs) == FCN_E_BADARG);
            const int D2 = max_d, S2 = max_segs / max_d;
            std::vector<int32_t> c2((size_t)D2 * S2), p2((size_t)D2 * S2);
            std::vector<double> g2((size_t)D2 * 4);
            for (int i = 0; i < D2 * S2; ++i) { c2[i] = rand() % 50; p2[i] = rand() % 40 == 0; }
            for (int d = 0; d < D2; ++d) { g2[4 * d] = 0; g2[4 * d + 1] = 0; g2[4 * d + 2] = 9; g2[4 * d + 3] = 10 + rand() % 60; }
            plan_case(c2, p2, g2, 25.0, D2, S2, D2, 1ll << 40, 2);
        }
        // argument handling: nothing written
        std::vector<int32_t> slot_box(4, -1);
        std::vector<int64_t> soff((size_t)D * S + 1, -1), off(5, -1);
        int32_t n_kept = -1, status = 0;
#define PLAN(c_, p_, g_, D_, S_, B_, cap_, sb_, so_, of_, nk_, st_) fcn_frustum_train_plan(c_, p_, g_, 25.0, D_, S_, B_, cap_, sb_, so_, of_, nk_, st_, nullptr)
        EXPECT(PLAN(nullptr, pos.data(), gt2d.data(), D, S, 4, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), nullptr, gt2d.data(), D, S, 4, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), nullptr, D, S, 4, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, S, 4, 100, nullptr, soff.data(), off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, S, 4, 100, slot_box.data(), nullptr, off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, S, 4, 100, slot_box.data(), soff.data(), nullptr, &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, S, 4, 100, slot_box.data(), soff.data(), off.data(), nullptr, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, S, 4, 100, slot_box.data(), soff.data(), off.data(), &n_kept, nullptr) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), -1, S, 4, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, 0, 4, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, S, 0, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, S, 4, -1, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), 2049, S, 4, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_LIMIT);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, S, 2049, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_LIMIT);
        EXPECT(PLAN(cnt.data(), pos.data(), gt2d.data(), D, 5462, 4, 100, slot_box.data(), soff.data(), off.data(), &n_kept, &status) == FCN_E_LIMIT);
#undef PLAN
        EXPECT(slot_box[0] == -1 && soff[0] == -1 && off[4] == -1 && n_kept == -1 && status == 0);
    }
    // ---- count -> plan -> fill on frames, into buffers of exactly capacity + 1 rows
    const int seg = fcn_frustum_select_seg();
    const double Pm[12] = {721.5377, 0, 609.5593, 44.85728, 0, 721.5377, 172.854, 0.2163791, 0, 0, 1, 0.002745884};
    const double Vm[12] = {0.007533745, -0.9999714, -0.000616602, -0.004069766, 0.01480249, 0.0007280733, -0.9998902, -0.07631618,
                           0.9998621, 0.00752379, 0.01480755, -0.2717806};
    const double Rm[9] = {0.9999239, 0.00983776, -0.007445048, -0.009869795, 0.9999421, -0.004278459, 0.007402527, 0.004351614, 0.9999631};
    for (int ps = 4; ps <= 5; ++ps) {
        const int F = 2, D = 6, S = 3;
        const int64_t len[F] = {5000, 2 * (int64_t)seg + 808};
        std::vector<int64_t> foff(F + 1, 0);
        for (int f = 0; f < F; ++f) foff[f + 1] = foff[f] + len[f];
        const int64_t n = foff[F];
        std::vector<float> pts((size_t)n * ps);
        srand(7);
        for (int64_t i = 0; i < n; ++i) {
            pts[i * ps] = 3.f + 40.f * rand() / RAND_MAX; pts[i * ps + 1] = -12.f + 24.f * rand() / RAND_MAX; pts[i * ps + 2] = -2.5f + 3.5f * rand() / RAND_MAX;
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = 0.5f;
        }
        std::vector<double> P(F * 12), V(F * 12), R(F * 9), wh(F * 2), boxes(D * 4), gt(D * 7), gt2d(D * 4);
        std::vector<int32_t> bframe(D);
        const double whole[4] = {-50, -50, 1300, 400}, part[4] = {300.25, 100.5, 900.75, 300};
        const double wide[7] = {0.0, 2.2, 20.0, 24.0, 16.0, 3.0, 0.4}, air[7] = {0.0, -6.0, 20.0, 3.9, 1.6, 1.5, -2.6};
        for (int f = 0; f < F; ++f) {
            for (int i = 0; i < 12; ++i) { P[f * 12 + i] = Pm[i]; V[f * 12 + i] = Vm[i]; }
            for (int i = 0; i < 9; ++i) R[f * 9 + i] = Rm[i];
            wh[2 * f] = 1242; wh[2 * f + 1] = 375;
        }
        for (int d = 0; d < D; ++d) {
            bframe[d] = d % 2;
            for (int k = 0; k < 4; ++k) { boxes[d * 4 + k] = d < 4 ? whole[k] : part[k]; gt2d[d * 4 + k] = part[k]; }
            for (int k = 0; k < 7; ++k) gt[d * 7 + k] = (d == 2 || d == 4) ? air[k] : wide[k];      // boxes 2, 4: no positive
        }
        bframe[5] = F;                                                        // out of range: skipped, not reported, never dereferenced
        std::vector<double> box2d(D * 4), angle(D), corners(D * 24);
        std::vector<int32_t> scnt((size_t)D * S, -1), spos((size_t)D * S, -1);
#define TCOUNT(p0, S_) fcn_frustum_train_count(p0, foff.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bframe.data(), D, S_, 0, 2.0, gt.data(), box2d.data(), angle.data(), scnt.data(), spos.data(), corners.data(), nullptr)
#define TFILL(so_, o_, os_) fcn_frustum_train_fill(pts.data(), foff.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bframe.data(), D, S, 0, 2.0, gt.data(), so_, o_, os_, nullptr)
        EXPECT(TCOUNT(pts.data(), S) == 0);
        // the same counts as the entry that reads the lists back (which reports the frame out of range)
        std::vector<int32_t> scnt2((size_t)D * S, -1), spos2((size_t)D * S, -1);
        EXPECT(fcn_frustum_label_count(pts.data(), foff.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bframe.data(), D, S, 0, 2.0, gt.data(), box2d.data(), angle.data(), scnt2.data(), spos2.data(), corners.data(), nullptr) == FCN_E_BADARG);
        EXPECT(scnt2 == scnt && spos2 == spos);
        EXPECT(scnt[5 * S] == 0 && scnt[5 * S + 2] == 0 && spos[2 * S] == 0 && spos[0] > 0 && spos[1 * S + 2] > 0);
        int64_t full[3] = {0, 0, 0};                                          // rows of boxes 0, 1, 3 (the survivors)
        for (int s = 0; s < S; ++s) { full[0] += scnt[s]; full[1] += scnt[S + s]; full[2] += scnt[3 * S + s]; }
        EXPECT(full[0] > 100 && full[1] > 100 && full[2] > 100);
        const int64_t all3 = full[0] + full[1] + full[2];
        // B slots, capacity: every regime; the fill writes into exactly capacity + 1 rows and never touches the spare one
        const struct { int B; int64_t cap; int status; } cases[] = {{2, full[0] + full[1], 0}, {3, all3, 0}, {3, all3 - 1, 4},
            {3, full[0] + 10, 4}, {5, all3 + 7, 2}, {4, 1, 6}, {1, full[0], 0}};
        for (const auto &c : cases) {
            std::vector<int32_t> slot_box(c.B, -1);
            std::vector<int64_t> soff((size_t)D * S + 1, -1), off(c.B + 1, -1);
            int32_t n_kept = -1, status = 0;
            EXPECT(fcn_frustum_train_plan(scnt.data(), spos.data(), gt2d.data(), 25.0, D, S, c.B, c.cap, slot_box.data(), soff.data(), off.data(), &n_kept, &status, nullptr) == 0);
            EXPECT(status == c.status && n_kept == (c.B < 3 ? c.B : 3) && slot_box[0] == 0 && soff[(size_t)D * S] <= c.cap && off[c.B] == soff[(size_t)D * S]);
            for (int i = n_kept; i < c.B; ++i) EXPECT(slot_box[i] == 0 && off[i] == off[c.B]);
            std::vector<float> out((size_t)(c.cap + 1) * ps, -7.f);
            std::vector<int64_t> oseg((size_t)c.cap + 1, -7);
            EXPECT(TFILL(soff.data(), out.data(), oseg.data()) == 0);
            const int64_t end = soff[(size_t)D * S];
            for (int64_t i = 0; i < end; ++i) EXPECT((oseg[i] == 0 || oseg[i] == 1) && out[i * ps + 2] > 0.f);
            for (int64_t i = end; i <= c.cap; ++i) EXPECT(oseg[i] == -7 && out[i * ps] == -7.f);
        }
        // more segments than a frame needs count 0; fewer than it needs is the caller's duty (no refusal, S segments searched)
        std::vector<int32_t> keep(scnt);
        scnt.assign((size_t)D * (S + 1), -1); spos.assign((size_t)D * (S + 1), -1);
        EXPECT(TCOUNT(pts.data(), S + 1) == 0 && scnt[S] == 0 && scnt[0] == keep[0] && scnt[(S + 1) + S] == 0);
        scnt.assign((size_t)D * (S - 1), -1); spos.assign((size_t)D * (S - 1), -1);
        EXPECT(TCOUNT(pts.data(), S - 1) == 0 && scnt[(S - 1)] == keep[S] && scnt[(S - 1) + 1] == keep[S + 1]);
        scnt.assign((size_t)D * S, -1); spos.assign((size_t)D * S, -1);
        // argument handling as the label entries have it
        EXPECT(TCOUNT(nullptr, S) == FCN_E_BADARG && TCOUNT(pts.data(), 0) == FCN_E_BADARG && scnt[0] == -1);
        std::vector<int64_t> soff((size_t)D * S + 1, 0);
        std::vector<float> out(ps, -7.f);
        std::vector<int64_t> oseg(1, -7);
        EXPECT(TFILL(nullptr, out.data(), oseg.data()) == FCN_E_BADARG && TFILL(soff.data(), nullptr, oseg.data()) == FCN_E_BADARG);
        EXPECT(TFILL(soff.data(), out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(TFILL(soff.data(), out.data(), oseg.data()) == 0 && out[0] == -7.f && oseg[0] == -7);      // every slice empty
#undef TCOUNT
#undef TFILL
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
