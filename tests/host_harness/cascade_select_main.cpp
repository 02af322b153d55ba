// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the two cascade
// entry points -- fcn_refine_select_count / _fill, csrc/refine_select.h compiled for the host against tests/host_harness/hip_emu --
// with exactly sized buffers: argument handling, out-of-range candidates, offsets that grant too few rows.  Built with
// -fsanitize=address,undefined by tests/test_cascade_sanitizer.py, so a read or write past any buffer is a report, not luck.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <vector>
#include "include/fcn_hip.h"
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
int main()
{
    for (int ps = 3; ps <= 4; ++ps) {
        const int F = 3, R = 4, D = 5;
        const int64_t cnts[F] = {1000, 77, 0};
        std::vector<int64_t> off = {0, 1000, 1077, 1077};
        std::vector<float> pts((size_t)1077 * ps);          // exactly sized: any read past the end is an ASan report
        srand(5);
        for (size_t i = 0; i < 1077; ++i) {
            pts[i * ps] = -8.f + 16.f * rand() / RAND_MAX; pts[i * ps + 1] = 2.f * rand() / RAND_MAX; pts[i * ps + 2] = 5.f + 20.f * rand() / RAND_MAX;
            if (ps == 4) pts[i * ps + 3] = 0.5f;
        }
        pts[10 * ps] = NAN;
        std::vector<float> dets = {0, 1.75f, 12, 6, 5, 1.5f, 0.f, .9f,   0, 6, 15, 40, 40, 10, 2.5f, .8f,
                                   100, 2, 100, 2, 2, 2, -1.57f, .7f,   0, 2.5f, 15, 12, 14, 3, 2.5f, .6f};
        std::vector<int32_t> crow = {0, 1, 2, 3, 1}, cframe = {0, 1, 0, 0, 2};
        std::vector<double> corners(D * 24), angle(D), size(D * 3);
        std::vector<int32_t> cnt(D, -1);
        (void)cnts;
        int rc = fcn_refine_select_count(pts.data(), off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2,
                                         corners.data(), angle.data(), size.data(), cnt.data(), nullptr);
        EXPECT(rc == 0);
        EXPECT(cnt[1] == 77 && cnt[2] == 0 && cnt[4] == 0 && cnt[0] > 0 && cnt[3] > 256);
        std::vector<int64_t> ooff(D + 1, 0);
        for (int d = 0; d < D; ++d) ooff[d + 1] = ooff[d] + cnt[d];
        std::vector<float> out((size_t)ooff[D] * ps);       // exactly sized
        rc = fcn_refine_select_fill(pts.data(), off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2,
                                    ooff.data(), out.data(), nullptr);
        EXPECT(rc == 0);
        // offsets that grant too few rows: the surplus must be dropped, not written
        std::vector<int64_t> small(ooff);
        for (int d = 4; d <= D; ++d) small[d] -= 50;
        std::vector<float> out2((size_t)small[D] * ps);
        rc = fcn_refine_select_fill(pts.data(), off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2,
                                    small.data(), out2.data(), nullptr);
        EXPECT(rc == 0);
        // out-of-range candidates: exact-size dets / off, so a dereference would be caught
        std::vector<int32_t> brow = {0, 4, -1, 3, 1}, bframe = {3, 1, 0, -5, 2};
        rc = fcn_refine_select_count(pts.data(), off.data(), F, ps, dets.data(), R, brow.data(), bframe.data(), D, 1.2,
                                     corners.data(), angle.data(), size.data(), cnt.data(), nullptr);
        EXPECT(rc == FCN_E_BADARG && cnt[0] == 0 && cnt[1] == 0 && cnt[2] == 0 && cnt[3] == 0 && cnt[4] == 0);
        rc = fcn_refine_select_fill(pts.data(), off.data(), F, ps, dets.data(), R, brow.data(), bframe.data(), D, 1.2,
                                    ooff.data(), out.data(), nullptr);
        EXPECT(rc == FCN_E_BADARG);
        // argument handling
        EXPECT(fcn_refine_select_count(pts.data(), off.data(), F, 2, dets.data(), R, crow.data(), cframe.data(), D, 1.2, corners.data(), angle.data(), size.data(), cnt.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_select_count(nullptr, off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2, corners.data(), angle.data(), size.data(), cnt.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_select_count(pts.data(), off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2, corners.data(), angle.data(), size.data(), nullptr, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_select_count(nullptr, nullptr, F, ps, nullptr, R, nullptr, nullptr, 0, 1.2, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
        EXPECT(fcn_refine_select_count(pts.data(), off.data(), 0, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2, corners.data(), angle.data(), size.data(), cnt.data(), nullptr) == 0);
        EXPECT(fcn_refine_select_count(pts.data(), off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), -1, 1.2, corners.data(), angle.data(), size.data(), cnt.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_select_fill(pts.data(), off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2, nullptr, out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_select_fill(pts.data(), off.data(), F, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2, ooff.data(), nullptr, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_select_fill(nullptr, nullptr, F, ps, nullptr, R, nullptr, nullptr, 0, 1.2, nullptr, nullptr, nullptr) == 0);
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
