// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the frustum
// extraction's entry points -- fcn_frustum_select_seg / _count / _fill, csrc/frustum_select.h compiled for the host against
// tests/host_harness/hip_emu -- with exactly sized buffers: the ragged frame lengths the kernels' paths turn on, an out-of-range
// frame, segment offsets that grant too few rows, argument handling.  Built with -fsanitize=address,undefined by
// tests/test_frustum_sanitizer.py, so a read or write past any buffer is a report, not luck.
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
    const int seg = fcn_frustum_select_seg();
    EXPECT(seg > 0 && seg % 256 == 0);
    const double Pm[12] = {721.5377, 0, 609.5593, 44.85728, 0, 721.5377, 172.854, 0.2163791, 0, 0, 1, 0.002745884};
    const double Vm[12] = {0.007533745, -0.9999714, -0.000616602, -0.004069766, 0.01480249, 0.0007280733, -0.9998902, -0.07631618,
                           0.9998621, 0.00752379, 0.01480755, -0.2717806};
    const double Rm[9] = {0.9999239, 0.00983776, -0.007445048, -0.009869795, 0.9999421, -0.004278459, 0.007402527, 0.004351614, 0.9999631};
    for (int ps = 3; ps <= 5; ++ps) {
        const int F = 10, D = 2 * F, S = 3;
        const int64_t len[F] = {0, 1, 63, 64, 65, 255, seg - 1, seg, seg + 1, 2 * (int64_t)seg + 100};
        std::vector<int64_t> off(F + 1, 0);
        for (int f = 0; f < F; ++f) off[f + 1] = off[f] + len[f];
        const int64_t n = off[F];
        std::vector<float> pts((size_t)n * ps);             // exactly sized: any read past the end is an ASan report
        srand(5);
        for (int64_t i = 0; i < n; ++i) {                   // velodyne: x forward 1..61 m, y left +-25 m, z up -2.5..1 m
            pts[i * ps] = 1.f + 60.f * rand() / RAND_MAX; pts[i * ps + 1] = -25.f + 50.f * rand() / RAND_MAX; pts[i * ps + 2] = -2.5f + 3.5f * rand() / RAND_MAX;
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = 0.5f;
        }
        pts[(off[9] + 10) * ps] = NAN;
        pts[(off[9] + seg + 1) * ps + 1] = INFINITY;
        std::vector<double> P(F * 12), V(F * 12), R(F * 9), wh(F * 2), boxes(D * 4);
        std::vector<int32_t> bframe(D);
        for (int f = 0; f < F; ++f) {
            for (int i = 0; i < 12; ++i) { P[f * 12 + i] = Pm[i]; V[f * 12 + i] = Vm[i]; }
            for (int i = 0; i < 9; ++i) R[f * 9 + i] = Rm[i];
            wh[2 * f] = 1242; wh[2 * f + 1] = 375;
            const double whole[4] = {-50, -50, 1300, 400}, part[4] = {300.25, 100.5, 900.75, 300};
            for (int k = 0; k < 4; ++k) { boxes[(2 * f) * 4 + k] = whole[k]; boxes[(2 * f + 1) * 4 + k] = part[k]; }
            bframe[2 * f] = f; bframe[2 * f + 1] = f;
        }
        std::vector<double> box2d(D * 4), angle(D);
        std::vector<int32_t> scnt((size_t)D * S, -1);
        int rc = fcn_frustum_select_count(pts.data(), off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(),
                                          bframe.data(), D, S, 1, 2.0, box2d.data(), angle.data(), scnt.data(), nullptr);
        EXPECT(rc == 0);
        EXPECT(scnt[0] == 0 && scnt[1] == 0 && scnt[2] == 0);                        // the empty frame
        EXPECT(scnt[(2 * 7) * S] > 256 && scnt[(2 * 7) * S + 1] == 0);               // frame of exactly seg rows: one segment
        EXPECT(scnt[(2 * 8) * S + 1] >= 0 && scnt[(2 * 8) * S + 2] == 0);            // seg + 1 rows: one row in the second
        EXPECT(scnt[(2 * 9) * S] > 256 && scnt[(2 * 9) * S + 1] > 256 && scnt[(2 * 9) * S + 2] > 0);
        EXPECT(box2d[0] == 0 && box2d[2] == 1241 && box2d[3] == 374 && angle[1] < 0);
        std::vector<int64_t> soff((size_t)D * S + 1, 0);
        for (int i = 0; i < D * S; ++i) { EXPECT(scnt[i] >= 0); soff[i + 1] = soff[i] + scnt[i]; }
        std::vector<float> out((size_t)soff[D * S] * ps);   // exactly sized
        rc = fcn_frustum_select_fill(pts.data(), off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(),
                                     bframe.data(), D, S, 1, 2.0, soff.data(), out.data(), nullptr);
        EXPECT(rc == 0);
        for (int64_t i = 0; i < soff[D * S]; ++i) EXPECT(out[i * ps + 2] > 0.f && (ps == 3 || out[i * ps + 3] == 0.5f));   // rect z
        // offsets that grant too few rows to the middle segment of the longest frame's first box: the surplus must be dropped
        std::vector<int64_t> small(soff);
        for (int i = (2 * 9) * S + 2; i <= D * S; ++i) small[i] -= 50;
        std::vector<float> out2((size_t)small[D * S] * ps);
        rc = fcn_frustum_select_fill(pts.data(), off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(),
                                     bframe.data(), D, S, 1, 2.0, small.data(), out2.data(), nullptr);
        EXPECT(rc == 0);
        // out-of-range frames: exact-size calibration / off, so a dereference would be caught
        std::vector<int32_t> bad(bframe);
        bad[3] = F; bad[18] = -1; bad[19] = 1 << 30;
        rc = fcn_frustum_select_count(pts.data(), off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(),
                                      bad.data(), D, S, 1, 2.0, box2d.data(), angle.data(), scnt.data(), nullptr);
        EXPECT(rc == FCN_E_BADARG && scnt[3 * S] == 0 && scnt[18 * S] == 0 && scnt[18 * S + 1] == 0 && scnt[19 * S + 2] == 0);
        EXPECT(scnt[(2 * 7) * S] > 256);
        for (int i = 0; i < D * S; ++i) soff[i + 1] = soff[i] + scnt[i];
        std::vector<float> out3((size_t)soff[D * S] * ps);
        rc = fcn_frustum_select_fill(pts.data(), off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(),
                                     bad.data(), D, S, 1, 2.0, soff.data(), out3.data(), nullptr);
        EXPECT(rc == FCN_E_BADARG);
        // a frame longer than S segments: refused, nothing launched (scnt keeps its values)
        scnt[0] = -5;
        rc = fcn_frustum_select_count(pts.data(), off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(),
                                      bframe.data(), D, S - 1, 1, 2.0, box2d.data(), angle.data(), scnt.data(), nullptr);
        EXPECT(rc == FCN_E_BADARG && scnt[0] == -5);
        // argument handling
#define COUNT(p0, ps_, D_, S_, cnt_) fcn_frustum_select_count(p0, off.data(), F, ps_, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bframe.data(), D_, S_, 1, 2.0, box2d.data(), angle.data(), cnt_, nullptr)
        EXPECT(COUNT(pts.data(), 2, D, S, scnt.data()) == FCN_E_BADARG);
        EXPECT(COUNT(nullptr, ps, D, S, scnt.data()) == FCN_E_BADARG);
        EXPECT(COUNT(pts.data(), ps, D, S, nullptr) == FCN_E_BADARG);
        EXPECT(COUNT(pts.data(), ps, D, 0, scnt.data()) == FCN_E_BADARG);
        EXPECT(COUNT(pts.data(), ps, -1, S, scnt.data()) == FCN_E_BADARG);
        EXPECT(COUNT(nullptr, ps, 0, S, nullptr) == 0);
        EXPECT(fcn_frustum_select_count(pts.data(), off.data(), 0, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bframe.data(), D, S, 1, 2.0, box2d.data(), angle.data(), scnt.data(), nullptr) == 0);
        EXPECT(scnt[0] == 0 && scnt[D * S - 1] == 0);
        EXPECT(fcn_frustum_select_fill(pts.data(), off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bframe.data(), D, S, 1, 2.0, nullptr, out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_frustum_select_fill(pts.data(), off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bframe.data(), D, S, 1, 2.0, soff.data(), nullptr, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_frustum_select_fill(nullptr, nullptr, F, ps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, S, 1, 2.0, nullptr, nullptr, nullptr) == 0);
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
