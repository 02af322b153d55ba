// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the labelled
// frustum extraction's entry points -- fcn_frustum_label_count / _fill, csrc/frustum_label.h compiled for the host against
// tests/host_harness/hip_emu -- with exactly sized buffers: the ragged frame lengths the kernels' paths turn on, segment offsets
// that grant too few rows (and none at all to a box), an out-of-range frame, a stride-4 buffer that is not 16-byte aligned,
// argument handling.  Built with -fsanitize=address,undefined by tests/test_frustum_label_sanitizer.py, so a read or write past
// any buffer is a report, not luck.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <cstring>
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
        srand(7);
        for (int64_t i = 0; i < n; ++i) {                   // velodyne: x forward 3..43 m, y left +-12 m, z up -2.5..1 m
            pts[i * ps] = 3.f + 40.f * rand() / RAND_MAX; pts[i * ps + 1] = -12.f + 24.f * rand() / RAND_MAX; pts[i * ps + 2] = -2.5f + 3.5f * rand() / RAND_MAX;
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = 0.5f;
        }
        pts[(off[9] + 10) * ps] = NAN;
        pts[(off[9] + seg + 1) * ps + 1] = INFINITY;
        std::vector<double> P(F * 12), V(F * 12), R(F * 9), wh(F * 2), boxes(D * 4), gt(D * 7);
        std::vector<int32_t> bframe(D);
        for (int f = 0; f < F; ++f) {
            for (int i = 0; i < 12; ++i) { P[f * 12 + i] = Pm[i]; V[f * 12 + i] = Vm[i]; }
            for (int i = 0; i < 9; ++i) R[f * 9 + i] = Rm[i];
            wh[2 * f] = 1242; wh[2 * f + 1] = 375;
            const double whole[4] = {-50, -50, 1300, 400}, part[4] = {300.25, 100.5, 900.75, 300};
            // rect camera coordinates: a wide box that holds a good part of the sweep, and one hanging in the air (no point)
            const double wide[7] = {0.0, 2.2, 20.0, 24.0, 16.0, 3.0, 0.4}, air[7] = {0.0, -6.0, 20.0, 3.9, 1.6, 1.5, -2.6};
            for (int k = 0; k < 4; ++k) { boxes[(2 * f) * 4 + k] = whole[k]; boxes[(2 * f + 1) * 4 + k] = part[k]; }
            for (int k = 0; k < 7; ++k) { gt[(2 * f) * 7 + k] = wide[k]; gt[(2 * f + 1) * 7 + k] = f % 2 ? air[k] : wide[k]; }
            bframe[2 * f] = f; bframe[2 * f + 1] = f;
        }
        std::vector<double> box2d(D * 4), angle(D), corners(D * 24);
        std::vector<int32_t> scnt((size_t)D * S, -1), spos((size_t)D * S, -1);
#define LCOUNT(p0, ps_, bf_, D_, S_, gt_, cnt_, pos_, cor_) fcn_frustum_label_count(p0, off.data(), F, ps_, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bf_, D_, S_, 0, 2.0, gt_, box2d.data(), angle.data(), cnt_, pos_, cor_, nullptr)
#define LFILL(p0, bf_, S_, gt_, so_, o_, os_) fcn_frustum_label_fill(p0, off.data(), F, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bf_, D, S_, 0, 2.0, gt_, so_, o_, os_, nullptr)
        int rc = LCOUNT(pts.data(), ps, bframe.data(), D, S, gt.data(), scnt.data(), spos.data(), corners.data());
        EXPECT(rc == 0);
        EXPECT(scnt[0] == 0 && spos[0] == 0 && spos[2] == 0);                        // the empty frame
        EXPECT(scnt[(2 * 7) * S] > 256 && scnt[(2 * 7) * S + 1] == 0 && spos[(2 * 7) * S + 1] == 0);
        EXPECT(spos[(2 * 9) * S] > 64 && spos[(2 * 9) * S + 1] > 64 && spos[(2 * 9) * S + 2] > 0);
        EXPECT(spos[(2 * 9 + 1) * S] == 0 && spos[(2 * 9 + 1) * S + 1] == 0 && scnt[(2 * 9 + 1) * S] > 64);   // the box in the air
        for (int i = 0; i < D * S; ++i) EXPECT(spos[i] >= 0 && spos[i] <= scnt[i]);
        EXPECT(box2d[0] == -50 && box2d[2] == 1300 && angle[1] < 0);                  // no clipping
        EXPECT(corners[1] == 2.2 && corners[4 * 3 + 1] == 2.2 - 3.0 && fabs(corners[2] - 20.0) < 16.0);
        std::vector<int64_t> soff((size_t)D * S + 1, 0);
        for (int i = 0; i < D * S; ++i) soff[i + 1] = soff[i] + scnt[i];
        std::vector<float> out((size_t)soff[D * S] * ps);   // exactly sized, both
        std::vector<int64_t> oseg((size_t)soff[D * S], -1);
        rc = LFILL(pts.data(), bframe.data(), S, gt.data(), soff.data(), out.data(), oseg.data());
        EXPECT(rc == 0);
        int64_t ones = 0, want = 0;
        for (int64_t i = 0; i < soff[D * S]; ++i) { EXPECT(oseg[i] == 0 || oseg[i] == 1); ones += oseg[i] == 1; EXPECT(out[i * ps + 2] > 0.f); }
        for (int i = 0; i < D * S; ++i) want += spos[i];
        EXPECT(ones == want && want > 0);
        // offsets that grant too few rows to the middle segment of the longest frame's first box, and none to its second box:
        // the surplus must be dropped from both buffers
        std::vector<int64_t> small((size_t)D * S + 1, 0);
        for (int i = 0; i < D * S; ++i) {
            int64_t c = scnt[i];
            if (i == (2 * 9) * S + 1) c -= 50;
            if (i / S == 2 * 9 + 1) c = 0;
            small[i + 1] = small[i] + c;
        }
        std::vector<float> out2((size_t)small[D * S] * ps);
        std::vector<int64_t> oseg2((size_t)small[D * S], -1);
        rc = LFILL(pts.data(), bframe.data(), S, gt.data(), small.data(), out2.data(), oseg2.data());
        EXPECT(rc == 0);
        for (int64_t i = 0; i < small[D * S]; ++i) EXPECT(oseg2[i] == 0 || oseg2[i] == 1);
        EXPECT(memcmp(out2.data(), out.data(), (size_t)small[(2 * 9) * S + 1] * ps * sizeof(float)) == 0);   // rows before the short slice
        // pt_stride 4 in a buffer that is not 16-byte aligned (input and output): the word-by-word path, the same answer
        if (ps == 4) {
            std::vector<float> shifted((size_t)n * ps + 1), outs((size_t)soff[D * S] * ps + 1);
            memcpy(shifted.data() + 1, pts.data(), (size_t)n * ps * sizeof(float));
            std::vector<int32_t> scnt2((size_t)D * S, -1), spos2((size_t)D * S, -1);
            std::vector<int64_t> osegs((size_t)soff[D * S], -1);
            rc = LCOUNT(shifted.data() + 1, ps, bframe.data(), D, S, gt.data(), scnt2.data(), spos2.data(), corners.data());
            EXPECT(rc == 0 && scnt2 == scnt && spos2 == spos);
            rc = LFILL(shifted.data() + 1, bframe.data(), S, gt.data(), soff.data(), outs.data() + 1, osegs.data());
            EXPECT(rc == 0 && osegs == oseg && memcmp(outs.data() + 1, out.data(), out.size() * sizeof(float)) == 0);
        }
        // out-of-range frames: exact-size calibration / off, so a dereference would be caught
        std::vector<int32_t> bad(bframe);
        bad[3] = F; bad[18] = -1; bad[19] = 1 << 30;
        corners[3 * 24] = -5.0;
        rc = LCOUNT(pts.data(), ps, bad.data(), D, S, gt.data(), scnt.data(), spos.data(), corners.data());
        EXPECT(rc == FCN_E_BADARG && scnt[3 * S] == 0 && spos[3 * S] == 0 && spos[18 * S] == 0 && spos[18 * S + 1] == 0 && spos[19 * S + 2] == 0);
        EXPECT(scnt[(2 * 7) * S] > 256 && spos[(2 * 7) * S] > 0 && corners[3 * 24] == -5.0);
        for (int i = 0; i < D * S; ++i) soff[i + 1] = soff[i] + scnt[i];
        std::vector<float> out3((size_t)soff[D * S] * ps);
        std::vector<int64_t> oseg3((size_t)soff[D * S], -1);
        rc = LFILL(pts.data(), bad.data(), S, gt.data(), soff.data(), out3.data(), oseg3.data());
        EXPECT(rc == FCN_E_BADARG);
        for (int64_t i = 0; i < soff[D * S]; ++i) EXPECT(oseg3[i] == 0 || oseg3[i] == 1);
        // a frame longer than S segments: refused, nothing launched (the counts keep their values)
        scnt[0] = -5; spos[0] = -6;
        rc = LCOUNT(pts.data(), ps, bframe.data(), D, S - 1, gt.data(), scnt.data(), spos.data(), corners.data());
        EXPECT(rc == FCN_E_BADARG && scnt[0] == -5 && spos[0] == -6);
        EXPECT(LFILL(pts.data(), bframe.data(), S - 1, gt.data(), soff.data(), out3.data(), oseg3.data()) == FCN_E_BADARG);
        // argument handling
        EXPECT(LCOUNT(pts.data(), 2, bframe.data(), D, S, gt.data(), scnt.data(), spos.data(), corners.data()) == FCN_E_BADARG);
        EXPECT(LCOUNT(nullptr, ps, bframe.data(), D, S, gt.data(), scnt.data(), spos.data(), corners.data()) == FCN_E_BADARG);
        EXPECT(LCOUNT(pts.data(), ps, bframe.data(), D, S, nullptr, scnt.data(), spos.data(), corners.data()) == FCN_E_BADARG);
        EXPECT(LCOUNT(pts.data(), ps, bframe.data(), D, S, gt.data(), nullptr, spos.data(), corners.data()) == FCN_E_BADARG);
        EXPECT(LCOUNT(pts.data(), ps, bframe.data(), D, S, gt.data(), scnt.data(), nullptr, corners.data()) == FCN_E_BADARG);
        EXPECT(LCOUNT(pts.data(), ps, bframe.data(), D, S, gt.data(), scnt.data(), spos.data(), nullptr) == FCN_E_BADARG);
        EXPECT(LCOUNT(pts.data(), ps, bframe.data(), D, 0, gt.data(), scnt.data(), spos.data(), corners.data()) == FCN_E_BADARG);
        EXPECT(LCOUNT(pts.data(), ps, bframe.data(), -1, S, gt.data(), scnt.data(), spos.data(), corners.data()) == FCN_E_BADARG);
        EXPECT(LCOUNT(pts.data(), ps, bframe.data(), 65536, S, gt.data(), scnt.data(), spos.data(), corners.data()) == FCN_E_BADARG);
        EXPECT(LCOUNT(nullptr, ps, nullptr, 0, S, nullptr, nullptr, nullptr, nullptr) == 0);
        EXPECT(scnt[0] == -5 && spos[0] == -6);
        EXPECT(fcn_frustum_label_count(pts.data(), off.data(), 0, ps, P.data(), V.data(), R.data(), wh.data(), boxes.data(), bframe.data(), D, S, 0, 2.0, gt.data(), box2d.data(), angle.data(), scnt.data(), spos.data(), corners.data(), nullptr) == 0);
        EXPECT(scnt[0] == 0 && scnt[D * S - 1] == 0 && spos[0] == 0 && spos[D * S - 1] == 0);
        EXPECT(LFILL(pts.data(), bframe.data(), S, nullptr, soff.data(), out3.data(), oseg3.data()) == FCN_E_BADARG);
        EXPECT(LFILL(pts.data(), bframe.data(), S, gt.data(), nullptr, out3.data(), oseg3.data()) == FCN_E_BADARG);
        EXPECT(LFILL(pts.data(), bframe.data(), S, gt.data(), soff.data(), nullptr, oseg3.data()) == FCN_E_BADARG);
        EXPECT(LFILL(pts.data(), bframe.data(), S, gt.data(), soff.data(), out3.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_frustum_label_fill(nullptr, nullptr, F, ps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, S, 0, 2.0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
#undef LCOUNT
#undef LFILL
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
