// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the SUN-RGBD frustum
// extraction's entry points -- fcn_frustum_sunrgbd_count / _fill / _label_count / _label_fill and fcn_frustum_subset_pos,
// csrc/frustum_sunrgbd.h compiled for the host against tests/host_harness/hip_emu -- with exactly sized buffers: the ragged frame
// lengths the kernels' paths turn on, strides 3, 4, 6 and 7, segment offsets that grant too few rows (and none at all to a box),
// out-of-range frames, a stride-4 buffer that is not 16-byte aligned, subsample indices out of range, argument handling.  Built
// with -fsanitize=address,undefined by tests/test_frustum_sunrgbd_sanitizer.py, so a read or write past any buffer is a report,
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
int main()
{
    const int seg = fcn_frustum_select_seg();
    EXPECT(seg > 0 && seg % 256 == 0);
    const double Km[9] = {529.5, 0, 365.0, 0, 529.5, 265.0, 0, 0, 1};
    const double Rm[9] = {0.99989, -0.0118, -0.0081, 0.0131, 0.98195, 0.1887, 0.0057, -0.1888, 0.98200};
    const int strides[4] = {3, 4, 6, 7};
    for (int si = 0; si < 4; ++si) {
        const int ps = strides[si];
        const int F = 10, D = 2 * F, S = 3;
        const int64_t len[F] = {0, 1, 63, 64, 65, 255, seg - 1, seg, seg + 1, 2 * (int64_t)seg + 100};
        std::vector<int64_t> off(F + 1, 0);
        for (int f = 0; f < F; ++f) off[f + 1] = off[f] + len[f];
        const int64_t n = off[F];
        std::vector<float> pts((size_t)n * ps);             // exactly sized: any read past the end is an ASan report
        srand(7);
        for (int64_t i = 0; i < n; ++i) {                   // upright depth: x right +-2.2 m, y forward 1.5..6 m (some behind), z up +-1.2 m
            pts[i * ps] = -2.2f + 4.4f * rand() / RAND_MAX; pts[i * ps + 1] = 1.5f + 4.5f * rand() / RAND_MAX; pts[i * ps + 2] = -1.2f + 2.4f * rand() / RAND_MAX;
            if (i % 17 == 5) pts[i * ps + 1] = -pts[i * ps + 1];
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = 0.5f;
        }
        pts[(off[9] + 10) * ps] = NAN;
        pts[(off[9] + seg + 1) * ps + 1] = INFINITY;
        std::vector<double> K(F * 9), R(F * 9), boxes(D * 4), gt(D * 7);
        std::vector<int32_t> bframe(D);
        for (int f = 0; f < F; ++f) {
            for (int i = 0; i < 9; ++i) { K[f * 9 + i] = Km[i]; R[f * 9 + i] = Rm[i]; }
            const double whole[4] = {-200, -200, 900, 700}, part[4] = {150.25, 100.5, 450.75, 400};
            // upright depth, half extents: a wide box that holds a good part of the frame, and one hanging in the air (no point)
            const double wide[7] = {0.0, 3.5, 0.0, 1.5, 1.2, 0.8, 0.4}, air[7] = {0.0, 3.0, 5.0, 0.5, 0.5, 0.3, -2.6};
            for (int k = 0; k < 4; ++k) { boxes[(2 * f) * 4 + k] = whole[k]; boxes[(2 * f + 1) * 4 + k] = part[k]; }
            for (int k = 0; k < 7; ++k) { gt[(2 * f) * 7 + k] = wide[k]; gt[(2 * f + 1) * 7 + k] = f % 2 ? air[k] : wide[k]; }
            bframe[2 * f] = f; bframe[2 * f + 1] = f;
        }
        std::vector<double> angle(D), corners(D * 24);
        std::vector<int32_t> scnt((size_t)D * S, -1), spos((size_t)D * S, -1), ucnt((size_t)D * S, -1);
#define LCOUNT(p0, ps_, bf_, D_, S_, gt_, cnt_, pos_, cor_) fcn_frustum_sunrgbd_label_count(p0, off.data(), F, ps_, K.data(), R.data(), boxes.data(), bf_, D_, S_, gt_, angle.data(), cnt_, pos_, cor_, nullptr)
#define LFILL(p0, bf_, S_, gt_, so_, o_, os_) fcn_frustum_sunrgbd_label_fill(p0, off.data(), F, ps, K.data(), R.data(), boxes.data(), bf_, D, S_, gt_, so_, o_, os_, nullptr)
#define UCOUNT(p0, bf_, S_, cnt_) fcn_frustum_sunrgbd_count(p0, off.data(), F, ps, K.data(), R.data(), boxes.data(), bf_, D, S_, angle.data(), cnt_, nullptr)
#define UFILL(p0, bf_, S_, so_, o_) fcn_frustum_sunrgbd_fill(p0, off.data(), F, ps, K.data(), R.data(), boxes.data(), bf_, D, S_, so_, o_, nullptr)
        int rc = LCOUNT(pts.data(), ps, bframe.data(), D, S, gt.data(), scnt.data(), spos.data(), corners.data());
        EXPECT(rc == 0);
        EXPECT(UCOUNT(pts.data(), bframe.data(), S, ucnt.data()) == 0 && ucnt == scnt);
        EXPECT(scnt[0] == 0 && spos[0] == 0 && spos[2] == 0);                        // the empty frame
        EXPECT(scnt[(2 * 7) * S] > 256 && scnt[(2 * 7) * S + 1] == 0 && spos[(2 * 7) * S + 1] == 0);
        EXPECT(spos[(2 * 9) * S] > 64 && spos[(2 * 9) * S + 1] > 64 && spos[(2 * 9) * S + 2] > 0);
        EXPECT(spos[(2 * 9 + 1) * S] == 0 && spos[(2 * 9 + 1) * S + 1] == 0 && scnt[(2 * 9 + 1) * S] > 64);   // the box in the air
        for (int i = 0; i < D * S; ++i) EXPECT(spos[i] >= 0 && spos[i] <= scnt[i]);
        EXPECT(std::isfinite(angle[1]) && corners[1] == -(0.8 + 0.0) && corners[4 * 3 + 1] == 0.8);          // upright camera y = -z
        std::vector<int64_t> soff((size_t)D * S + 1, 0);
        for (int i = 0; i < D * S; ++i) soff[i + 1] = soff[i] + scnt[i];
        std::vector<float> out((size_t)soff[D * S] * ps), outu((size_t)soff[D * S] * ps);   // exactly sized, all
        std::vector<int64_t> oseg((size_t)soff[D * S], -1);
        rc = LFILL(pts.data(), bframe.data(), S, gt.data(), soff.data(), out.data(), oseg.data());
        EXPECT(rc == 0);
        EXPECT(UFILL(pts.data(), bframe.data(), S, soff.data(), outu.data()) == 0 && memcmp(out.data(), outu.data(), out.size() * sizeof(float)) == 0);
        int64_t ones = 0, want = 0;
        for (int64_t i = 0; i < soff[D * S]; ++i) { EXPECT(oseg[i] == 0 || oseg[i] == 1); ones += oseg[i] == 1; EXPECT(std::isfinite(out[i * ps + 2])); }
        for (int i = 0; i < D * S; ++i) want += spos[i];
        EXPECT(ones == want && want > 0);
        // the positives under subsamples: units = boxes, one with every second row, one with indices out of range, the rest without
        {
            std::vector<int64_t> uoff(D), sub_off(D + 1, 0);
            std::vector<int32_t> ucount(D), sub, pos(D, -1);
            for (int d = 0; d < D; ++d) {
                uoff[d] = soff[(size_t)d * S];
                ucount[d] = (int32_t)(soff[(size_t)(d + 1) * S] - soff[(size_t)d * S]);
                if (d == 2 * 9) for (int k = 0; k < ucount[d]; k += 2) sub.push_back(k);
                if (d == 2 * 8) { sub.push_back(-1); sub.push_back(ucount[d]); sub.push_back(1 << 30); sub.push_back(0); }
                sub_off[d + 1] = (int64_t)sub.size();
            }
            EXPECT(fcn_frustum_subset_pos(oseg.data(), uoff.data(), ucount.data(), sub.data(), sub_off.data(), D, pos.data(), nullptr) == 0);
            for (int d = 0; d < D; ++d) {
                int64_t w = 0;
                if (d == 2 * 9) { for (int k = 0; k < ucount[d]; k += 2) w += oseg[uoff[d] + k]; }
                else if (d == 2 * 8) w = oseg[uoff[d]];
                else for (int k = 0; k < ucount[d]; ++k) w += oseg[uoff[d] + k];
                EXPECT(pos[d] == w);
            }
            EXPECT(fcn_frustum_subset_pos(oseg.data(), uoff.data(), ucount.data(), sub.data(), sub_off.data(), 0, nullptr, nullptr) == 0);
            EXPECT(fcn_frustum_subset_pos(nullptr, uoff.data(), ucount.data(), sub.data(), sub_off.data(), D, pos.data(), nullptr) == FCN_E_BADARG);
            EXPECT(fcn_frustum_subset_pos(oseg.data(), uoff.data(), ucount.data(), sub.data(), sub_off.data(), D, nullptr, nullptr) == FCN_E_BADARG);
            EXPECT(fcn_frustum_subset_pos(oseg.data(), uoff.data(), ucount.data(), sub.data(), sub_off.data(), -1, pos.data(), nullptr) == FCN_E_BADARG);
        }
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
        EXPECT(UFILL(pts.data(), bframe.data(), S, small.data(), out2.data()) == 0);
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
        EXPECT(UCOUNT(pts.data(), bad.data(), S, ucnt.data()) == FCN_E_BADARG && ucnt == scnt);
        for (int i = 0; i < D * S; ++i) soff[i + 1] = soff[i] + scnt[i];
        std::vector<float> out3((size_t)soff[D * S] * ps);
        std::vector<int64_t> oseg3((size_t)soff[D * S], -1);
        rc = LFILL(pts.data(), bad.data(), S, gt.data(), soff.data(), out3.data(), oseg3.data());
        EXPECT(rc == FCN_E_BADARG);
        for (int64_t i = 0; i < soff[D * S]; ++i) EXPECT(oseg3[i] == 0 || oseg3[i] == 1);
        EXPECT(UFILL(pts.data(), bad.data(), S, soff.data(), out3.data()) == FCN_E_BADARG);
        // a frame longer than S segments: refused, nothing launched (the counts keep their values)
        scnt[0] = -5; spos[0] = -6;
        rc = LCOUNT(pts.data(), ps, bframe.data(), D, S - 1, gt.data(), scnt.data(), spos.data(), corners.data());
        EXPECT(rc == FCN_E_BADARG && scnt[0] == -5 && spos[0] == -6);
        EXPECT(UCOUNT(pts.data(), bframe.data(), S - 1, scnt.data()) == FCN_E_BADARG && scnt[0] == -5);
        EXPECT(LFILL(pts.data(), bframe.data(), S - 1, gt.data(), soff.data(), out3.data(), oseg3.data()) == FCN_E_BADARG);
        EXPECT(UFILL(pts.data(), bframe.data(), S - 1, soff.data(), out3.data()) == FCN_E_BADARG);
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
        EXPECT(fcn_frustum_sunrgbd_label_count(pts.data(), off.data(), 0, ps, K.data(), R.data(), boxes.data(), bframe.data(), D, S, gt.data(), angle.data(), scnt.data(), spos.data(), corners.data(), nullptr) == 0);
        EXPECT(scnt[0] == 0 && scnt[D * S - 1] == 0 && spos[0] == 0 && spos[D * S - 1] == 0);
        scnt[0] = -5;
        EXPECT(fcn_frustum_sunrgbd_count(pts.data(), off.data(), 0, ps, K.data(), R.data(), boxes.data(), bframe.data(), D, S, angle.data(), scnt.data(), nullptr) == 0 && scnt[0] == 0);
        EXPECT(LFILL(pts.data(), bframe.data(), S, nullptr, soff.data(), out3.data(), oseg3.data()) == FCN_E_BADARG);
        EXPECT(LFILL(pts.data(), bframe.data(), S, gt.data(), nullptr, out3.data(), oseg3.data()) == FCN_E_BADARG);
        EXPECT(LFILL(pts.data(), bframe.data(), S, gt.data(), soff.data(), nullptr, oseg3.data()) == FCN_E_BADARG);
        EXPECT(LFILL(pts.data(), bframe.data(), S, gt.data(), soff.data(), out3.data(), nullptr) == FCN_E_BADARG);
        EXPECT(UFILL(pts.data(), bframe.data(), S, nullptr, out3.data()) == FCN_E_BADARG);
        EXPECT(UFILL(pts.data(), bframe.data(), S, soff.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_frustum_sunrgbd_label_fill(nullptr, nullptr, F, ps, nullptr, nullptr, nullptr, nullptr, 0, S, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
        EXPECT(fcn_frustum_sunrgbd_fill(nullptr, nullptr, F, ps, nullptr, nullptr, nullptr, nullptr, 0, S, nullptr, nullptr, nullptr) == 0);
#undef LCOUNT
#undef LFILL
#undef UCOUNT
#undef UFILL
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
