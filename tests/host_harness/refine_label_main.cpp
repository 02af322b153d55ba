// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the refinement
// stage's training link -- fcn_refine_match, fcn_refine_label_count / _fill, csrc/refine_label.h compiled for the host against
// tests/host_harness/hip_emu -- with exactly sized buffers: ragged frame lengths around the segment and wave boundaries, chained
// jitter copies, unmatched candidates, segment offsets that grant too few rows (and none at all to a unit), out-of-range rows,
// frames and labels, a stride-4 buffer that is not 16-byte aligned, argument handling.  Built with -fsanitize=address,undefined by
// tests/test_refine_label_sanitizer.py, so a read or write past any buffer is a report, not luck.
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
int main()
{
    const int seg = fcn_frustum_select_seg();
    EXPECT(seg > 0 && seg % 256 == 0);
    for (int ps = 3; ps <= 5; ++ps) {
        const int F = 9, S = 3, A = 3, R = 6, G = 5;
        const int64_t len[F] = {0, 1, 63, 65, 255, seg - 1, seg, seg + 1, 2 * (int64_t)seg + 100};
        std::vector<int64_t> off(F + 1, 0);
        for (int f = 0; f < F; ++f) off[f + 1] = off[f] + len[f];
        const int64_t n = off[F];
        std::vector<float> pts((size_t)n * ps);             // exactly sized: any read past the end is an ASan report
        srand(11);
        for (int64_t i = 0; i < n; ++i) {                   // rect camera coordinates around the boxes below
            pts[i * ps] = (float)(-4.0 + 8.0 * unit()); pts[i * ps + 1] = (float)(0.0 + 2.0 * unit()); pts[i * ps + 2] = (float)(16.0 + 8.0 * unit());
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = 0.5f;
        }
        pts[(off[8] + 10) * ps] = NAN;
        pts[(off[8] + seg + 1) * ps + 1] = INFINITY;
        // label boxes (tx, ty, tz, l, w, h, ry; t the bottom centre): frames 0..7 share none, frame 8 has rows 1..4, row 0 belongs
        // to frame 4; label_off is exactly F + 1 long
        const double gtv[G][7] = {{0, 1.8, 20, 6, 4, 1.6, 0.3}, {0, 1.8, 20, 6, 4, 1.6, 0.3}, {0, 1.8, 20, 6, 4, 1.6, 0.3},
                                  {1.5, 1.7, 19, 4, 3, 1.5, -2.9}, {30, 1.8, 60, 4, 2, 1.5, 1.0}};
        std::vector<double> gt(G * 7);
        for (int j = 0; j < G; ++j) for (int k = 0; k < 7; ++k) gt[j * 7 + k] = gtv[j][k];
        std::vector<int64_t> goff(F + 1, 0);
        for (int f = 0; f <= F; ++f) goff[f] = f <= 4 ? 0 : (f <= 8 ? 1 : 5);
        const float detv[R][8] = {{0.1f, 1.8f, 20.1f, 6.2f, 3.9f, 1.6f, 0.32f, 0.9f}, {1.4f, 1.7f, 19.1f, 4.1f, 3.0f, 1.5f, 3.1f, 0.8f},
                                  {9.f, 1.8f, 30.f, 4.f, 2.f, 1.5f, 0.f, 0.7f}, {0.f, 1.8f, 20.f, 6.f, 4.f, 1.6f, 0.3f, 0.6f},
                                  {30.f, 1.8f, 60.f, 4.f, 2.f, 1.5f, 1.f, 0.5f}, {0.2f, 1.9f, 20.2f, 5.8f, 4.1f, 1.7f, -3.1f, 0.4f}};
        std::vector<float> dets(R * 8);
        for (int r = 0; r < R; ++r) for (int k = 0; k < 8; ++k) dets[r * 8 + k] = detv[r][k];
        // candidates: one per frame 0..7 on row 0 (frame 4 has a label), then frame 8: rows 0 (tie of labels 1 and 2), 1, 2 (matches
        // nothing), 4 (far away: no point), 5, 3
        const int D = 14;
        const int32_t crow_[D] = {0, 0, 0, 0, 3, 0, 0, 0, 0, 1, 2, 4, 5, 3};
        const int32_t cframe_[D] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8, 8, 8, 8};
        std::vector<int32_t> crow(crow_, crow_ + D), cframe(cframe_, cframe_ + D), gidx(D, -9);
        std::vector<float> best(D, -9.f);
        int rc = fcn_refine_match(dets.data(), R, crow.data(), cframe.data(), D, gt.data(), G, goff.data(), F, 0.5, gidx.data(), best.data(), nullptr);
        EXPECT(rc == 0);
        for (int d = 0; d < 4; ++d) EXPECT(gidx[d] == -1 && best[d] == 0.f);
        EXPECT(gidx[4] == 0 && best[4] > 0.99f && gidx[5] == -1 && gidx[8] == 1 && best[8] > 0.5f && gidx[9] == 3 && gidx[10] == -1);
        EXPECT(gidx[11] == 4 && gidx[12] == 1 && gidx[13] == 1 && best[13] > 0.99f);
        const int U = D * A;
        std::vector<double> jit((size_t)U * 7);
        for (size_t i = 0; i < jit.size(); ++i) jit[i] = unit();
        std::vector<int32_t> scnt((size_t)U * S, -1), spos((size_t)U * S, -1);
        std::vector<double> pc(U * 24), pa(U), psz(U * 3), gc(U * 24), gh(U), gs(U * 3);
#define RCOUNT(p0, ps_, cr_, cf_, cg_, D_, A_, j_, S_, cnt_, pos_) fcn_refine_label_count(p0, off.data(), F, ps_, dets.data(), R, cr_, cf_, D_, 1.2, cg_, gt.data(), G, A_, j_, 0.05, S_, cnt_, pos_, pc.data(), pa.data(), psz.data(), gc.data(), gh.data(), gs.data(), nullptr)
#define RFILL(p0, cr_, cf_, cg_, A_, j_, S_, so_, o_) fcn_refine_label_fill(p0, off.data(), F, ps, dets.data(), R, cr_, cf_, D, 1.2, cg_, gt.data(), G, A_, j_, 0.05, S_, so_, o_, nullptr)
        rc = RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, A, jit.data(), S, scnt.data(), spos.data());
        EXPECT(rc == 0);
        for (int i = 0; i < U * S; ++i) EXPECT(spos[i] >= 0 && spos[i] <= scnt[i]);
        for (int u = 0; u < 4 * A; ++u) for (int s = 0; s < S; ++s) EXPECT(scnt[u * S + s] == 0);     // unmatched: empty units
        EXPECT(scnt[(4 * A) * S] > 10 && spos[(4 * A) * S] > 5 && scnt[(4 * A) * S + 1] == 0);        // frame 4: 255 rows, one segment
        for (int a = 0; a < A; ++a) for (int s = 0; s < S; ++s) EXPECT(scnt[(8 * A + a) * S + s] > 0 && spos[(13 * A + a) * S + s] > 0);
        for (int a = 0; a < A; ++a) for (int s = 0; s < S; ++s) EXPECT(scnt[(11 * A + a) * S + s] == 0 && scnt[(10 * A + a) * S + s] == 0);
        EXPECT(psz[(8 * A) * 3] != psz[(8 * A + 1) * 3] && fabs(pa[9 * A]) <= M_PI + 1e-9 && gs[(9 * A) * 3] == 4.0 && gh[9 * A] == -2.9);
        std::vector<int64_t> soff((size_t)U * S + 1, 0);
        for (int i = 0; i < U * S; ++i) soff[i + 1] = soff[i] + scnt[i];
        std::vector<float> out((size_t)soff[U * S] * ps);   // exactly sized
        rc = RFILL(pts.data(), crow.data(), cframe.data(), gidx.data(), A, jit.data(), S, soff.data(), out.data());
        EXPECT(rc == 0 && soff[U * S] > 1000);
        for (int64_t i = 0; i < soff[U * S]; ++i) EXPECT(out[i * ps + 2] >= 15.f && out[i * ps + 2] <= 25.f && std::isfinite(out[i * ps]));
        // offsets that grant too few rows to the middle segment of candidate 8's second copy and none to candidate 13: the surplus is dropped
        std::vector<int64_t> small((size_t)U * S + 1, 0);
        for (int i = 0; i < U * S; ++i) {
            int64_t c = scnt[i];
            if (i == (8 * A + 1) * S + 1) c -= 20;
            if (i / S / A == 13) c = 0;
            small[i + 1] = small[i] + (c < 0 ? 0 : c);
        }
        std::vector<float> out2((size_t)small[U * S] * ps);
        rc = RFILL(pts.data(), crow.data(), cframe.data(), gidx.data(), A, jit.data(), S, small.data(), out2.data());
        EXPECT(rc == 0);
        EXPECT(memcmp(out2.data(), out.data(), (size_t)small[(8 * A + 1) * S + 1] * ps * sizeof(float)) == 0);      // rows before the short slice
        // one copy, no jitter: NULL jitter is valid with A == 1 only
        {
            std::vector<int32_t> c1((size_t)D * S, -1), p1((size_t)D * S, -1);
            rc = RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, 1, nullptr, S, c1.data(), p1.data());
            EXPECT(rc == 0 && c1[8 * S] > 0 && psz[8 * 3] == (double)detv[0][3] * 1.2);
            std::vector<int64_t> so1((size_t)D * S + 1, 0);
            for (int i = 0; i < D * S; ++i) so1[i + 1] = so1[i] + c1[i];
            std::vector<float> o1((size_t)so1[D * S] * ps);
            EXPECT(RFILL(pts.data(), crow.data(), cframe.data(), gidx.data(), 1, nullptr, S, so1.data(), o1.data()) == 0);
            EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, 2, nullptr, S, c1.data(), p1.data()) == FCN_E_BADARG);
            EXPECT(RFILL(pts.data(), crow.data(), cframe.data(), gidx.data(), 2, nullptr, S, so1.data(), o1.data()) == FCN_E_BADARG);
        }
        // pt_stride 4 in a buffer that is not 16-byte aligned (input and output): the word-by-word path, the same answer
        if (ps == 4) {
            std::vector<float> shifted((size_t)n * ps + 1), outs((size_t)soff[U * S] * ps + 1);
            memcpy(shifted.data() + 1, pts.data(), (size_t)n * ps * sizeof(float));
            std::vector<int32_t> scnt2((size_t)U * S, -1), spos2((size_t)U * S, -1);
            rc = RCOUNT(shifted.data() + 1, ps, crow.data(), cframe.data(), gidx.data(), D, A, jit.data(), S, scnt2.data(), spos2.data());
            EXPECT(rc == 0 && scnt2 == scnt && spos2 == spos);
            rc = RFILL(shifted.data() + 1, crow.data(), cframe.data(), gidx.data(), A, jit.data(), S, soff.data(), outs.data() + 1);
            EXPECT(rc == 0 && memcmp(outs.data() + 1, out.data(), out.size() * sizeof(float)) == 0);
        }
        // out-of-range rows, frames and labels: exact-size dets / off / gt, so a dereference would be caught
        {
            std::vector<int32_t> br(crow), bf(cframe), bg(gidx), gi2(D, -9);
            br[8] = R; br[9] = -1; bf[12] = F; bf[13] = -(1 << 30);
            rc = fcn_refine_match(dets.data(), R, br.data(), bf.data(), D, gt.data(), G, goff.data(), F, 0.5, gi2.data(), best.data(), nullptr);
            EXPECT(rc == FCN_E_BADARG && gi2[8] == -1 && gi2[9] == -1 && gi2[12] == -1 && gi2[13] == -1 && gi2[4] == 0 && gi2[11] == 4);
            bg[4] = G; bg[11] = 1 << 30;
            pc[8 * A * 24] = -5.0; gc[4 * A * 24] = -6.0;
            std::vector<int32_t> c3((size_t)U * S, -1), p3((size_t)U * S, -1);
            rc = RCOUNT(pts.data(), ps, br.data(), bf.data(), bg.data(), D, A, jit.data(), S, c3.data(), p3.data());
            EXPECT(rc == FCN_E_BADARG && pc[8 * A * 24] == -5.0 && gc[4 * A * 24] == -6.0);
            for (int d : {4, 8, 9, 11, 12, 13}) for (int i = d * A * S; i < (d + 1) * A * S; ++i) EXPECT(c3[i] == 0 && p3[i] == 0);
            for (int i = 0; i < U * S; ++i) EXPECT(c3[i] >= 0);
            std::vector<int64_t> so3((size_t)U * S + 1, 0);
            for (int i = 0; i < U * S; ++i) so3[i + 1] = so3[i] + c3[i];
            std::vector<float> o3((size_t)so3[U * S] * ps);
            EXPECT(RFILL(pts.data(), br.data(), bf.data(), bg.data(), A, jit.data(), S, so3.data(), o3.data()) == FCN_E_BADARG);
            // only cand_gt out of range
            EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), bg.data(), D, A, jit.data(), S, c3.data(), p3.data()) == FCN_E_BADARG);
        }
        // a frame longer than S segments: refused, nothing launched (the counts keep their values)
        scnt[0] = -5; spos[0] = -6;
        rc = RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, A, jit.data(), S - 1, scnt.data(), spos.data());
        EXPECT(rc == FCN_E_BADARG && scnt[0] == -5 && spos[0] == -6);
        EXPECT(RFILL(pts.data(), crow.data(), cframe.data(), gidx.data(), A, jit.data(), S - 1, soff.data(), out.data()) == FCN_E_BADARG);
        // argument handling
        EXPECT(RCOUNT(pts.data(), 2, crow.data(), cframe.data(), gidx.data(), D, A, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(nullptr, ps, crow.data(), cframe.data(), gidx.data(), D, A, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, nullptr, cframe.data(), gidx.data(), D, A, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), nullptr, gidx.data(), D, A, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), nullptr, D, A, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, A, jit.data(), S, nullptr, spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, A, jit.data(), S, scnt.data(), nullptr) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, 0, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, 65, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), D, A, jit.data(), 0, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), -1, A, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(pts.data(), ps, crow.data(), cframe.data(), gidx.data(), 21846, A, jit.data(), S, scnt.data(), spos.data()) == FCN_E_BADARG);
        EXPECT(RCOUNT(nullptr, ps, nullptr, nullptr, nullptr, 0, A, nullptr, S, nullptr, nullptr) == 0);
        EXPECT(scnt[0] == -5 && spos[0] == -6);
        EXPECT(fcn_refine_label_count(pts.data(), off.data(), 0, ps, dets.data(), R, crow.data(), cframe.data(), D, 1.2, gidx.data(), gt.data(), G, A, jit.data(), 0.05, S, scnt.data(), spos.data(), pc.data(), pa.data(), psz.data(), gc.data(), gh.data(), gs.data(), nullptr) == 0);
        EXPECT(scnt[0] == 0 && scnt[U * S - 1] == 0 && spos[0] == 0 && spos[U * S - 1] == 0);
        EXPECT(RFILL(pts.data(), crow.data(), cframe.data(), gidx.data(), A, jit.data(), S, nullptr, out.data()) == FCN_E_BADARG);
        EXPECT(RFILL(pts.data(), crow.data(), cframe.data(), gidx.data(), A, jit.data(), S, soff.data(), nullptr) == FCN_E_BADARG);
        EXPECT(RFILL(pts.data(), crow.data(), cframe.data(), nullptr, A, jit.data(), S, soff.data(), out.data()) == FCN_E_BADARG);
        EXPECT(fcn_refine_label_fill(nullptr, nullptr, F, ps, nullptr, R, nullptr, nullptr, 0, 1.2, nullptr, nullptr, G, A, nullptr, 0.05, S, nullptr, nullptr, nullptr) == 0);
        EXPECT(fcn_refine_match(nullptr, R, crow.data(), cframe.data(), D, gt.data(), G, goff.data(), F, 0.5, gidx.data(), best.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_match(dets.data(), R, crow.data(), cframe.data(), D, gt.data(), G, nullptr, F, 0.5, gidx.data(), best.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_match(dets.data(), R, crow.data(), cframe.data(), D, gt.data(), G, goff.data(), F, 0.5, nullptr, best.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_refine_match(nullptr, R, nullptr, nullptr, 0, nullptr, G, nullptr, F, 0.5, nullptr, nullptr, nullptr) == 0);
        EXPECT(fcn_refine_match(dets.data(), R, crow.data(), cframe.data(), D, gt.data(), G, goff.data(), 0, 0.5, gidx.data(), best.data(), nullptr) == 0);
        EXPECT(gidx[4] == -1 && best[4] == 0.f && gidx[D - 1] == -1);
#undef RCOUNT
#undef RFILL
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
