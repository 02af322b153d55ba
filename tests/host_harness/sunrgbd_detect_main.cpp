// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives capturable SUN-RGBD
// inference -- fcn_frustum_sunrgbd_detect_count / _plan / _fill (csrc/frustum_sunrgbd_detect_plan.h) and fcn_det_rows
// (csrc/det_eval.h), compiled for the host against tests/host_harness/hip_emu -- with exactly sized buffers, on the cases that sit on
// a boundary: n_boxes at, beyond and below the table, box frames and classes out of range, more and fewer survivors than slots, counts
// at the bar and at the cap, the capacity met, one row short and 0, D = S = B = 1 and the largest plan; count -> plan -> fill ->
// fcn_frustum_subsample_draw -> fcn_draw_batch_sliced on frames of 4096, 4097 and 0 rows into a point buffer of exactly capacity + 1
// rows and a subsample table of exactly sub_off[B] entries; the tail on keep lists with counts of 0, top_k, beyond top_k and -1 and
// rows at and beyond num_dets; argument handling.  Built with -fsanitize=address,undefined by
// tests/test_sunrgbd_detect_source_sanitizer.py, so a read or write past any buffer is a report, not luck.
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

struct Plan {
    std::vector<int32_t> slot_box, cnt32, sub_len, slot_group;
    std::vector<int64_t> soff, off, counts, sub_off, sub_start;
    int32_t n = -1, status = 0;
    Plan(int D, int S, int B) : slot_box(B, -1), cnt32(B, -1), sub_len(B, -1), slot_group(B, -1), soff((size_t)D * S + 1, -1), off(B + 1, -1),
                                counts(B, -1), sub_off(B + 1, -1), sub_start(B, -1) {}
    bool operator==(const Plan &o) const
    {
        return slot_box == o.slot_box && cnt32 == o.cnt32 && sub_len == o.sub_len && slot_group == o.slot_group && soff == o.soff &&
               off == o.off && counts == o.counts && sub_off == o.sub_off && sub_start == o.sub_start && n == o.n && status == o.status;
    }
};

// the plan as the contract states it, sequentially
static Plan plan_ref(const std::vector<int32_t> &cnt, const std::vector<int32_t> &frame, const std::vector<int32_t> &cls, int nb, int thr,
                     int cap, int D, int S, int B, int64_t capacity, int F, int C)
{
    Plan p(D, S, B);
    p.slot_box.assign(B, D); p.off.assign(B + 1, capacity); p.counts.assign(B, 0); p.cnt32.assign(B, 0); p.sub_len.assign(B, 0);
    p.sub_start.assign(B, 0); p.slot_group.assign(B, F * C);
    p.n = 0; p.status = 0;
    if (nb < 0 || nb > D) { p.status |= 1024; nb = nb < 0 ? 0 : D; }
    int survivors = 0;
    int64_t run = 0;
    for (int d = 0; d < D; ++d) {
        bool keep = d < nb;
        if (keep && (frame[d] < 0 || frame[d] >= F || cls[d] < 0 || cls[d] >= C)) { p.status |= 1024; keep = false; }
        if (keep) {
            int64_t q = 0;
            for (int s = 0; s < S; ++s) q += cnt[(size_t)d * S + s] > 0 ? cnt[(size_t)d * S + s] : 0;
            keep = (q < cap ? q : cap) >= (thr > 1 ? thr : 1);
        }
        const bool slot = keep && survivors < B;
        if (keep) ++survivors;
        const int64_t lo = run < capacity ? run : capacity;
        for (int s = 0; s < S; ++s) {
            p.soff[(size_t)d * S + s] = run < capacity ? run : capacity;
            if (slot && cnt[(size_t)d * S + s] > 0) run += cnt[(size_t)d * S + s];
        }
        if (slot) {
            p.slot_box[p.n] = d; p.off[p.n] = lo; p.counts[p.n] = (run < capacity ? run : capacity) - lo;
            p.slot_group[p.n] = frame[d] * C + cls[d];
            ++p.n;
        }
    }
    p.soff[(size_t)D * S] = run < capacity ? run : capacity;
    p.off[B] = p.soff[(size_t)D * S];
    int64_t at = 0;
    for (int i = 0; i < B; ++i) {
        const bool sub = p.counts[i] > cap;
        p.cnt32[i] = (int32_t)p.counts[i];
        p.sub_off[i] = at; p.sub_start[i] = sub ? at : 0; p.sub_len[i] = sub ? cap : 0;
        if (sub) at += cap;
    }
    p.sub_off[B] = at;
    p.status |= (survivors > B ? 256 : 0) | (run > capacity ? 4 : 0);
    return p;
}

static int run_plan(const std::vector<int32_t> &cnt, const std::vector<int32_t> &frame, const std::vector<int32_t> &cls, int nb, int thr,
                    int cap, int D, int S, int B, int64_t capacity, int F, int C, Plan &p)
{
    const std::vector<int32_t> nbv(1, nb);
    return fcn_frustum_sunrgbd_detect_plan(cnt.data(), frame.data(), cls.data(), nbv.data(), thr, cap, D, S, B, capacity, F, C,
                                           p.slot_box.data(), &p.n, p.soff.data(), p.off.data(), p.counts.data(), p.cnt32.data(),
                                           p.sub_off.data(), p.sub_start.data(), p.sub_len.data(), p.slot_group.data(), &p.status, nullptr);
}

static int plan_case(const std::vector<int32_t> &cnt, const std::vector<int32_t> &frame, const std::vector<int32_t> &cls, int nb, int D,
                     int S, int B, int64_t capacity, int F, int C, int want_status, int thr = 2, int cap = 6)
{
    Plan p(D, S, B);
    EXPECT(run_plan(cnt, frame, cls, nb, thr, cap, D, S, B, capacity, F, C, p) == 0);
    EXPECT(p == plan_ref(cnt, frame, cls, nb, thr, cap, D, S, B, capacity, F, C));
    EXPECT(p.status == want_status);
    return p.n;
}

static void rows_case(const std::vector<int32_t> &keep, const std::vector<int32_t> &cnt, int G, int K, int nd, int want_status)
{
    std::vector<float> dets((size_t)nd * 8);
    for (size_t i = 0; i < dets.size(); ++i) dets[i] = (float)i;
    std::vector<int32_t> det_off(G + 1, -9), rows((size_t)G * K, -9);
    std::vector<float> scores((size_t)G * K, -9.f), corners((size_t)G * K * 24, -9.f);
    int32_t n_rows = -9, status = 0;
    EXPECT(fcn_det_rows(keep.data(), cnt.data(), G, K, nd ? dets.data() : nullptr, nd, det_off.data(), rows.data(), scores.data(), &n_rows,
                        &status, nullptr) == 0);
    EXPECT(fcn_box3d_corners(nd ? dets.data() : nullptr, nd, rows.data(), G * K, corners.data(), nullptr) == 0);
    int at = 0;
    for (int g = 0; g < G; ++g) {
        EXPECT(det_off[g] == at);
        const int c = cnt[g] < 0 ? 0 : (cnt[g] > K ? K : cnt[g]);
        for (int j = 0; j < c; ++j, ++at) {
            const int r = keep[(size_t)g * K + j];
            const bool in = r >= 0 && r < nd;
            EXPECT(rows[at] == r && (in ? scores[at] == dets[(size_t)r * 8 + 7] : std::isnan(scores[at])));
            EXPECT(in ? std::isfinite(corners[(size_t)at * 24]) : std::isnan(corners[(size_t)at * 24 + 23]));
        }
    }
    EXPECT(det_off[G] == at && n_rows == at && status == want_status);
    for (int e = at; e < G * K; ++e) EXPECT(rows[e] == -1 && std::isnan(scores[e]) && std::isnan(corners[(size_t)e * 24]));
}

int main()
{
    // ---- the plan on its boundaries: exactly sized counts, frames, classes and outputs (bar 2 rows, cap 6)
    {
        const int D = 6, S = 2, F = 2, C = 3;
        const std::vector<int32_t> cnt = {3, 0, 1, 0, 2, 5, 4, 4, 0, 0, 6, 0};             // 3, 1 (under the bar), 7, 8, 0, 6 (== cap)
        const std::vector<int32_t> frame = {0, 1, 1, 0, 1, 0}, cls = {2, 0, 1, 2, 1, 0};
        EXPECT(plan_case(cnt, frame, cls, D, D, S, 6, 100, F, C, 0) == 4);
        EXPECT(plan_case(cnt, frame, cls, D, D, S, 4, 100, F, C, 0) == 4);                 // exactly B survivors
        EXPECT(plan_case(cnt, frame, cls, D, D, S, 3, 100, F, C, 256) == 3);               // B + 1
        EXPECT(plan_case(cnt, frame, cls, 0, D, S, 3, 100, F, C, 0) == 0);                 // n_boxes = 0: every slot at the spare row
        EXPECT(plan_case(cnt, frame, cls, D + 1, D, S, 6, 100, F, C, 1024) == 4);          // beyond the table: row D is never read
        EXPECT(plan_case(cnt, frame, cls, INT32_MAX, D, S, 6, 100, F, C, 1024) == 4);
        EXPECT(plan_case(cnt, frame, cls, -1, D, S, 6, 100, F, C, 1024) == 0);
        EXPECT(plan_case(cnt, frame, cls, INT32_MIN, D, S, 6, 100, F, C, 1024) == 0);
        EXPECT(plan_case(cnt, frame, cls, 3, D, S, 6, 100, F, C, 0) == 2);
        for (int32_t v : {-1, 3, INT32_MIN, INT32_MAX}) {
            std::vector<int32_t> bad(frame), badc(cls);
            bad[2] = v; badc[2] = v;
            EXPECT(plan_case(cnt, bad, cls, D, D, S, 6, 100, F, C, 1024) == 3);
            EXPECT(plan_case(cnt, frame, badc, D, D, S, 6, 100, F, C, 1024) == 3);
            EXPECT(plan_case(cnt, bad, badc, 2, D, S, 6, 100, F, C, 0) == 1);              // beyond n_boxes it is nobody's business
        }
        EXPECT(plan_case(cnt, frame, cls, D, D, S, 6, 24, F, C, 0) == 4);                  // 3 + 7 + 8 + 6 = 24: exactly met
        EXPECT(plan_case(cnt, frame, cls, D, D, S, 6, 23, F, C, 4) == 4);                  // one row short
        EXPECT(plan_case(cnt, frame, cls, D, D, S, 6, 9, F, C, 4) == 4);                   // box 2 stores 6 rows: no subsample any more
        EXPECT(plan_case(cnt, frame, cls, D, D, S, 6, 10, F, C, 4) == 4);                  // exactly at box 2's end, 0 rows of box 3
        EXPECT(plan_case(cnt, frame, cls, D, D, S, 6, 0, F, C, 4) == 4);
        EXPECT(plan_case({5}, {0}, {0}, 1, 1, 1, 1, 100, 1, 1, 0, 5, 64) == 1);             // D = S = B = 1, count == point_threshold
        EXPECT(plan_case({4}, {0}, {0}, 1, 1, 1, 1, 100, 1, 1, 0, 5, 64) == 0);
        EXPECT(plan_case({64}, {0}, {0}, 1, 1, 1, 1, 100, 1, 1, 0, 5, 64) == 1);            // cap, cap + 1
        EXPECT(plan_case({65}, {0}, {0}, 1, 1, 1, 1, 100, 1, 1, 0, 5, 64) == 1);
        EXPECT(plan_case({0}, {0}, {0}, 1, 1, 1, 1, 100, 1, 1, 0, 0, 64) == 0);             // the bar is max(1, threshold)
        EXPECT(plan_case({1}, {0}, {0}, 1, 1, 1, 1, 100, 1, 1, 0, -3, 64) == 1);
    }
    {
        int max_d = 0, max_segs = 0;
        EXPECT(fcn_frustum_detect_plan_limits(&max_d, &max_segs) == 0 && max_d == 2048 && max_segs == 65536);
        const int D = max_d, S = max_segs / max_d;
        srand(5);
        std::vector<int32_t> cnt((size_t)D * S), frame(D), cls(D);
        for (int d = 0; d < D; ++d) {
            const bool rows = unit() < 0.6;
            for (int s = 0; s < S; ++s) cnt[(size_t)d * S + s] = rows ? (int)(unit() * 50) : 0;
            frame[d] = (int)(unit() * 11) - 1;                                              // -1 .. 9 of F = 9
            cls[d] = (int)(unit() * 12) - 1;                                                // -1 .. 10 of C = 10
        }
        plan_case(cnt, frame, cls, D, D, S, D, (int64_t)1 << 40, 9, 10, 1024, 5, 700);
        plan_case(cnt, frame, cls, D - 3, D, S, 300, 9000, 9, 10, 1024 | 256 | 4, 5, 700);
    }
    // ---- count -> plan -> fill -> the two draws on frames of 4096, 4097 and 0 rows: Rtilt = identity, a pinhole K
    {
        const int F = 3, ps = 6, S = 2, D = 7, B = 5, cap = 64, N = 32, C = 10;
        const std::vector<int64_t> foff = {0, 4096, 8193, 8193};
        std::vector<float> pts((size_t)8193 * ps);
        srand(9);
        for (size_t i = 0; i < pts.size() / ps; ++i) {                                     // upright depth: y is the camera's depth axis
            pts[i * ps] = (float)(-3.0 + 6.0 * unit()); pts[i * ps + 1] = (float)(1.5 + 4.0 * unit());
            pts[i * ps + 2] = (float)(-2.0 + 4.0 * unit());
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = (float)unit();
        }
        std::vector<double> K, Rt;
        for (int f = 0; f < F; ++f) {
            const double k[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1}, r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            K.insert(K.end(), k, k + 9); Rt.insert(Rt.end(), r, r + 9);
        }
        // a box wider than the image and an inner box per frame, and a seventh that the table's n_boxes = 6 leaves out
        std::vector<double> boxes;
        for (int d = 0; d < D; ++d) {
            const double whole[4] = {-2000, -2000, 3000, 3000}, inner[4] = {150.25, 100.5, 450.75, 400.0};
            boxes.insert(boxes.end(), d % 2 ? inner : whole, (d % 2 ? inner : whole) + 4);
        }
        const std::vector<int32_t> bframe = {0, 0, 1, 1, 2, 2, 0}, bclass = {1, 3, 7, 4, 9, 8, 2};
        // the reading selection over all seven boxes
        std::vector<double> wang(D, -9.0);
        std::vector<int32_t> wcnt((size_t)D * S, -9);
        EXPECT(fcn_frustum_sunrgbd_count(pts.data(), foff.data(), F, ps, K.data(), Rt.data(), boxes.data(), bframe.data(), D, S, wang.data(),
                                         wcnt.data(), nullptr) == 0);
        EXPECT(wcnt[0] == 4096 && wcnt[1] == 0 && wcnt[4] == 4096 && wcnt[5] == 1 && wcnt[8] == 0 && wcnt[12] == 4096 && wcnt[2] > cap && wcnt[2] < 2000);
        std::vector<int64_t> wsoff((size_t)D * S + 1, 0);
        for (int i = 0; i < D * S; ++i) wsoff[i + 1] = wsoff[i] + wcnt[i];
        std::vector<float> wrows((size_t)wsoff[(size_t)D * S] * ps, -9.f);
        EXPECT(fcn_frustum_sunrgbd_fill(pts.data(), foff.data(), F, ps, K.data(), Rt.data(), boxes.data(), bframe.data(), D, S, wsoff.data(),
                                        wrows.data(), nullptr) == 0);
        for (int32_t nb : {6, 7, 9, 0, -4}) {
            for (int bad = 0; bad < 3; ++bad) {                                            // box 2's frame: as it is, F, -1
                std::vector<int32_t> bf(bframe);
                if (bad) bf[2] = bad == 1 ? F : -1;
                const std::vector<int32_t> nbv(1, nb);
                std::vector<double> ang(D, -9.0);
                std::vector<int32_t> cnt((size_t)D * S, -9);
                EXPECT(fcn_frustum_sunrgbd_detect_count(pts.data(), foff.data(), F, ps, K.data(), Rt.data(), boxes.data(), bf.data(), D, S,
                                                        nbv.data(), ang.data(), cnt.data(), nullptr) == 0);
                for (int d = 0; d < D; ++d) {
                    const bool dead = d >= nb || (bad && d == 2);
                    for (int s = 0; s < S; ++s) EXPECT(cnt[(size_t)d * S + s] == (dead ? 0 : wcnt[(size_t)d * S + s]));
                    EXPECT(dead ? ang[d] == -9.0 : memcmp(&ang[d], &wang[d], 8) == 0);
                }
                int64_t total = 0;
                for (int d = 0; d < D; ++d) total += cnt[(size_t)d * S] + cnt[(size_t)d * S + 1];
                for (int64_t capacity : {total, total - 1, total / 2, (int64_t)0}) {
                    if (capacity < 0) continue;
                    Plan p(D, S, B);
                    EXPECT(run_plan(cnt, bf, bclass, nb, 5, cap, D, S, B, capacity, F, C, p) == 0);
                    EXPECT(p == plan_ref(cnt, bf, bclass, nb, 5, cap, D, S, B, capacity, F, C));
                    const int want_bits = ((nb > D || nb < 0) ? 1024 : 0) | ((bad && nb > 2) ? 1024 : 0) | (capacity < total ? 4 : 0);
                    EXPECT(p.status == want_bits && p.soff[(size_t)D * S] == capacity && p.off[B] == capacity);
                    // exactly capacity + 1 rows: the spare row behind the buffer is read by an empty slot, never written
                    std::vector<float> out((size_t)(capacity + 1) * ps, -9.f);
                    EXPECT(fcn_frustum_sunrgbd_detect_fill(pts.data(), foff.data(), F, ps, K.data(), Rt.data(), boxes.data(), bf.data(), D, S,
                                                           nbv.data(), p.soff.data(), out.data(), nullptr) == 0);
                    for (int k = 0; k < ps; ++k) EXPECT(out[(size_t)capacity * ps + k] == -9.f);
                    int64_t stored = 0;
                    for (int b = 0; b < B; ++b) {
                        stored += p.counts[b];
                        EXPECT(b < p.n ? (p.slot_box[b] < D && p.off[b] + p.counts[b] <= capacity)
                                       : (p.slot_box[b] == D && p.off[b] == capacity && p.counts[b] == 0 && p.slot_group[b] == F * C));
                        if (b < p.n && capacity == total && !bad) {                        // the live, in-range boxes: the reading fill's rows
                            const int d = p.slot_box[b];
                            EXPECT(memcmp(&out[(size_t)p.off[b] * ps], &wrows[(size_t)wsoff[(size_t)d * S] * ps], (size_t)p.counts[b] * ps * 4) == 0);
                        }
                    }
                    EXPECT(stored == capacity);
                    for (int64_t i = 0; i < capacity * ps; ++i)
                        if (out[i] == -9.f) { EXPECT(out[i] != -9.f); break; }             // every granted row is written
                    // the subsample table: exactly sub_off[B] entries; then the resample through (sub_start, sub_len)
                    std::vector<int32_t> sub((size_t)p.sub_off[B] + 1, -9), choice((size_t)B * N, -9);
                    int64_t state = 3;
                    int32_t dstatus = 0;
                    EXPECT(fcn_frustum_subsample_draw(p.cnt32.data(), p.sub_off.data(), B, cap, 77, &state, 1, sub.data(), &dstatus, nullptr) == 0);
                    EXPECT(state == 4 && sub[(size_t)p.sub_off[B]] == -9);
                    for (int b = 0; b < B; ++b)
                        for (int64_t j = p.sub_off[b]; j < p.sub_off[b + 1]; ++j) EXPECT(sub[j] >= 0 && sub[j] < p.counts[b]);
                    std::vector<double> coin(B, -9.0), normal(B, -9.0), hshift(B, -9.0);
                    const fcn_draw_desc dd = {B, N, 0, 0};
                    EXPECT(fcn_draw_batch_sliced(&dd, p.counts.data(), sub.data(), p.sub_start.data(), p.sub_len.data(), 78, &state,
                                                 choice.data(), coin.data(), normal.data(), hshift.data(), &dstatus, nullptr) == 0);
                    for (int b = 0; b < B; ++b)
                        for (int i = 0; i < N; ++i) {
                            const int32_t c = choice[(size_t)b * N + i];
                            EXPECT(p.counts[b] > 0 ? (c >= 0 && c < p.counts[b]) : c == 0);
                        }
                }
            }
        }
        // ---- argument handling
        {
            const std::vector<int32_t> nbv(1, D);
            std::vector<int32_t> cnt((size_t)D * S, -9);
            std::vector<int64_t> soff((size_t)D * S + 1, 0);
            EXPECT(fcn_frustum_sunrgbd_detect_count(pts.data(), foff.data(), F, ps, K.data(), Rt.data(), boxes.data(), bframe.data(), D, S, nullptr,
                                                    wang.data(), cnt.data(), nullptr) == 10001);
            EXPECT(fcn_frustum_sunrgbd_detect_fill(pts.data(), foff.data(), F, ps, K.data(), Rt.data(), boxes.data(), bframe.data(), D, S, nullptr,
                                                   soff.data(), pts.data(), nullptr) == 10001);
            EXPECT(fcn_frustum_sunrgbd_detect_count(pts.data(), foff.data(), F, 2, K.data(), Rt.data(), boxes.data(), bframe.data(), D, S,
                                                    nbv.data(), wang.data(), cnt.data(), nullptr) == 10001);
            Plan p(D, S, 4);
            const Plan fresh(D, S, 4);
            EXPECT(fcn_frustum_sunrgbd_detect_plan(cnt.data(), bframe.data(), bclass.data(), nullptr, 5, cap, D, S, 4, 100, F, C, p.slot_box.data(),
                                                   &p.n, p.soff.data(), p.off.data(), p.counts.data(), p.cnt32.data(), p.sub_off.data(),
                                                   p.sub_start.data(), p.sub_len.data(), p.slot_group.data(), &p.status, nullptr) == 10001);
            EXPECT(run_plan(cnt, bframe, bclass, D, 5, cap, 2049, S, 4, 100, F, C, p) == 10002);
            EXPECT(run_plan(cnt, bframe, bclass, D, 5, 0, D, S, 4, 100, F, C, p) == 10001);
            EXPECT(run_plan(cnt, bframe, bclass, D, 5, cap, D, S, 4, 100, F, 0, p) == 10001);
            EXPECT(run_plan(cnt, bframe, bclass, D, 5, cap, D, S, 4, 100, 1 << 30, C, p) == 10001);
            EXPECT(p == fresh && cnt[0] == -9);
        }
    }
    // ---- the tail: exactly sized keep lists, counts, detections and outputs
    {
        rows_case({3, 1, -1, 0, -1, -1, 2, 4, 5, 1, 1, 1}, {2, 0, 3, -1}, 4, 3, 5, 2048);   // a row equal to num_dets; a group over 4096
        rows_case({3, 1, -1, 0, -1, -1, 2, 4, 5, 1, 1, 1}, {9, 3, 1, 0}, 4, 3, 5, 0);       // a count beyond top_k; -1 inside a count
        rows_case({4, INT32_MAX, INT32_MIN}, {3}, 1, 3, 5, 0);                              // G = 1; the last row; far out of range
        rows_case({0, 0, 0, 0}, {1, 1, 1, 1}, 4, 1, 0, 0);                                  // top_k = 1; no detection at all
        srand(3);
        for (int G : {255, 256, 257}) {                                                     // a thread's run goes from one group to two
            std::vector<int32_t> keep((size_t)G * 4), cnt(G);
            for (auto &k : keep) k = (int)(unit() * 40) - 2;
            for (auto &c : cnt) c = (int)(unit() * 6);
            rows_case(keep, cnt, G, 4, 37, 0);
        }
        std::vector<int32_t> keep(12, 0), cnt(4, 0), det_off(5, -9), rows(12, -9);
        std::vector<float> scores(12, -9.f), dets(40, 0.f);
        int32_t n_rows = -9, status = -9;
        EXPECT(fcn_det_rows(nullptr, cnt.data(), 4, 3, dets.data(), 5, det_off.data(), rows.data(), scores.data(), &n_rows, &status, nullptr) == 10001);
        EXPECT(fcn_det_rows(keep.data(), cnt.data(), 4, 3, nullptr, 5, det_off.data(), rows.data(), scores.data(), &n_rows, &status, nullptr) == 10001);
        EXPECT(fcn_det_rows(keep.data(), cnt.data(), 0, 3, dets.data(), 5, det_off.data(), rows.data(), scores.data(), &n_rows, &status, nullptr) == 10001);
        EXPECT(fcn_det_rows(keep.data(), cnt.data(), 4, 4097, dets.data(), 5, det_off.data(), rows.data(), scores.data(), &n_rows, &status, nullptr) == 10002);
        EXPECT(fcn_det_rows(keep.data(), cnt.data(), 65537, 3, dets.data(), 5, det_off.data(), rows.data(), scores.data(), &n_rows, &status, nullptr) == 10002);
        EXPECT(det_off[0] == -9 && rows[0] == -9 && scores[0] == -9.f && n_rows == -9 && status == -9);
    }
    if (!fails) printf("all ok\n");
    return fails ? 1 : 0;
}
