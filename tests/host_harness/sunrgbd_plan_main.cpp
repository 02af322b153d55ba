// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the capturable
// SUN-RGBD training input -- fcn_box2d_perturb_sunrgbd, fcn_frustum_sunrgbd_train_count / _plan / _fill / _slots,
// fcn_frustum_subsample_draw, fcn_frustum_subset_pos and fcn_draw_batch_sliced, csrc/frustum_sunrgbd_plan.h compiled for the host
// against tests/host_harness/hip_emu -- with exactly sized buffers: more boxes than one workgroup's lanes, boxes of cap - 1, cap,
// cap + 1 rows, the subsample through the whole-row sort and through the radix select (cap = 2048, boxes on either side of 4096
// rows), capacities that cut a box in the middle and drop whole boxes (the fill then writes into exactly capacity + 1 rows), more
// and fewer survivors than slots, B = D = 1, argument handling.  Every result is compared with a plain sequential restatement
// (std::sort of the composites for the subsample).  Built with -fsanitize=address,undefined by
// tests/test_sunrgbd_plan_sanitizer.py, so a read or write past any buffer is a report, not luck.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <vector>
#include "include/fcn_hip.h"
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *o)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// row b's N indices from n >= N rows (tag 0): the contract, the plain way
static std::vector<int32_t> choice_ref(uint64_t seed, uint64_t step, int b, int64_t n, int N)
{
    std::vector<uint64_t> comp((size_t)n);
    uint32_t w[4];
    for (int64_t j = 0; j < n; ++j) {
        if ((j & 3) == 0) philox((uint32_t)(j >> 2), (uint32_t)b, (uint32_t)step, (uint32_t)(step >> 32) << 2, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        comp[j] = ((uint64_t)w[j & 3] << 32) | (uint64_t)j;
    }
    std::sort(comp.begin(), comp.end());
    std::vector<int32_t> out((size_t)N);
    for (int i = 0; i < N; ++i) out[i] = (int32_t)(uint32_t)comp[i];
    return out;
}

struct Chain {
    std::vector<int64_t> soff, row0, sub_off, off, counts, sub_start;
    std::vector<int32_t> stored, sub, pos, slot_box, sub_len;
    int32_t n_kept, status;
};

// plan -> subsample -> subset_pos -> slots through the entries on exactly sized buffers, each against its sequential restatement.
// labels: per box its rows' labels; the packed seg buffer is what the fill would have stored (exactly the stored rows long)
static Chain chain(const std::vector<int32_t> &cnt, const std::vector<int32_t> &pos, const std::vector<std::vector<int64_t>> &labels,
                   int D, int S, int B, int cap, int min_pos, int64_t capacity, uint64_t seed, int64_t step)
{
    Chain c;
    c.soff.assign((size_t)D * S + 1, -1); c.row0.assign(D, -1); c.stored.assign(D, -1); c.sub_off.assign((size_t)D + 1, -1);
    c.status = 0;
    EXPECT(fcn_frustum_sunrgbd_train_plan(cnt.data(), pos.data(), min_pos, cap, D, S, capacity, c.soff.data(), c.row0.data(),
                                          c.stored.data(), c.sub_off.data(), &c.status, nullptr) == 0);
    // ---- the plan, sequentially
    std::vector<char> pre(D);
    std::vector<int64_t> packed;
    int64_t run = 0, sub_run = 0;
    for (int d = 0; d < D; ++d) {
        int64_t p = 0;
        for (int s = 0; s < S; ++s) p += pos[(size_t)d * S + s];
        pre[d] = p >= min_pos;
        const int64_t start = run < capacity ? run : capacity;
        EXPECT(c.row0[d] == start);
        for (int s = 0; s < S; ++s) {
            EXPECT(c.soff[(size_t)d * S + s] == (run < capacity ? run : capacity));
            if (pre[d] && cnt[(size_t)d * S + s] > 0) run += cnt[(size_t)d * S + s];
        }
        const int64_t end = run < capacity ? run : capacity;
        EXPECT(c.stored[d] == end - start && c.sub_off[d] == sub_run);
        if (end - start > cap) sub_run += cap;
        if (pre[d]) packed.insert(packed.end(), labels[d].begin(), labels[d].end());
    }
    const int64_t end = run < capacity ? run : capacity;
    EXPECT(c.soff[(size_t)D * S] == end && c.sub_off[D] == sub_run && c.status == (run > capacity ? 4 : 0));
    packed.resize((size_t)end);                                              // exactly the stored rows
    // ---- the subsample: exactly sub_off[D] entries
    c.sub.assign((size_t)sub_run > 0 ? (size_t)sub_run : 1, -7);
    int64_t state = step;
    int32_t dstatus = 0;
    EXPECT(fcn_frustum_subsample_draw(c.stored.data(), c.sub_off.data(), D, cap, seed, &state, 1, c.sub.data(), &dstatus, nullptr) == 0);
    EXPECT(state == step + 1 && dstatus == 0);
    for (int d = 0; d < D; ++d) {
        if (c.sub_off[d + 1] == c.sub_off[d]) continue;
        const std::vector<int32_t> want = choice_ref(seed, (uint64_t)step, d, c.stored[d], cap);
        EXPECT(memcmp(want.data(), &c.sub[(size_t)c.sub_off[d]], (size_t)cap * 4) == 0);
        for (int i = 0; i < cap; ++i) EXPECT(want[i] >= 0 && want[i] < c.stored[d]);
    }
    if (sub_run == 0) EXPECT(c.sub[0] == -7);
    // ---- the positives after the subsample
    c.pos.assign(D, -7);
    if (packed.empty()) packed.push_back(0);
    EXPECT(fcn_frustum_subset_pos(packed.data(), c.row0.data(), c.stored.data(), c.sub.data(), c.sub_off.data(), D, c.pos.data(), nullptr) == 0);
    for (int d = 0; d < D; ++d) {
        int want = 0;
        if (c.sub_off[d + 1] > c.sub_off[d]) {
            for (int64_t j = c.sub_off[d]; j < c.sub_off[d + 1]; ++j) want += packed[(size_t)(c.row0[d] + c.sub[(size_t)j])] != 0;
        } else {
            for (int k = 0; k < c.stored[d]; ++k) want += packed[(size_t)(c.row0[d] + k)] != 0;
        }
        EXPECT(c.pos[d] == want);
    }
    // ---- the slots
    c.slot_box.assign(B, -7); c.off.assign(B, -7); c.counts.assign(B, -7); c.sub_start.assign(B, -7); c.sub_len.assign(B, -7);
    c.n_kept = -7;
    const int32_t before = c.status;
    EXPECT(fcn_frustum_sunrgbd_train_slots(pos.data(), c.pos.data(), c.row0.data(), c.stored.data(), c.sub_off.data(), min_pos, D, S, B,
                                           capacity, c.slot_box.data(), &c.n_kept, c.off.data(), c.counts.data(), c.sub_start.data(),
                                           c.sub_len.data(), &c.status, nullptr) == 0);
    int n = 0, survivors = 0;
    for (int d = 0; d < D; ++d) {
        if (!(pre[d] && c.pos[d] >= min_pos)) continue;
        if (survivors++ >= B) continue;
        const int64_t len = c.sub_off[d + 1] - c.sub_off[d];
        EXPECT(c.slot_box[n] == d && c.off[n] == c.row0[d] && c.counts[n] == c.stored[d] && c.sub_len[n] == len &&
               c.sub_start[n] == (len > 0 ? c.sub_off[d] : 0));
        ++n;
    }
    EXPECT(c.n_kept == n && c.status == (before | (survivors < B ? 2 : 0)));
    for (int i = n; i < B; ++i) EXPECT(c.slot_box[i] == 0 && c.off[i] == capacity && c.counts[i] == 0 && c.sub_start[i] == 0 && c.sub_len[i] == 0);
    return c;
}

static void make(const std::vector<int> &rows, int S, int every, std::vector<int32_t> &cnt, std::vector<int32_t> &pos,
                 std::vector<std::vector<int64_t>> &labels)
{
    const int D = (int)rows.size();
    cnt.assign((size_t)D * S, 0); pos.assign((size_t)D * S, 0); labels.assign(D, {});
    for (int d = 0; d < D; ++d) {
        labels[d].resize(rows[d]);
        for (int k = 0; k < rows[d]; ++k) {
            labels[d][k] = (k + d) % every == 0;
            const int s = (int)((int64_t)k * S / rows[d]);
            cnt[(size_t)d * S + s] += 1;
            pos[(size_t)d * S + s] += (int32_t)labels[d][k];
        }
    }
}

int main()
{
    // ---- perturb: 300 boxes (two workgroups), exactly sized
    {
        const int D = 300;
        std::vector<double> boxes((size_t)D * 4), out((size_t)D * 4, -7.0), again((size_t)D * 4, -7.0);
        srand(5);
        for (int d = 0; d < D; ++d) {
            const double x0 = -60 + 600.0 * rand() / RAND_MAX, y0 = -60 + 400.0 * rand() / RAND_MAX;
            boxes[4 * d] = x0; boxes[4 * d + 1] = y0; boxes[4 * d + 2] = x0 + 5 + 180.0 * rand() / RAND_MAX; boxes[4 * d + 3] = y0 + 5 + 100.0 * rand() / RAND_MAX;
        }
        int64_t state = 3;
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), D, 0.1, 99, &state, 1, out.data(), nullptr) == 0 && state == 4);
        for (int d = 0; d < D; ++d) {
            const double w = boxes[4 * d + 2] - boxes[4 * d], w2 = out[4 * d + 2] - out[4 * d];
            EXPECT(w2 >= 0.9 * w - 1e-9 && w2 <= 1.1 * w + 1e-9 && memcmp(&out[4 * d], &boxes[4 * d], 32) != 0);
        }
        state = 3;
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), D, 0.1, 99, &state, 0, again.data(), nullptr) == 0 && state == 3 && again == out);
        state = (1ll << 32) + 5;
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), 1, 0.1, 99, &state, 1, again.data(), nullptr) == 0);
        EXPECT(state == (1ll << 32) + 6 && again[0] != out[0] && again[4] == out[4]);                    // D = 1: one row written
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), 0, 0.1, 99, &state, 1, again.data(), nullptr) == 0 && state == (1ll << 32) + 7);
        EXPECT(fcn_box2d_perturb_sunrgbd(nullptr, D, 0.1, 99, &state, 1, out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), D, 0.1, 99, nullptr, 1, out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), D, 0.1, 99, &state, 1, nullptr, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), -1, 0.1, 99, &state, 1, out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), D, 1.0, 99, &state, 1, out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(fcn_box2d_perturb_sunrgbd(boxes.data(), D, NAN, 99, &state, 1, out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(state == (1ll << 32) + 7);
    }
    // ---- the chain on hand-made counts
    {
        std::vector<int32_t> cnt, pos;
        std::vector<std::vector<int64_t>> labels;
        const int cap = 16;
        // cap - 1, cap, cap + 1 rows, many more; 3: under the bar of positives; 5: no row
        make({15, 16, 17, 4, 400, 0, 90, 33, 1000, 16}, 3, 3, cnt, pos, labels);
        int64_t total = 15 + 16 + 17 + 400 + 90 + 33 + 1000 + 16;
        Chain c = chain(cnt, pos, labels, 10, 3, 4, cap, 5, 1ll << 40, 7, 0);
        EXPECT(c.status == 0 && c.n_kept == 4 && c.sub_off[10] == 5 * cap && c.stored[3] == 0);
        c = chain(cnt, pos, labels, 10, 3, 10, cap, 5, total, 7, 1);
        EXPECT(c.status == 2 && c.n_kept == 8);
        c = chain(cnt, pos, labels, 10, 3, 10, cap, 5, total - 1, 7, (1ll << 32) + 5);
        EXPECT(c.status == 6 && c.stored[9] == 15);                            // one row short: the last box, no subsample needed
        c = chain(cnt, pos, labels, 10, 3, 3, cap, 5, 15 + 16 + 16, 7, 2);     // cuts the box of cap + 1 rows to cap: no subsample
        EXPECT(c.status == 4 && c.stored[2] == 16 && c.sub_off[10] == 0 && c.n_kept == 3);
        c = chain(cnt, pos, labels, 10, 3, 6, cap, 5, 15 + 16 + 17 + 100, 7, 3);   // in the middle of a large box; the rest dropped whole
        EXPECT(c.status == 6 && c.stored[4] == 100 && c.stored[6] == 0 && c.sub_off[10] == 2 * cap);
        c = chain(cnt, pos, labels, 10, 3, 2, cap, 5, 0, 7, 4);                // no room at all
        EXPECT(c.n_kept == 0 && c.status == 6);
        c = chain(cnt, pos, labels, 10, 3, 2, cap, 2000, 1ll << 40, 7, 5);     // nobody over the bar
        EXPECT(c.n_kept == 0 && c.status == 2 && c.soff[30] == 0);
        make({9}, 1, 2, cnt, pos, labels);                                     // B = D = S = 1
        c = chain(cnt, pos, labels, 1, 1, 1, 8, 1, 100, 7, 6);
        EXPECT(c.n_kept == 1 && c.sub_len[0] == 8 && c.status == 0);
        // more boxes than the workgroup has lanes, a count that is no multiple of it
        std::vector<int> rows(777);
        srand(3);
        for (int &r : rows) r = rand() % 60;
        make(rows, 2, 2, cnt, pos, labels);
        c = chain(cnt, pos, labels, 777, 2, 300, cap, 5, 1ll << 40, 7, 7);
        EXPECT(c.n_kept == 300 && c.status == 0);
        c = chain(cnt, pos, labels, 777, 2, 777, cap, 5, 9000, 7, 8);
        EXPECT(c.status == 6);
        // cap = 2048: the whole-row sort (n <= 4096) and the radix select (n > 4096), and a capacity that moves a box between them
        make({2049, 4096, 4097, 12365, 2048}, 3, 5, cnt, pos, labels);
        c = chain(cnt, pos, labels, 5, 3, 5, 2048, 5, 1ll << 40, 11, 9);
        EXPECT(c.n_kept == 5 && c.sub_off[5] == 4 * 2048 && c.status == 0);
        c = chain(cnt, pos, labels, 5, 3, 5, 2048, 5, 2049 + 4096 + 4097 + 5000, 11, 10);
        EXPECT(c.stored[3] == 5000 && c.stored[4] == 0 && c.status == 6);
    }
    // ---- argument handling: nothing written
    {
        std::vector<int32_t> cnt(6, 50), pos(6, 9), stored(2, -1), sub(128, -1), p2(2, 9), slot_box(2, -1), sub_len(2, -1);
        std::vector<int64_t> soff(7, -1), row0(2, -1), sub_off(3, -1), off(2, -1), counts(2, -1), sub_start(2, -1);
        int32_t status = 0, n_kept = -1;
        int64_t state = 0;
#define PLAN(c_, p_, cap_, D_, S_, cy_, so_, r_, st_, su_, s_) fcn_frustum_sunrgbd_train_plan(c_, p_, 5, cap_, D_, S_, cy_, so_, r_, st_, su_, s_, nullptr)
        EXPECT(PLAN(nullptr, pos.data(), 64, 2, 3, 100, soff.data(), row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), nullptr, 64, 2, 3, 100, soff.data(), row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2, 3, 100, nullptr, row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2, 3, 100, soff.data(), nullptr, stored.data(), sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2, 3, 100, soff.data(), row0.data(), nullptr, sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2, 3, 100, soff.data(), row0.data(), stored.data(), nullptr, &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2, 3, 100, soff.data(), row0.data(), stored.data(), sub_off.data(), nullptr) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 0, 2, 3, 100, soff.data(), row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, -1, 3, 100, soff.data(), row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2, 0, 100, soff.data(), row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2, 3, -1, soff.data(), row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_BADARG);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2049, 3, 100, soff.data(), row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_LIMIT);
        EXPECT(PLAN(cnt.data(), pos.data(), 64, 2, 32769, 100, soff.data(), row0.data(), stored.data(), sub_off.data(), &status) == FCN_E_LIMIT);
#undef PLAN
        EXPECT(soff[0] == -1 && row0[0] == -1 && stored[0] == -1 && sub_off[0] == -1 && status == 0);
        std::vector<int32_t> st2 = {100, 3};
        std::vector<int64_t> so2 = {0, 64, 64};
#define SUBS(c_, o_, D_, cap_, st_, su_, s_) fcn_frustum_subsample_draw(c_, o_, D_, cap_, 9, st_, 1, su_, s_, nullptr)
        EXPECT(SUBS(nullptr, so2.data(), 2, 64, &state, sub.data(), &status) == FCN_E_BADARG);
        EXPECT(SUBS(st2.data(), nullptr, 2, 64, &state, sub.data(), &status) == FCN_E_BADARG);
        EXPECT(SUBS(st2.data(), so2.data(), 2, 64, nullptr, sub.data(), &status) == FCN_E_BADARG);
        EXPECT(SUBS(st2.data(), so2.data(), 2, 64, &state, nullptr, &status) == FCN_E_BADARG);
        EXPECT(SUBS(st2.data(), so2.data(), 2, 64, &state, sub.data(), nullptr) == FCN_E_BADARG);
        EXPECT(SUBS(st2.data(), so2.data(), -1, 64, &state, sub.data(), &status) == FCN_E_BADARG);
        EXPECT(SUBS(st2.data(), so2.data(), 2, 0, &state, sub.data(), &status) == FCN_E_BADARG);
        EXPECT(SUBS(st2.data(), so2.data(), 2, 2049, &state, sub.data(), &status) == FCN_E_LIMIT);
        EXPECT(state == 0 && sub[0] == -1 && status == 0);
        EXPECT(SUBS(st2.data(), so2.data(), 0, 64, &state, sub.data(), &status) == 0 && state == 1 && sub[0] == -1);   // the pass-through
#undef SUBS
#define SLOTS(sp_, p_, r_, st_, so_, D_, S_, B_, cy_, sb_, nk_, of_, co_, ss_, sl_, s_) \
    fcn_frustum_sunrgbd_train_slots(sp_, p_, r_, st_, so_, 5, D_, S_, B_, cy_, sb_, nk_, of_, co_, ss_, sl_, s_, nullptr)
        row0 = {0, 100}; sub_off = {0, 64, 64};
        EXPECT(SLOTS(nullptr, p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), nullptr, row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), nullptr, st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), nullptr, sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), nullptr, 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, nullptr, &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), nullptr, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, nullptr, counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), nullptr, sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), nullptr, sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), nullptr, &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), nullptr) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), -1, 3, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 0, 2, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 0, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2, -1, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_BADARG);
        EXPECT(SLOTS(pos.data(), p2.data(), row0.data(), st2.data(), sub_off.data(), 2, 3, 2049, 200, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status) == FCN_E_LIMIT);
#undef SLOTS
        EXPECT(slot_box[0] == -1 && n_kept == -1 && off[0] == -1 && counts[0] == -1 && sub_start[0] == -1 && sub_len[0] == -1 && status == 0);
    }
    // ---- count -> plan -> fill -> subsample -> positives -> slots -> sliced draw on frames, into buffers of exactly capacity + 1 rows
    const int seg = fcn_frustum_select_seg();
    const double Km[9] = {529.5, 0, 365.0, 0, 529.5, 265.0, 0, 0, 1};
    const double Rm[9] = {0.979589, 0.012593, -0.200614, 0.012593, 0.992231, 0.123772, 0.200614, -0.123772, 0.971820};
    for (int ps = 4; ps <= 6; ps += 2) {
        const int F = 2, D = 6, S = 3, N = 64, cap = 256;
        const int64_t len[F] = {5000, 2 * (int64_t)seg + 808};
        std::vector<int64_t> foff(F + 1, 0);
        for (int f = 0; f < F; ++f) foff[f + 1] = foff[f] + len[f];
        const int64_t n = foff[F];
        std::vector<float> pts((size_t)n * ps);
        srand(7);
        for (int64_t i = 0; i < n; ++i) {
            pts[i * ps] = -2.f + 4.f * rand() / RAND_MAX; pts[i * ps + 1] = 1.5f + 4.f * rand() / RAND_MAX; pts[i * ps + 2] = -1.f + 2.f * rand() / RAND_MAX;
            for (int k = 3; k < ps; ++k) pts[i * ps + k] = 0.5f;
        }
        std::vector<double> K(F * 9), R(F * 9), boxes(D * 4), gt(D * 7);
        std::vector<int32_t> bframe(D);
        const double whole[4] = {-50, -50, 800, 600}, part[4] = {300.25, 200.5, 420.75, 330};
        const double wide[7] = {0.0, 3.5, 0.0, 1.5, 1.5, 0.8, 0.4}, air[7] = {0.0, 3.0, 5.0, 0.5, 0.5, 0.3, -2.6};
        for (int f = 0; f < F; ++f)
            for (int i = 0; i < 9; ++i) { K[f * 9 + i] = Km[i]; R[f * 9 + i] = Rm[i]; }
        for (int d = 0; d < D; ++d) {
            bframe[d] = d % 2;
            for (int k = 0; k < 4; ++k) boxes[d * 4 + k] = d < 4 ? whole[k] : part[k];
            for (int k = 0; k < 7; ++k) gt[d * 7 + k] = d == 2 ? air[k] : wide[k];          // box 2: no positive
        }
        bframe[5] = F;                                                        // out of range: skipped, not reported, never dereferenced
        std::vector<double> angle(D), corners(D * 24);
        std::vector<int32_t> scnt((size_t)D * S, -1), spos((size_t)D * S, -1);
#define TCOUNT(p0, S_) fcn_frustum_sunrgbd_train_count(p0, foff.data(), F, ps, K.data(), R.data(), boxes.data(), bframe.data(), D, S_, gt.data(), angle.data(), scnt.data(), spos.data(), corners.data(), nullptr)
#define TFILL(so_, o_, os_) fcn_frustum_sunrgbd_train_fill(pts.data(), foff.data(), F, ps, K.data(), R.data(), boxes.data(), bframe.data(), D, S, gt.data(), so_, o_, os_, nullptr)
        EXPECT(TCOUNT(pts.data(), S) == 0);
        std::vector<int32_t> scnt2((size_t)D * S, -1), spos2((size_t)D * S, -1);
        EXPECT(fcn_frustum_sunrgbd_label_count(pts.data(), foff.data(), F, ps, K.data(), R.data(), boxes.data(), bframe.data(), D, S, gt.data(), angle.data(), scnt2.data(), spos2.data(), corners.data(), nullptr) == FCN_E_BADARG);
        EXPECT(scnt2 == scnt && spos2 == spos);
        int64_t full[D];
        for (int d = 0; d < D; ++d) { full[d] = 0; for (int s = 0; s < S; ++s) full[d] += scnt[(size_t)d * S + s]; }
        EXPECT(full[0] > cap && full[1] > 4096 && full[3] > 4096 && full[4] > 5 && full[5] == 0 && spos[2 * S] == 0 && spos[0] > 5);
        const int64_t all = full[0] + full[1] + full[3] + full[4];            // the pre-kept boxes: 0, 1, 3, 4
        const struct { int B; int64_t capacity; int status; } cases[] = {{4, all, 0}, {3, all + 9, 0}, {4, all - 1, 4}, {5, full[0] + 10, 6},
            {6, full[0] + full[1] + 300, 6}, {2, 1, 6}, {1, full[0], 4}};
        for (const auto &c : cases) {
            std::vector<int64_t> soff((size_t)D * S + 1, -1), row0(D, -1), sub_off(D + 1, -1);
            std::vector<int32_t> stored(D, -1);
            int32_t status = 0, dstatus = 0;
            EXPECT(fcn_frustum_sunrgbd_train_plan(scnt.data(), spos.data(), 5, cap, D, S, c.capacity, soff.data(), row0.data(), stored.data(), sub_off.data(), &status, nullptr) == 0);
            std::vector<float> out((size_t)(c.capacity + 1) * ps, -7.f);
            std::vector<int64_t> oseg((size_t)c.capacity + 1, -7);
            EXPECT(TFILL(soff.data(), out.data(), oseg.data()) == 0);
            const int64_t end = soff[(size_t)D * S];
            EXPECT(end <= c.capacity);
            for (int64_t i = 0; i < end; ++i) EXPECT(oseg[i] == 0 || oseg[i] == 1);
            for (int64_t i = end; i <= c.capacity; ++i) EXPECT(oseg[i] == -7 && out[i * ps] == -7.f);
            oseg[(size_t)c.capacity] = 0;                                     // (the spare row the source keeps zeroed)
            std::vector<int32_t> sub((size_t)sub_off[D] > 0 ? (size_t)sub_off[D] : 1, -7), pos(D, -7);
            int64_t state = 12;
            EXPECT(fcn_frustum_subsample_draw(stored.data(), sub_off.data(), D, cap, 21, &state, 1, sub.data(), &dstatus, nullptr) == 0);
            for (int d = 0; d < D; ++d)
                for (int64_t j = sub_off[d]; j < sub_off[d + 1]; ++j) EXPECT(sub[(size_t)j] >= 0 && sub[(size_t)j] < stored[d]);
            EXPECT(fcn_frustum_subset_pos(oseg.data(), row0.data(), stored.data(), sub.data(), sub_off.data(), D, pos.data(), nullptr) == 0);
            std::vector<int32_t> slot_box(c.B, -7), sub_len(c.B, -7), choice((size_t)c.B * N, -7);
            std::vector<int64_t> off(c.B, -7), counts(c.B, -7), sub_start(c.B, -7);
            std::vector<double> coin(c.B), normal(c.B), hshift(c.B);
            int32_t n_kept = -7;
            EXPECT(fcn_frustum_sunrgbd_train_slots(spos.data(), pos.data(), row0.data(), stored.data(), sub_off.data(), 5, D, S, c.B, c.capacity, slot_box.data(), &n_kept, off.data(), counts.data(), sub_start.data(), sub_len.data(), &status, nullptr) == 0);
            EXPECT(status == c.status && n_kept >= 0 && n_kept <= c.B);
            fcn_draw_desc dd = {c.B, N, 1, 1};
            EXPECT(fcn_draw_batch_sliced(&dd, counts.data(), sub.data(), sub_start.data(), sub_len.data(), 20, &state, choice.data(), coin.data(), normal.data(), hshift.data(), &dstatus, nullptr) == 0);
            EXPECT(state == 14 && dstatus == (n_kept < c.B ? 1 : 0));
            for (int i = 0; i < c.B; ++i)
                for (int k = 0; k < N; ++k) {
                    const int32_t j = choice[(size_t)i * N + k];
                    EXPECT(i < n_kept ? (j >= 0 && j < counts[i] && off[i] + j < end) : (j == 0 && off[i] == c.capacity));
                }
        }
        EXPECT(TCOUNT(nullptr, S) == FCN_E_BADARG && TCOUNT(pts.data(), 0) == FCN_E_BADARG);
        std::vector<int64_t> soff((size_t)D * S + 1, 0);
        std::vector<float> out(ps, -7.f);
        std::vector<int64_t> oseg(1, -7);
        EXPECT(TFILL(nullptr, out.data(), oseg.data()) == FCN_E_BADARG && TFILL(soff.data(), nullptr, oseg.data()) == FCN_E_BADARG);
        EXPECT(TFILL(soff.data(), out.data(), nullptr) == FCN_E_BADARG);
        EXPECT(TFILL(soff.data(), out.data(), oseg.data()) == 0 && out[0] == -7.f && oseg[0] == -7);      // every slice empty
#undef TCOUNT
#undef TFILL
    }
    // ---- the sliced draw's own refusals
    {
        std::vector<int64_t> counts = {10, 20}, st = {0, 0};
        std::vector<int32_t> tab(4, 0), ln = {0, 0}, choice(16, -7);
        std::vector<double> coin(2, -7), normal(2, -7);
        int64_t state = 0;
        int32_t status = 0;
        fcn_draw_desc dd = {2, 8, 1, 1}, big = {2, 2049, 1, 1}, none = {0, 8, 1, 1};
        EXPECT(fcn_draw_batch_sliced(nullptr, counts.data(), tab.data(), st.data(), ln.data(), 9, &state, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_draw_batch_sliced(&dd, nullptr, tab.data(), st.data(), ln.data(), 9, &state, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_draw_batch_sliced(&dd, counts.data(), nullptr, st.data(), ln.data(), 9, &state, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_draw_batch_sliced(&dd, counts.data(), tab.data(), nullptr, ln.data(), 9, &state, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_draw_batch_sliced(&dd, counts.data(), tab.data(), st.data(), nullptr, 9, &state, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_draw_batch_sliced(&dd, counts.data(), tab.data(), st.data(), ln.data(), 9, nullptr, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_draw_batch_sliced(&dd, counts.data(), tab.data(), st.data(), ln.data(), 9, &state, nullptr, coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_draw_batch_sliced(&dd, counts.data(), tab.data(), st.data(), ln.data(), 9, &state, choice.data(), coin.data(), normal.data(), nullptr, nullptr, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_draw_batch_sliced(&big, counts.data(), tab.data(), st.data(), ln.data(), 9, &state, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_LIMIT);
        EXPECT(fcn_draw_batch_sliced(&none, counts.data(), tab.data(), st.data(), ln.data(), 9, &state, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(state == 0 && choice[0] == -7 && coin[0] == -7 && status == 0);
        EXPECT(fcn_draw_batch_sliced(&dd, counts.data(), tab.data(), st.data(), ln.data(), 9, &state, choice.data(), coin.data(), normal.data(), nullptr, &status, nullptr) == 0);
        EXPECT(state == 1 && choice[15] >= 0 && choice[15] < 20);
    }
    printf(fails ? "%d FAILED\n" : "all ok (%d)\n", fails);
    return fails != 0;
}
