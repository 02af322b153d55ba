// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the device draws --
// fcn_draw_batch / fcn_draw_limits, csrc/draws.h compiled for the host against tests/host_harness/hip_emu -- with exactly sized
// buffers over the row shapes the kernel's three paths turn on, and a SMALL instantiation of the same routine (DIGIT_BITS = 2,
// SORT_CAP = 64, n up to 5000) that drives the radix select's refine loop several digits deep, which the production sizes do not
// reach.  Every row is compared with a plain std::sort of the composites.  Built with -fsanitize=address,undefined by
// tests/test_draws_sanitizer.py, so a read or write past any buffer is a report, not luck.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <vector>
#define FCN_DRAWS_NO_ENTRY 1                       // the C entries live in inputs.hip's translation unit
#include "frustum_convnet_amd/csrc/draws.h"
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static const uint64_t SEED = 0x0123456789ABCDEFull;

// the contract, the plain way: every composite, std::sort, the first N
static std::vector<int32_t> ref_row(uint64_t step, int b, int64_t n, int N, const int32_t *sub)
{
    std::vector<int32_t> out((size_t)N, 0);
    if (n <= 0 || n >= 2147483648LL) return out;
    const uint32_t c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32) << 2, k0 = (uint32_t)SEED, k1 = (uint32_t)(SEED >> 32);
    uint32_t w[4];
    if (n < N) {
        for (int i = 0; i < N; ++i) {
            if ((i & 3) == 0) draw_philox((uint32_t)(i >> 2), (uint32_t)b, c2, c3 | 1u, k0, k1, w);
            const uint32_t r = (uint32_t)(((uint64_t)w[i & 3] * (uint64_t)n) >> 32);
            out[i] = sub ? sub[r] : (int32_t)r;
        }
        return out;
    }
    std::vector<uint64_t> comp((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        if ((j & 3) == 0) draw_philox((uint32_t)(j >> 2), (uint32_t)b, c2, c3, k0, k1, w);
        comp[j] = ((uint64_t)w[j & 3] << 32) | (uint64_t)j;
    }
    std::sort(comp.begin(), comp.end());
    for (int i = 0; i < N; ++i) { const uint32_t j = (uint32_t)comp[i]; out[i] = sub ? sub[j] : (int32_t)j; }
    return out;
}

struct Run {
    std::vector<int32_t> choice;
    std::vector<double> coin, normal, hshift;
    int64_t state;
    int32_t status;
    int rc;
};

// exactly sized buffers, all of them; small = the <2, 64> instantiation through the launcher, else the C entry
static Run run(const std::vector<int64_t> &counts, int N, uint64_t step, bool small, const std::vector<int32_t> *sub = nullptr,
               const std::vector<int64_t> *sub_off = nullptr, int flip = 1, int shift = 1)
{
    const int B = (int)counts.size();
    Run r;
    r.choice.assign((size_t)B * N, -7);
    r.coin.assign(B, -1.0); r.normal.assign(B, -1.0); r.hshift.assign(B, -1.0);
    r.state = (int64_t)step; r.status = 0;
    if (small) {
        DrawArgs a;
        a.B = B; a.N = N; a.flip = flip; a.shift = shift; a.counts = counts.data();
        a.sub = sub ? sub->data() : nullptr; a.sub_off = sub_off ? sub_off->data() : nullptr;
        a.seed = SEED; a.state = &r.state; a.choice = r.choice.data(); a.coin = r.coin.data(); a.normal = r.normal.data();
        a.hshift = r.hshift.data(); a.status = &r.status;
        r.rc = draw_batch_launch<2, 64>(a, nullptr);
    } else {
        fcn_draw_desc d = {B, N, flip, shift};
        r.rc = fcn_draw_batch(&d, counts.data(), sub ? sub->data() : nullptr, sub_off ? sub_off->data() : nullptr, SEED, &r.state,
                              r.choice.data(), r.coin.data(), r.normal.data(), r.hshift.data(), &r.status, nullptr);
    }
    return r;
}

static void compare(const Run &r, const std::vector<int64_t> &counts, int N, uint64_t step, const std::vector<int32_t> *sub = nullptr,
                    const std::vector<int64_t> *sub_off = nullptr)
{
    EXPECT(r.rc == 0 && r.state == (int64_t)step + 1);
    bool any_bad = false;
    for (size_t b = 0; b < counts.size(); ++b) {
        int64_t n = counts[b];
        const int32_t *s = nullptr;
        if (sub && (*sub_off)[b + 1] > (*sub_off)[b]) { n = (*sub_off)[b + 1] - (*sub_off)[b]; s = sub->data() + (*sub_off)[b]; }
        any_bad = any_bad || n <= 0 || n >= 2147483648LL;
        const std::vector<int32_t> want = ref_row(step, (int)b, n, N, s);
        if (memcmp(want.data(), r.choice.data() + b * (size_t)N, sizeof(int32_t) * (size_t)N) != 0) {
            printf("FAIL row %zu: n = %lld, N = %d, step %llu\n", b, (long long)n, N, (unsigned long long)step);
            ++fails;
        }
        EXPECT(r.coin[b] >= 0.0 && r.coin[b] < 1.0 && r.hshift[b] >= 0.0 && r.hshift[b] < 1.0 && std::fabs(r.normal[b]) <= 8.6);
    }
    EXPECT(r.status == (any_bad ? 1 : 0));
}

int main()
{
    int max_n = 0, cap = 0;
    EXPECT(fcn_draw_limits(&max_n, &cap) == 0 && max_n == DRAW_MAX_N && cap == DRAW_SORT_CAP);
    EXPECT(fcn_draw_limits(nullptr, &cap) == FCN_E_BADARG && fcn_draw_limits(&max_n, nullptr) == FCN_E_BADARG);
    // ---- the production instantiation: every path and its edges mixed into one launch of 37 rows, and alone
    const int Ns[5] = {1, 4, 8, 1024, 2048};
    for (int ni = 0; ni < 5; ++ni) {
        const int N = Ns[ni];
        const std::vector<int64_t> counts = {1, 5, N > 1 ? N - 1 : 1, N, N + 1, 3, 63, 65, 255, 257, 777, 1023, 1025, 2047, 2049, 2050, 3001,
                                             cap - 1, cap, cap + 1, cap + 3, 5000, 8191, 8193, 10007, 12345, 20011, 33333, 50021,
                                             70001, 100003, 4, 64, 256, 6, 2, 4099};
        EXPECT(counts.size() == 37);
        compare(run(counts, N, 11 + ni, false), counts, N, 11 + ni);
    }
    const int64_t singles[][2] = {{1, 1}, {1, 4}, {5, 8}, {7, 8}, {8, 8}, {9, 8}, {1023, 1024}, {1024, 1024}, {1025, 1024}, {2047, 2048},
                                  {2048, 2048}, {2049, 2048}, {4095, 1024}, {4096, 1024}, {4097, 1024}, {4097, 2048}, {70001, 2048},
                                  {100003, 2048}, {100003, 1}, {1000003, 2048}};
    for (size_t i = 0; i < sizeof(singles) / sizeof(singles[0]); ++i) {
        const std::vector<int64_t> counts = {singles[i][0]};
        const uint64_t step = (1ull << 32) - 3 + i;                       // across the 32-bit carry of the step
        compare(run(counts, (int)singles[i][1], step, false), counts, (int)singles[i][1], step);
    }
    // rows nothing can be drawn from: zeros, the flag, the others untouched by it
    {
        const std::vector<int64_t> counts = {12, 0, 9000, -4, 3, (int64_t)1 << 31, ((int64_t)1 << 31) + 5};
        const Run r = run(counts, 8, 3, false);
        compare(r, counts, 8, 3);
        for (int c = 0; c < 8; ++c) EXPECT(r.choice[8 + c] == 0 && r.choice[24 + c] == 0 && r.choice[40 + c] == 0 && r.choice[48 + c] == 0);
    }
    // flags off: the constants
    {
        const std::vector<int64_t> counts = {9, 100, 5000};
        const Run r = run(counts, 16, 2, false, nullptr, nullptr, 0, 0);
        EXPECT(r.rc == 0);
        for (int b = 0; b < 3; ++b) EXPECT(r.coin[b] == 0.0 && r.normal[b] == 0.0 && r.hshift[b] == 0.5);
    }
    // the optional composition: exactly sized sub, rows with and without a slice, a slice shorter than N, one over the cap
    {
        const std::vector<int64_t> counts = {9000, 40, 6000, 7, 50000};
        const int lens[5] = {2048, 0, 5, 0, 4500};
        std::vector<int32_t> sub;
        std::vector<int64_t> sub_off(6, 0);
        for (int b = 0; b < 5; ++b) {
            for (int k = 0; k < lens[b]; ++k) sub.push_back((int32_t)(((int64_t)k * 7919 + b) % counts[b]));
            sub_off[b + 1] = (int64_t)sub.size();
        }
        compare(run(counts, 16, 9, false, &sub, &sub_off), counts, 16, 9, &sub, &sub_off);
        compare(run(counts, 2048, 9, false, &sub, &sub_off), counts, 2048, 9, &sub, &sub_off);
    }
    // refusals: nothing is written
    {
        const std::vector<int64_t> counts = {4, 40};
        std::vector<int32_t> choice(16, -7), sub(1, 0);
        std::vector<int64_t> sub_off(3, 0);
        std::vector<double> f(2, -1.0);
        int64_t state = 5;
        int32_t status = 0;
        fcn_draw_desc d = {2, 8, 1, 1}, d0 = {0, 8, 1, 1}, dn = {2, 0, 1, 1}, dl = {2, max_n + 1, 1, 1};
#define CALL(D, C, S, SO, ST, CH, CO, NO, SS) fcn_draw_batch(D, C, S, SO, SEED, ST, CH, CO, NO, f.data(), SS, nullptr)
        EXPECT(CALL(nullptr, counts.data(), nullptr, nullptr, &state, choice.data(), f.data(), f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&d, nullptr, nullptr, nullptr, &state, choice.data(), f.data(), f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&d, counts.data(), sub.data(), nullptr, &state, choice.data(), f.data(), f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&d, counts.data(), nullptr, sub_off.data(), &state, choice.data(), f.data(), f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&d, counts.data(), nullptr, nullptr, nullptr, choice.data(), f.data(), f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&d, counts.data(), nullptr, nullptr, &state, nullptr, f.data(), f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&d, counts.data(), nullptr, nullptr, &state, choice.data(), nullptr, f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&d, counts.data(), nullptr, nullptr, &state, choice.data(), f.data(), nullptr, &status) == FCN_E_BADARG);
        EXPECT(CALL(&d, counts.data(), nullptr, nullptr, &state, choice.data(), f.data(), f.data(), nullptr) == FCN_E_BADARG);
        EXPECT(CALL(&d0, counts.data(), nullptr, nullptr, &state, choice.data(), f.data(), f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&dn, counts.data(), nullptr, nullptr, &state, choice.data(), f.data(), f.data(), &status) == FCN_E_BADARG);
        EXPECT(CALL(&dl, counts.data(), nullptr, nullptr, &state, choice.data(), f.data(), f.data(), &status) == FCN_E_LIMIT);
        EXPECT(state == 5 && status == 0 && f[0] == -1.0);
        for (int i = 0; i < 16; ++i) EXPECT(choice[i] == -7);
        // hshift is optional
        EXPECT(fcn_draw_batch(&d, counts.data(), nullptr, nullptr, SEED, &state, choice.data(), f.data(), f.data(), nullptr, &status, nullptr) == 0);
        EXPECT(state == 6);
    }
    // ---- the small instantiation: 2-bit digits, 64 composites in LDS -- the refine loop runs until a bin fits, up to 32 digits deep
    {
        const int Ns2[6] = {1, 2, 7, 33, 63, 64};
        for (int ni = 0; ni < 6; ++ni) {
            const int N = Ns2[ni];
            const std::vector<int64_t> counts = {1, 5, N, N + 1, 63, 64, 65, 66, 100, 129, 257, 1000, 1023, 2049, 4099, 5000, 3, 777};
            compare(run(counts, N, 100 + ni, true), counts, N, 100 + ni);
        }
        DrawArgs a;
        memset(&a, 0, sizeof(a));
        a.B = 1; a.N = 65;
        EXPECT((draw_batch_launch<2, 64>(a, nullptr)) == FCN_E_LIMIT);     // N beyond what the LDS array holds: refused before the launch
    }
    if (fails == 0) printf("all ok\n");
    return fails ? 1 : 0;
}
