// TEST INFRASTRUCTURE ONLY.  A stand-alone host program (its own main, nothing loaded into python) that drives the epoch sampler --
// fcn_epoch_pick / fcn_epoch_pick_limits, csrc/epoch_pick.h compiled for the host against tests/host_harness/hip_emu -- with
// exactly sized buffers, and a SMALL instantiation of the same kernel (DIGIT_BITS = 2, SORT_CAP = 64, G up to 5000) that drives both
// boundary walks of the rank-window select many digits deep, which the production sizes do not reach.  Every window of two epochs
// is compared with a plain std::sort of the composites.  Built with -fsanitize=address,undefined by
// tests/test_epoch_pick_sanitizer.py, so a read or write past any buffer is a report, not luck.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#define FCN_DRAWS_NO_ENTRY 1                       // the C entries live in inputs.hip's translation unit
#include "frustum_convnet_amd/csrc/epoch_pick.h"
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static const uint64_t SEED = 0x0123456789ABCDEFull;

// the contract, the plain way: every composite of epoch e, std::sort
static std::vector<int32_t> ref_perm(uint64_t e, int64_t G)
{
    const uint32_t c2 = (uint32_t)e, c3 = (uint32_t)(e >> 32) << 2, k0 = (uint32_t)SEED, k1 = (uint32_t)(SEED >> 32);
    std::vector<uint64_t> comp((size_t)G);
    uint32_t w[4];
    for (int64_t j = 0; j < G; ++j) {
        if ((j & 3) == 0) draw_philox((uint32_t)(j >> 2), 0u, c2, c3, k0, k1, w);
        comp[j] = ((uint64_t)w[j & 3] << 32) | (uint64_t)j;
    }
    std::sort(comp.begin(), comp.end());
    std::vector<int32_t> out((size_t)G);
    for (int64_t i = 0; i < G; ++i) out[i] = (int32_t)(uint32_t)comp[i];
    return out;
}

struct Run {
    std::vector<int32_t> pick;
    int64_t state[2];
    int32_t status;
    int rc;
};

// exactly sized buffers; small = the <2, 64> instantiation through the launcher, else the C entry
static Run run(int64_t G, int D, int rank, int world, int64_t e, int64_t t, bool small, int advance = 1)
{
    Run r;
    r.pick.assign((size_t)D, -7);
    r.state[0] = e; r.state[1] = t; r.status = 0;
    std::vector<int64_t> count(1, G);
    if (small) {
        EpochArgs a;
        a.count = count.data(); a.D = D; a.rank = rank; a.world = world; a.advance = advance; a.seed = SEED; a.state = r.state;
        a.pick = r.pick.data(); a.status = &r.status;
        r.rc = epoch_pick_launch<2, 64>(a, nullptr);
    } else {
        r.rc = fcn_epoch_pick(count.data(), D, rank, world, SEED, r.state, advance, r.pick.data(), &r.status, nullptr);
    }
    return r;
}

// every window of epochs e0 and e0 + 1, every rank, walked through the state the kernel leaves behind
static void walk(int64_t G, int D, int world, int64_t e0, bool small)
{
    const int64_t T = G / ((int64_t)D * world);
    std::vector<int64_t> e(world, e0), t(world, 0);
    for (int ep = 0; ep < 2; ++ep) {
        const std::vector<int32_t> perm = ref_perm((uint64_t)(e0 + ep), G);
        for (int64_t turn = 0; turn < T; ++turn)
            for (int rank = 0; rank < world; ++rank) {
                EXPECT(e[rank] == e0 + ep && t[rank] == turn);
                const Run r = run(G, D, rank, world, e[rank], t[rank], small);
                EXPECT(r.rc == 0 && r.status == 0);
                const int64_t r0 = (turn * world + rank) * D;
                if (memcmp(r.pick.data(), perm.data() + r0, sizeof(int32_t) * (size_t)D) != 0) {
                    printf("FAIL window: G = %lld, D = %d, world %d, rank %d, epoch %lld, turn %lld%s\n", (long long)G, D, world, rank,
                           (long long)(e0 + ep), (long long)turn, small ? " (small)" : "");
                    ++fails;
                }
                e[rank] = r.state[0]; t[rank] = r.state[1];
            }
    }
    for (int rank = 0; rank < world; ++rank) EXPECT(e[rank] == e0 + 2 && t[rank] == 0);
}

static void failure(int64_t G, int D, int rank, int world, int64_t e, int64_t t, bool small)
{
    const Run r = run(G, D, rank, world, e, t, small);
    EXPECT(r.rc == 0 && r.status == 1 && r.state[0] == e && r.state[1] == t);
    for (int i = 0; i < D; ++i) EXPECT(r.pick[i] == 0);
}

int main()
{
    int max_d = 0, cap = 0;
    EXPECT(fcn_epoch_pick_limits(&max_d, &cap) == 0 && max_d == DRAW_MAX_N && cap == DRAW_SORT_CAP);
    EXPECT(fcn_epoch_pick_limits(nullptr, &cap) == FCN_E_BADARG && fcn_epoch_pick_limits(&max_d, nullptr) == FCN_E_BADARG);
    // ---- the production instantiation: both paths and the edge between them, whole epochs at small G, chosen turns at large G
    {
        const int64_t whole[][3] = {{1, 1, 1}, {2, 1, 1}, {5, 2, 1}, {256, 256, 1}, {257, 16, 1}, {4095, 48, 1}, {4096, 2048, 1},
                                    {4097, 48, 1}, {5000, 7, 3}, {5000, 1024, 2}};
        for (size_t i = 0; i < sizeof(whole) / sizeof(whole[0]); ++i)
            walk(whole[i][0], (int)whole[i][1], (int)whole[i][2], ((int64_t)1 << 32) - 1, false);       // across the carry of the epoch
        const int64_t G = 70001;
        const std::vector<int32_t> perm = ref_perm(5, G);
        const int Ds[3] = {1, 48, 2048};
        for (int di = 0; di < 3; ++di) {
            const int D = Ds[di];
            const int64_t T = G / D, turns[4] = {0, 1, T / 2, T - 1};
            for (int k = 0; k < 4; ++k) {
                const Run r = run(G, D, 0, 1, 5, turns[k], false);
                EXPECT(r.rc == 0 && r.status == 0 && memcmp(r.pick.data(), perm.data() + turns[k] * D, sizeof(int32_t) * (size_t)D) == 0);
                EXPECT(turns[k] + 1 < T ? (r.state[0] == 5 && r.state[1] == turns[k] + 1) : (r.state[0] == 6 && r.state[1] == 0));
            }
        }
        const Run keep = run(G, 48, 0, 1, 5, 7, false, 0);             // advance = 0: the state stays
        EXPECT(keep.rc == 0 && keep.state[0] == 5 && keep.state[1] == 7);
    }
    // ---- the defined failures: zeros, bit 0, the state as it was
    for (int small = 0; small < 2; ++small) {
        failure(0, 8, 0, 1, 0, 0, small);
        failure(-3, 8, 0, 1, 0, 0, small);
        failure((int64_t)1 << 31, 8, 0, 1, 0, 0, small);
        failure(15, 8, 0, 2, 0, 0, small);                             // D * world > G
        failure(100, 8, 1, 2, 3, 6, small);                            // t = T
        failure(100, 8, 1, 2, 3, -1, small);
        failure(100, 8, 1, 2, -1, 0, small);
        failure(5000, 8, 1, 2, 3, 312, small);
    }
    // ---- refusals: nothing is written
    {
        std::vector<int64_t> count(1, 100);
        std::vector<int32_t> pick(8, -7);
        int64_t state[2] = {3, 4};
        int32_t status = 0;
        EXPECT(fcn_epoch_pick(nullptr, 8, 0, 1, SEED, state, 1, pick.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_epoch_pick(count.data(), 8, 0, 1, SEED, nullptr, 1, pick.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_epoch_pick(count.data(), 8, 0, 1, SEED, state, 1, nullptr, &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_epoch_pick(count.data(), 8, 0, 1, SEED, state, 1, pick.data(), nullptr, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_epoch_pick(count.data(), 0, 0, 1, SEED, state, 1, pick.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_epoch_pick(count.data(), 8, 0, 0, SEED, state, 1, pick.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_epoch_pick(count.data(), 8, -1, 1, SEED, state, 1, pick.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_epoch_pick(count.data(), 8, 1, 1, SEED, state, 1, pick.data(), &status, nullptr) == FCN_E_BADARG);
        EXPECT(fcn_epoch_pick(count.data(), max_d + 1, 0, 1, SEED, state, 1, pick.data(), &status, nullptr) == FCN_E_LIMIT);
        EXPECT(state[0] == 3 && state[1] == 4 && status == 0);
        for (int i = 0; i < 8; ++i) EXPECT(pick[i] == -7);
        EpochArgs a;
        memset(&a, 0, sizeof(a));
        a.count = count.data(); a.state = state; a.pick = pick.data(); a.status = &status; a.D = 65; a.world = 1;
        EXPECT((epoch_pick_launch<2, 64>(a, nullptr)) == FCN_E_LIMIT);     // D beyond what the LDS array holds: refused before the launch
    }
    // ---- the small instantiation: 2-bit digits, 64 composites in LDS -- both walks run until a bin fits, up to 32 digits deep
    {
        const int64_t cases[][3] = {{1, 1, 1}, {5, 2, 1}, {64, 64, 1}, {64, 7, 1}, {65, 7, 1}, {65, 64, 1}, {66, 33, 2}, {100, 1, 1},
                                    {129, 16, 1}, {257, 63, 1}, {1000, 64, 1}, {1023, 33, 3}, {2049, 64, 2}, {4099, 64, 1},
                                    {5000, 64, 1}, {5000, 50, 1}, {5000, 7, 3}, {777, 3, 1}};
        for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i)
            walk(cases[i][0], (int)cases[i][1], (int)cases[i][2], 100 + (int64_t)i, true);
    }
    if (fails == 0) printf("all ok\n");
    return fails ? 1 : 0;
}
