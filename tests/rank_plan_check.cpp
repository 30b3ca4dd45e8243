// The blocking arithmetic of ptnn_rank_convergence (csrc/ptnn_rank_plan.hpp) on its own: for a few (C, h, Q, per_chain, budget) the
// blocks of both passes are walked as the host loop walks them, every quantity's sort words, series and flag are touched in buffers
// of the sizes the call allocates, and the plan's invariants are checked.  tests/test_rank_plan_cpu.py builds this with
// -fsanitize=address,undefined and runs it; it prints "ok" and returns 0.
#include "ptnn_rank_plan.hpp"

#include <climits>
#include <cstdio>
#include <vector>

using ptnn::RankPlan;

static int failures = 0;
#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; }                     \
    } while (0)

struct Args { int C, h, Q; bool per_chain; std::size_t budget; };

// the invariants that need no buffer
static void check_plan(const Args& a, const RankPlan& p) {
    CHECK(p.L == 2LL * a.C * a.h);
    CHECK(p.npow >= p.L && p.npow >= 2 && (p.npow & (p.npow - 1)) == 0 && (p.npow == 2 || p.npow / 2 < p.L));
    CHECK(p.npow_chain >= 2LL * a.h && (p.npow_chain & (p.npow_chain - 1)) == 0);
    CHECK(2 * p.npow <= INT_MAX);                                       // the sort's span after its last doubling
    CHECK(p.Qb >= 1 && p.Qb <= a.Q && p.Qb <= ptnn::RANK_MAX_GRID_Y);
    CHECK(p.Qb_chain >= 1 && p.Qb_chain <= p.Qb);
    CHECK(p.Qb_chain == 1 || (long long)p.Qb_chain * a.C <= ptnn::RANK_MAX_GRID_Y);
    CHECK(p.Qb == 1 || p.per_q * (std::size_t)p.Qb <= a.budget / 2);    // one quantity always runs, more only within the budget
    CHECK(p.conv_budget >= 1 && p.conv_budget + a.budget / 2 == std::max<std::size_t>(a.budget, 1 + a.budget / 2));
    CHECK(p.key_words >= (std::size_t)p.npow && (!a.per_chain || p.key_words >= (std::size_t)(p.npow_chain * a.C)));
}

// the two passes over buffers of the call's sizes: every word, series element and flag of every block lies inside them
static void walk(const Args& a, const RankPlan& p) {
    std::vector<unsigned long long> keys(p.key_words * (std::size_t)p.Qb);
    std::vector<double> ser((std::size_t)p.L * (std::size_t)p.Qb);
    std::vector<int> seen((std::size_t)a.Q, 0);
    for (int pass = 0; pass < (a.per_chain ? 2 : 1); ++pass) {
        const int blk = pass ? p.Qb_chain : p.Qb;
        const long long npow = pass ? p.npow_chain : p.npow, Ls = pass ? 2LL * a.h : p.L;
        for (long long q0 = 0; q0 < a.Q; q0 += blk) {
            const int nq = (int)std::min<long long>(blk, a.Q - q0);
            const long long nseg = pass ? (long long)nq * a.C : nq;
            CHECK(nseg <= ptnn::RANK_MAX_GRID_Y || nq == 1);
            keys[(std::size_t)(nseg * npow) - 1] = ~0ull;               // the last word of the block's last segment
            keys[(std::size_t)((nseg - 1) * npow)] = 0;
            ser[(std::size_t)(Ls * nseg) - 1] = 1.0;                    // [Ls][nseg]: the last draw's last column
            for (int k = 0; k < nq; ++k) seen[(std::size_t)(q0 + k)] += 1;
        }
    }
    for (int q = 0; q < a.Q; ++q) CHECK(seen[(std::size_t)q] == (a.per_chain ? 2 : 1));
}

int main() {
    const std::size_t GiB = (std::size_t)1 << 30;
    const Args small[] = {
        {1, 2, 1, false, GiB},       {1, 2, 1, true, 1},         {2, 2, 63, true, GiB},     {7, 50, 65, true, 200000},
        {7, 50, 65, true, 1},        {64, 2, 300, false, GiB},   {130, 2, 3, true, 4096},   {3, 2000, 2, true, 1 << 20},
        {4, 512, 2, true, 100000},   {4, 513, 2, false, 100000}, {1, 2050, 2, true, GiB},   {256, 3, 1000, true, 1 << 22},
        {65535, 2, 5, true, 1 << 26}, {64, 2500, 40, true, 1 << 26},
    };
    for (const Args& a : small) {
        const RankPlan p = ptnn::rank_plan(a.C, a.h, a.Q, a.per_chain, a.budget);
        check_plan(a, p);
        walk(a, p);
    }
    // the benchmark's shapes and the largest arguments the call accepts: the arithmetic alone (the buffers would be the device's)
    const Args large[] = {
        {64, 2500, 17, true, GiB},          {128, 50, 17410, true, GiB},          {256, 25, 17410, true, GiB},
        {1, 1 << 28, 1, true, GiB},         {65535, 4096, INT_MAX, true, GiB},    {1 << 14, 1 << 14, INT_MAX, false, ~(std::size_t)0},
        {65535, 2, INT_MAX, true, 0},
    };
    for (const Args& a : large) {
        CHECK(2LL * a.C * a.h <= ptnn::RANK_MAX_POOLED);
        check_plan(a, ptnn::rank_plan(a.C, a.h, a.Q, a.per_chain, a.budget));
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
