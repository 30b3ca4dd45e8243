// ptnn_rank_plan.hpp -- how ptnn_rank_convergence (ptnn_analysis.hip) divides its scratch budget and its
// quantities into blocks.  Host arithmetic alone, with no HIP in it: ptnn_analysis.hip includes it, and so does
// tests/rank_plan_check.cpp, which walks the blocks of a few arguments under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>

namespace ptnn {

// The pooled kept draws of one quantity at the most.  The bitonic sort counts in int and doubles its span once past the segment:
// 2^29 words keep that within int.
constexpr long long RANK_MAX_POOLED = 1LL << 29;
constexpr int RANK_MAX_GRID_Y = 65535;       // segments of one launch: a segment per grid.y

// Q quantities of C chains with h kept draws per half chain under `budget` bytes of scratch: the words per segment, the bytes of
// one quantity and the quantities per block.  Half the budget is the sort's and the series', half is conv_drive's.  The pooled
// pass has a segment per quantity, the per-chain pass one per quantity and chain: only the latter's block shrinks with C.
struct RankPlan {
    long long L, npow, npow_chain;      // kept draws of a quantity; words of its segment, and of one chain's
    std::size_t key_words;              // sort words of one quantity (the larger of the two passes' where both run)
    std::size_t per_q, conv_budget;
    int Qb, Qb_chain;                   // quantities per block of the pooled and of the per-chain pass (Qb_chain <= Qb)
};
inline RankPlan rank_plan(int C, int h, int Q, bool per_chain, std::size_t budget) {
    RankPlan p{};
    p.L = 2LL * C * h;
    p.npow = 2; while (p.npow < p.L) p.npow <<= 1;
    p.npow_chain = 2; while (p.npow_chain < 2LL * h) p.npow_chain <<= 1;
    p.key_words = (std::size_t)(per_chain ? std::max(p.npow, p.npow_chain * C) : p.npow);
    p.per_q = sizeof(unsigned long long) * p.key_words + sizeof(double) * (std::size_t)p.L + sizeof(int);
    const std::size_t half = budget / 2;
    p.conv_budget = std::max<std::size_t>(1, budget - half);
    p.Qb = (int)std::max<std::size_t>(1, std::min<std::size_t>({half / p.per_q, (std::size_t)Q, (std::size_t)RANK_MAX_GRID_Y}));
    p.Qb_chain = std::min(p.Qb, std::max(1, RANK_MAX_GRID_Y / C));
    return p;
}

}  // namespace ptnn
