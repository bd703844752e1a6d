// exchange_plan.hpp — the host arithmetic of the multi-GPU exchange protocol (comm.hip), free of
// HIP and RCCL so that it is checked on a CPU (tests/exchange_plan_host_check.cpp).
//
// Two ranks that disagree about a message size or a round do not compute a wrong answer: they
// hang. What both ends of a message must compute alike is here, once; each end calls it with
// arguments both have seen (a count, the window number, the world size), and that is the whole
// agreement: no message carries a size.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace gsgpu {
namespace plan {

// ---- speculative slots ----
// The slot of the next speculative message after a delta of maxc pairs: twice that (at least 4K
// pairs), in steps of 1024, clamped to the pairs an export buffer holds behind its count word.
inline uint64_t next_slot(uint64_t cap_pairs, uint64_t maxc) {
    uint64_t S = std::max<uint64_t>(2 * maxc, 4096);
    S = (S + 1023) & ~(uint64_t)1023;
    return std::min<uint64_t>(S, cap_pairs - 1);
}
// the pairs [slot, n) of a delta that outgrew its slot (sent in the verification's tail round)
inline uint64_t tail_of(uint64_t n, uint64_t slot) { return n > slot ? n - slot : 0; }
// a speculative message [u64 count | slot pairs], in 32-bit words and bytes
inline uint64_t slot_words(uint64_t slot, uint64_t pair_bytes) { return 2 + pair_bytes / 4 * slot; }
inline uint64_t slot_bytes(uint64_t slot, uint64_t pair_bytes) { return slot_words(slot, pair_bytes) * 4; }

// Rank 0 receives what the senders have (exact deltas, or tails) packed in rank order: sender q's
// pairs start at pair (*off)[q]. Returns the pairs in all, which is also off->back().
inline uint64_t packed_offsets(const std::vector<uint64_t>& cnt, std::vector<uint64_t>* off) {
    off->assign(cnt.size() + 1, 0);
    for (size_t q = 0; q < cnt.size(); ++q) (*off)[q + 1] = (*off)[q] + cnt[q];
    return off->back();
}

// ---- which rounds of a gather to rank 0 are exact (counts to the host first, then exactly the pairs) ----
// The first window of a stream (no slot sized yet); every window of a world with more senders than
// a fold with per-slot capacities takes; and, for the prefilter's survivors, the first kExactYoung
// windows: their survivors are large (a padded speculative slot would move twice their bytes), and
// rank 0 folds them in one call through the young fold.
constexpr uint64_t kExactYoung = 16;
inline bool exact_round(bool young_exact, uint64_t win, bool slots_sized, int world, int max_slot_caps) {
    return (young_exact && win < kExactYoung) || !slots_sized || world > max_slot_caps;
}
// rank 0 folds an exact round's deltas one call per sender while the largest exceeds this (young
// windows: each call's short head launch makes the big joins first, cc_api.hip kMergeHead)
constexpr uint64_t kBulkDeltaPairs = 1ull << 21;

// ---- the prefilter's filter-state broadcasts (round 6) ----
// After the first kBcastSync closes the broadcast is on the critical path: the next window's filter
// waits for it (window 2 needs the giant window 1 formed; with no bitmap at all every edge of
// window 2 would go to rank 0). After that they are asynchronous (window 3 filters against close 0's
// bitmap: 3.5 M survivors at the 8-rank RMAT-26 layout instead of 2.3 M, but its filter overlaps
// rank 0's window 2; rank model P = 8 2.23 -> 2.27x, P = 4 1.77 -> 1.84x with one synchronous
// broadcast instead of two, profiles/r06_k_sim_ab.txt): a sender receives the state of close j into
// staging slot bcast_slot(j) and installs it before its filter kBcastLag windows later (a staler
// bitmap only lets more edges survive: components only merge until reset). While the giant grows
// (windows < kBcastAsyncYoung) every window's state goes out, then every kBcastAsyncEvery-th
// (8 MiB at 2^26 ids, ~130 us of link time at 64 GB/s).
constexpr uint64_t kBcastSync = 1;
constexpr uint64_t kBcastAsyncYoung = 16;
constexpr uint64_t kBcastAsyncEvery = 4;
constexpr uint64_t kBcastLag = 2;                  // installed before the filter of window j + kBcastLag
inline bool bcast_sync(uint64_t win) { return win < kBcastSync; }
inline bool bcast_async(uint64_t win) {
    return win >= kBcastSync && (win < kBcastAsyncYoung || win % kBcastAsyncEvery == kBcastAsyncEvery - 1);
}
inline int bcast_slot(uint64_t j) { return (int)(j & 1); }
// before the filter of window win: *j = the window whose state is due for install (false: none yet)
inline bool bcast_install_due(uint64_t win, uint64_t* j) {
    *j = win - kBcastLag;
    return win >= kBcastLag;
}

// ---- ConnectedComponentsTree's pairwise rounds ----
// In the round of step 2^r rank i + step sends to rank i (i % 2^(r+1) == 0); a rank that has sent is
// done for the window. After ceil(log2 world) rounds rank 0 holds every edge.
struct TreeRole { enum Kind { Idle, Send, Recv } kind; int peer; };
inline TreeRole tree_role(int rank, int world, int step) {
    if (rank % (2 * step) == step) return {TreeRole::Send, rank - step};
    if (rank % (2 * step) == 0 && rank + step < world) return {TreeRole::Recv, rank + step};
    return {TreeRole::Idle, -1};
}

}  // namespace plan
}  // namespace gsgpu
