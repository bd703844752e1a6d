// exchange_plan_host_check.cpp — the agreement arithmetic of the multi-GPU exchange
// (csrc/exchange_plan.hpp) walked on a CPU: a sender-side plan and a root-side plan, written apart
// the way comm.hip's two sides are, are fed the same per-sender counts window after window and must
// plan the same messages. Built with -fsanitize=address,undefined and run directly
// (tests/test_exchange_plan_host.py). The properties are read off the protocol (comm.hip
// gather_round / settle_gather, merge_prefilter, merge_tree), not measured.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "exchange_plan.hpp"

using namespace gsgpu::plan;

static long failures = 0, checks = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        ++checks;                                                               \
        if (!(cond) && ++failures <= 20) std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    } while (0)

constexpr int kMaxSlotCaps = 16;   // common.hpp's: the slots a fold with per-slot capacities takes
constexpr int kWindows = 40;

struct Setup {
    int world;
    uint64_t cap_pairs, pair_bytes;
    bool young_exact;              // GS_MERGE_PREFILTER (else GS_MERGE_GATHER)
};

// what one sender sends in a window: [count word] + pairs (exact), or one slot message and, at the
// window's verification, its tail
struct Sent {
    bool exact;
    uint64_t slot, first_bytes, tail_bytes;
};
struct SenderPlan {
    Setup u;
    bool sized = false;
    uint64_t slot = 0, win = 0;
    Sent window(uint64_t n) {
        const bool exact = exact_round(u.young_exact, win++, sized, u.world, kMaxSlotCaps);
        sized = true;
        const Sent m{exact, slot, exact ? n * u.pair_bytes : slot_bytes(slot, u.pair_bytes),
                     exact ? 0 : tail_of(n, slot) * u.pair_bytes};
        slot = next_slot(u.cap_pairs, n);
        return m;
    }
};

// what rank 0 receives in a window from every sender, and where
struct Received {
    bool exact;
    std::vector<uint64_t> slot, first_bytes, first_at, tail_bytes, tail_at;   // per sender; *_at in bytes
    uint64_t first_room, tail_room;                                             // bytes the buffers are grown to
};
struct RootPlan {
    Setup u;
    std::vector<uint64_t> gslot;
    uint64_t win = 0;
    Received window(const std::vector<uint64_t>& n) {
        const int P = u.world;
        Received r;
        r.exact = exact_round(u.young_exact, win++, !gslot.empty(), P, kMaxSlotCaps);
        if (gslot.empty()) gslot.assign(P, 0);
        r.slot = gslot;
        r.first_bytes.assign(P, 0);
        r.first_at.assign(P, 0);
        r.tail_bytes.assign(P, 0);
        r.tail_at.assign(P, 0);
        r.first_room = r.tail_room = 0;
        std::vector<uint64_t> off;
        if (r.exact) {
            r.first_room = packed_offsets(n, &off) * u.pair_bytes;
            for (int q = 1; q < P; ++q) {
                r.first_bytes[q] = n[q] * u.pair_bytes;
                r.first_at[q] = off[q] * u.pair_bytes;
            }
        } else {
            uint64_t smax = 0;
            for (int q = 1; q < P; ++q) smax = std::max(smax, gslot[q]);
            r.first_room = (uint64_t)P * slot_bytes(smax, u.pair_bytes);
            std::vector<uint64_t> tail(P, 0);
            for (int q = 1; q < P; ++q) {
                r.first_bytes[q] = slot_bytes(gslot[q], u.pair_bytes);
                r.first_at[q] = (uint64_t)q * slot_bytes(smax, u.pair_bytes);
                tail[q] = tail_of(n[q], gslot[q]);
            }
            r.tail_room = packed_offsets(tail, &off) * u.pair_bytes;
            for (int q = 1; q < P; ++q) {
                r.tail_bytes[q] = tail[q] * u.pair_bytes;
                r.tail_at[q] = off[q] * u.pair_bytes;
            }
        }
        for (int q = 1; q < P; ++q) gslot[q] = next_slot(u.cap_pairs, n[q]);
        return r;
    }
};

// messages laid end to end from byte 0 up to `room`, in rank order (dense), or each inside its own
// stride (slots): none overlaps another or runs past the buffer
static void check_layout(const std::vector<uint64_t>& at, const std::vector<uint64_t>& bytes, uint64_t room, bool dense) {
    uint64_t end = 0;
    for (size_t q = 1; q < at.size(); ++q) {
        if (bytes[q] == 0 && dense) continue;
        CHECK(dense ? at[q] == end : at[q] >= end);
        end = at[q] + bytes[q];
    }
    CHECK(dense ? end == room : end <= room);
}

enum Shape { Constant, Growing, Burst, Zeros, Full, kShapes };
static uint64_t count_of(Shape sh, const Setup& u, int q, int w) {
    const uint64_t top = u.cap_pairs - 1;
    uint64_t n = 0;
    switch (sh) {
    case Constant: n = 5000 + 37 * (uint64_t)q; break;
    case Growing: n = (uint64_t)w * w * 300 + (uint64_t)q * (w + 1); break;
    case Burst: n = (w % 7 == 5 && q % 2 == 1) ? top - (uint64_t)q : 100 + (uint64_t)w; break;   // far past the slot
    case Zeros: n = (w % 3 == 1 && q == 1) ? 1 : 0; break;
    default: n = top; break;
    }
    return std::min(n, top);
}

static void walk(const Setup& u, Shape sh) {
    const int P = u.world;
    std::vector<SenderPlan> senders(P);
    for (auto& s : senders) s.u = u;
    RootPlan root;
    root.u = u;
    for (int w = 0; w < kWindows; ++w) {
        std::vector<uint64_t> n(P, 0);
        for (int q = 1; q < P; ++q) n[q] = count_of(sh, u, q, w);
        const Received r = root.window(n);
        // which rounds are exact: the first, every round past kMaxSlotCaps ranks, the prefilter's young ones
        const bool want_exact = w == 0 || P > kMaxSlotCaps || (u.young_exact && (uint64_t)w < kExactYoung);
        CHECK(r.exact == want_exact);
        for (int q = 1; q < P; ++q) {
            const Sent m = senders[q].window(n[q]);
            CHECK(m.exact == r.exact);
            CHECK(m.slot == r.slot[q]);
            CHECK(m.first_bytes == r.first_bytes[q]);
            CHECK(m.tail_bytes == r.tail_bytes[q]);
            if (!m.exact)                          // slot and tail together are the whole count, once
                CHECK(std::min(n[q], m.slot) * u.pair_bytes + m.tail_bytes == n[q] * u.pair_bytes);
            const uint64_t next = senders[q].slot;
            CHECK(next == root.gslot[q]);
            CHECK(next >= 1 && next <= u.cap_pairs - 1);
            CHECK(next % 1024 == 0 || next == u.cap_pairs - 1);
            CHECK(next >= std::min(n[q], u.cap_pairs - 1));   // a repeat of this count fits
        }
        check_layout(r.first_at, r.first_bytes, r.first_room, r.exact);
        check_layout(r.tail_at, r.tail_bytes, r.tail_room, true);
    }
}

// 64 windows of one prefilter sender's staging slots, as merge_prefilter drives them: install before
// the filter, receive after the round
static void walk_broadcasts() {
    int64_t held[2] = {-1, -1};
    std::set<uint64_t> received, installed;
    for (uint64_t win = 0; win < 64; ++win) {
        uint64_t j = 0;
        if (bcast_install_due(win, &j)) {
            CHECK(j + kBcastLag == win);
            const int k = bcast_slot(j);
            if (held[k] == (int64_t)j) {
                installed.insert(j);
                held[k] = -1;
            }
        } else {
            CHECK(win < kBcastLag);
        }
        CHECK(!(bcast_sync(win) && bcast_async(win)));
        if (bcast_async(win)) {
            const int k = bcast_slot(win);
            CHECK(k == 0 || k == 1);
            CHECK(held[k] == -1);                  // its previous state was installed (or there was none)
            held[k] = (int64_t)win;
            received.insert(win);
        }
    }
    // every state received in window j was installed in window j + kBcastLag (those still in flight
    // at the end aside), and nothing else was
    for (uint64_t j : received) CHECK(j + kBcastLag >= 64 || installed.count(j) == 1);
    for (uint64_t j : installed) CHECK(received.count(j) == 1);
    CHECK(bcast_sync(0) && !bcast_async(0) && bcast_async(kBcastSync));
    for (uint64_t win = kBcastAsyncYoung; win < 64; ++win)
        CHECK(bcast_async(win) == (win % kBcastAsyncEvery == kBcastAsyncEvery - 1));
}

static void walk_tree(int P) {
    std::vector<int> sends(P, 0);
    for (int step = 1; step < P; step *= 2) {
        for (int r = 0; r < P; ++r) {
            const TreeRole me = tree_role(r, P, step);
            if (me.kind == TreeRole::Idle) continue;
            CHECK(me.peer >= 0 && me.peer < P && me.peer != r);
            if (me.peer < 0 || me.peer >= P) continue;
            const TreeRole peer = tree_role(me.peer, P, step);
            CHECK(peer.peer == r);
            CHECK(peer.kind == (me.kind == TreeRole::Send ? TreeRole::Recv : TreeRole::Send));
            if (me.kind == TreeRole::Send) {
                CHECK(sends[r] == 0);              // a rank that has sent is done for the window
                ++sends[r];
            }
        }
    }
    CHECK(sends[0] == 0);
    for (int r = 1; r < P; ++r) CHECK(sends[r] == 1);
}

int main() {
    const int worlds[] = {2, 3, 8, 16, 17};
    const uint64_t caps[] = {2ull << 10, 2ull << 16, 2ull << 26};   // (2 x 1024: every slot is clamped)
    for (int P : worlds) {
        for (uint64_t cap : caps)
            for (uint64_t pb : {8ull, 16ull})
                for (bool young : {false, true}) {
                    if (young && pb == 16) continue;                   // the prefilter is dense-only
                    for (int sh = 0; sh < kShapes; ++sh) walk(Setup{P, cap, pb, young}, (Shape)sh);
                }
        walk_tree(P);
    }
    walk_broadcasts();
    // next_slot's floor, step and clamp; the tail
    CHECK(next_slot(1 << 20, 0) == 4096 && next_slot(1 << 20, 2048) == 4096 && next_slot(1 << 20, 2049) == 5120);
    CHECK(next_slot(1 << 20, 1 << 20) == (1 << 20) - 1 && next_slot(2048, 0) == 2047);
    CHECK(tail_of(10, 10) == 0 && tail_of(11, 10) == 1 && tail_of(0, 10) == 0);
    if (failures) {
        std::fprintf(stderr, "exchange_plan_host_check: %ld of %ld checks failed\n", failures, checks);
        return 1;
    }
    std::printf("exchange_plan_host_check OK (%ld checks)\n", checks);
    return 0;
}
