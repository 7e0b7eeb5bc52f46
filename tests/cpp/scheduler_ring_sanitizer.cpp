// CPU-only harness for the KV block ring of lmdeploy_amd/csrc/scheduler.h under AddressSanitizer + UndefinedBehaviorSanitizer: the random call
// stream of scheduler_sanitizer.cpp (submit / admit / token / cancel / forget, abort) on a scheduler with set_ring(R), R small enough that most
// requests are cut to the ring and the pool is smaller than many requests' whole context.  After every call: a running request owns exactly
// min(blocks_for(prompt + max_new), R) distinct blocks, no block has two owners, free + owned == pool.  Built and run by
// tests/test_host_kv_ring.py::test_ring_scheduler_under_sanitizers (g++ -fsanitize=address,undefined).
#include "../../lmdeploy_amd/csrc/scheduler.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

using namespace tmk;

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

int main(int argc, char** argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    std::mt19937   rng(seed);
    const int      B = 5, NBLK = 7, SESSION = 2048;
    const int      R = kv_ring_blocks(40 + (int)(seed % 3) * 64, 64);  // 3, 4 or 5 blocks
    BatchScheduler s(B, NBLK, SESSION, 64);
    CHECK(R >= 3 && R <= 5 && s.set_ring(R) && s.ring_blocks() == R);
    std::set<int64_t> live;  // ids not yet forgotten
    long tokens = 0, cut = 0, beyond_pool = 0;
    for (int it = 0; it < 20000; ++it) {
        const int op = (int)(rng() % 100);
        if (op < 25) {  // submit: whole contexts of up to 29 blocks against a pool of 7 -- never refused for the pool while R <= pool
            const int        n = (int)(rng() % 1500), mx = (int)(rng() % 400);
            std::vector<int> ids(n > 0 ? n : 1, 7);
            int64_t          id = -1;
            const int        rc = s.submit(ids.data(), n, mx, (rng() & 1) ? 3 : -1, &id);
            CHECK(rc == 0 || rc == 1 || rc == 6);
            CHECK(!s.set_ring(R));  // too late: a submit was seen
            if (rc == 0) {
                live.insert(id);
                beyond_pool += s.blocks_for(n + mx) > NBLK;
            }
        }
        else if (op < 45) {  // admission
            for (const SchedAdmit& a : s.admit(1 + (int)(rng() % 600))) {
                const SchedRequest* r = s.find(a.id);
                CHECK(r && r->running && r->slot == a.slot && s.slot_request(a.slot) == a.id);
                const int logical = s.blocks_for((int)r->prompt.size() + r->max_new);
                CHECK((int)r->blocks.size() == (logical < R ? logical : R) && (int)r->blocks.size() == s.owned_for((int)r->prompt.size() + r->max_new));
                cut += logical > R;
            }
        }
        else if (op < 85) {  // one decode step
            for (int b = 0; b < B; ++b) {
                const int64_t id = s.slot_request(b);
                if (id < 0) {
                    continue;
                }
                const bool fin = s.on_token(b, (int)(rng() % 12));
                ++tokens;
                const SchedRequest* r = s.find(id);
                CHECK(r != nullptr && (r->status == 7) == fin && (fin ? s.slot_request(b) < 0 : s.slot_request(b) == id));
            }
        }
        else if (op < 92 && !live.empty()) {  // cancel
            auto it2 = live.begin();
            std::advance(it2, rng() % live.size());
            int slot = -2;
            CHECK(s.cancel(*it2, &slot) == 0);
            CHECK(slot == -1 || (slot >= 0 && slot < B && s.slot_request(slot) < 0));
        }
        else if (!live.empty()) {  // forget (only finished / cancelled requests go)
            auto it2 = live.begin();
            std::advance(it2, rng() % live.size());
            const SchedRequest* r   = s.find(*it2);
            const bool          fin = r && r->status != 0;
            CHECK(s.erase(*it2) == fin);
            if (fin) {
                live.erase(it2);
            }
        }
        // invariants: every block is free or owned by exactly one running request, a request never owns more than the ring
        std::set<int> seen;
        int           owned = 0, running = 0;
        for (int64_t id : live) {
            const SchedRequest* r = s.find(id);
            CHECK(r != nullptr && (int)r->blocks.size() <= R);
            for (int blk : r->blocks) {
                CHECK(blk >= 0 && blk < NBLK && seen.insert(blk).second);
            }
            owned += (int)r->blocks.size();
            running += r->running;
            CHECK(r->running ? r->status == 0 : r->blocks.empty());
        }
        CHECK(owned + s.n_free_blocks() == NBLK && running == s.n_active() && s.n_records() == live.size());
    }
    CHECK(cut > 0 && beyond_pool > 0);
    if (argc > 2) {
        s.abort_all(5);
        CHECK(s.n_active() == 0 && s.n_free_blocks() == NBLK);
    }
    std::printf("ok seed %u ring %d: %ld tokens, %ld admissions cut to the ring, %ld requests beyond the pool, %zu requests alive\n", seed, R, tokens,
                cut, beyond_pool, live.size());
    return 0;
}
