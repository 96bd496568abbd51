// dev / test: the forward-graph replacement policy (csrc/qv_graph_policy.h) on hand-written key sequences -- host only, no GPU.
//
//     c++ -std=c++17 -fsanitize=address,undefined tools/fwd_graph_policy_check.cpp -o fwd_graph_policy_check && ./fwd_graph_policy_check
//
// Exit status 0 when every rule holds; tests/test_fwd_graph_policy_host.py builds and runs it.
#include "../offline-tarteel_amd/csrc/qv_graph_policy.h"

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

namespace {

constexpr int N = 4;   // QV_FWD_GRAPHS
using Cache = FwdGraphCache<std::string, int, N>;

// what qv_model_forward does around the policy, with a counter in place of a graph: handles are the capture's serial number
struct Ctx {
    Cache c;
    int captures = 0, launches = 0, destroyed = 0, plain = 0, serial = 0;
    bool capture_fails = false;
    Cache::Plan fwd(const std::string &key) {
        Cache::Plan p = c.next(key), asked = p;
        if (p.act == Cache::CAPTURE) {
            if (capture_fails) { c.disabled = true; p.act = Cache::PLAIN; }
            else {
                if (p.evict) ++destroyed;
                c.store(p.slot, key, ++serial);
                ++captures;
                p.act = Cache::REPLAY;
            }
        }
        if (p.act == Cache::REPLAY) { CHECK(c.slot[p.slot].key == key && c.slot[p.slot].handle > 0); ++launches; }
        else ++plain;
        return asked;
    }
};

void fills_its_slots_at_first_sight() {
    Ctx x;
    const char *keys[N] = {"k0", "k1", "k2", "k3"};
    for (int i = 0; i < N; ++i) {
        Cache::Plan p = x.fwd(keys[i]);
        CHECK(p.act == Cache::CAPTURE && p.slot == i && !p.evict);
    }
    CHECK(x.c.n == N && x.captures == N && x.c.last_capture == N && x.c.tick == N);
    for (int i = 0; i < N; ++i) {
        Cache::Plan p = x.fwd(keys[i]);
        CHECK(p.act == Cache::REPLAY && p.slot == i && x.c.slot[i].last_use == N + 1 + i);
    }
    CHECK(x.captures == N && x.launches == 2 * N && x.plain == 0);
    // a key that was captured at first sight was entered into the ring on the way (it neither hit nor was there)
    CHECK(x.c.n_seen == N && x.c.seen[0] == "k0" && x.c.seen[N - 1] == "k3");
}

void a_full_cache_captures_only_a_key_that_came_back_and_only_after_the_pause() {
    Ctx x;
    for (const char *k : {"k0", "k1", "k2", "k3"}) x.fwd(k);                  // ticks 1..4, last capture at 4
    CHECK(x.fwd("new").act == Cache::PLAIN);                                  // tick 5: first sight of a fifth key -> ring only
    CHECK(x.c.seen[0] == "new" && x.c.seen_at == 1);
    CHECK(x.fwd("new").act == Cache::PLAIN && x.c.seen_at == 1);              // tick 6: in the ring, but 6 - 4 < 2 * N; not entered twice
    for (int t = 7; t <= 11; ++t) CHECK(x.fwd("k1").act == Cache::REPLAY);    // ticks 7..11
    CHECK(x.c.tick == 11);
    CHECK(x.fwd("never seen").act == Cache::PLAIN);                           // tick 12: pause over (12 - 4 >= 8) but not in the ring before
    Cache::Plan p = x.fwd("new");                                             // tick 13: in the ring and the pause is over
    CHECK(p.act == Cache::CAPTURE && p.evict && p.slot == 0);                 // k0 (last used at tick 1) is the least recently used
    CHECK(x.c.slot[0].key == "new" && x.c.last_capture == 13 && x.c.slot[0].last_use == 13 && x.destroyed == 1);
    CHECK(x.fwd("never seen").act == Cache::PLAIN);                           // tick 14: came back, but 14 - 13 < 8
    CHECK(x.captures == N + 1 && x.c.n == N);
}

void the_pause_is_over_at_exactly_twice_the_slots() {
    Ctx x;
    for (const char *k : {"k0", "k1", "k2", "k3"}) x.fwd(k);                  // ticks 1..4, last capture at 4
    CHECK(x.fwd("new").act == Cache::PLAIN);                                  // tick 5: into the ring
    for (int t = 6; t <= 10; ++t) x.fwd("k1");
    CHECK(x.c.tick == 10 && x.c.last_capture == 4);
    CHECK(x.fwd("new").act == Cache::PLAIN);                                  // tick 11: 11 - 4 = 2 * N - 1
    CHECK(x.fwd("new").act == Cache::CAPTURE && x.c.last_capture == 12);      // tick 12: 12 - 4 = 2 * N exactly
    CHECK(x.fwd("other").act == Cache::PLAIN);                                // tick 13: into the ring; the same from a later capture
    for (int t = 14; t <= 18; ++t) x.fwd("k1");
    CHECK(x.fwd("other").act == Cache::PLAIN);                                // tick 19: 19 - 12 = 2 * N - 1
    CHECK(x.fwd("other").act == Cache::CAPTURE && x.c.last_capture == 20);    // tick 20: 20 - 12 = 2 * N exactly
    CHECK(x.captures == N + 2 && x.destroyed == 2);
}

void the_victim_is_the_least_recently_used_slot() {
    Ctx x;
    for (const char *k : {"k0", "k1", "k2", "k3"}) x.fwd(k);
    x.fwd("e");                                                               // tick 5: into the ring
    for (const char *k : {"k0", "k1", "k3", "k0", "k1", "k3", "k0"}) x.fwd(k);   // ticks 6..12: k2 (slot 2) last used at tick 3
    Cache::Plan p = x.fwd("e");
    CHECK(p.act == Cache::CAPTURE && p.evict && p.slot == 2 && x.c.slot[2].key == "e");
    CHECK(x.fwd("k2").act == Cache::PLAIN);                                   // the evicted key no longer hits
}

void the_ring_holds_the_last_uncaptured_keys_only() {
    Ctx x;
    for (const char *k : {"k0", "k1", "k2", "k3"}) x.fwd(k);
    for (const char *k : {"r0", "r1", "r2", "r3", "r4"}) x.fwd(k);            // ticks 5..9: r0 is pushed out of the ring by r4
    CHECK(x.c.seen[0] == "r4" && x.c.seen[1] == "r1" && x.c.seen_at == 1);
    for (int i = 0; i < 3; ++i) x.fwd("k0");                                  // ticks 10..12: hits leave the ring alone
    CHECK(x.c.seen[0] == "r4" && x.c.seen_at == 1);
    CHECK(x.fwd("r0").act == Cache::PLAIN && x.c.seen[1] == "r0");            // tick 13: pause over, but r0 had left the ring: entered again
    CHECK(x.fwd("r3").act == Cache::CAPTURE);                                 // tick 14: r3 is still in it
}

void a_disabled_context_never_captures_again() {
    Ctx x;
    x.fwd("k0");
    x.capture_fails = true;
    CHECK(x.fwd("k1").act == Cache::CAPTURE && x.c.disabled && x.c.n == 1);   // the capture was asked for and failed: nothing stored
    x.capture_fails = false;
    for (int i = 0; i < 20; ++i) CHECK(x.fwd("k1").act == Cache::PLAIN);
    CHECK(x.fwd("k0").act == Cache::REPLAY);                                  // the graph it holds still replays
    CHECK(x.captures == 1 && x.c.last_capture == 1);
}

// the order of tests/test_gpu_forward.py::test_forward_graph_replay_equals_the_plain_launches on a two-context engine: "a" and
// "p" are one key, qv_predict_batch deals the forwards round-robin to the contexts, starting at context 0
void the_gpu_tests_order_stays_inside_its_bounds() {
    std::vector<std::string> order;
    auto add = [&](std::vector<std::string> names, int times) { for (int i = 0; i < times; ++i) order.insert(order.end(), names.begin(), names.end()); };
    add({"a"}, 6); add({"p"}, 4); add({"a", "p"}, 3);
    for (const char *b : {"b1", "b2", "b3", "b5", "b6", "b7"}) add({b}, 4);
    add({"a"}, 4); add({"b1", "p", "b7", "a", "a", "p", "p"}, 1); add({"b1", "b2", "b3"}, 5);
    Ctx ctx[2];
    for (size_t i = 0; i < order.size(); ++i) ctx[i % 2].fwd(order[i] == "p" ? "a" : order[i]);
    const int captures = ctx[0].captures + ctx[1].captures, launches = ctx[0].launches + ctx[1].launches;
    printf("replay order: %zu forwards, %d captures (%d + %d), %d graph launches, %d plain\n", order.size(), captures, ctx[0].captures,
           ctx[1].captures, launches, ctx[0].plain + ctx[1].plain);
    CHECK(8 < captures && captures <= 14);
    CHECK(launches >= (int)order.size() / 2);
    // what the policy gives for this order today: a change of these totals is a change of the policy
    CHECK(order.size() == 66 && ctx[0].captures == 6 && ctx[1].captures == 4 && launches == 52);
}

}  // namespace

int main() {
    fills_its_slots_at_first_sight();
    a_full_cache_captures_only_a_key_that_came_back_and_only_after_the_pause();
    the_pause_is_over_at_exactly_twice_the_slots();
    the_victim_is_the_least_recently_used_slot();
    the_ring_holds_the_last_uncaptured_keys_only();
    a_disabled_context_never_captures_again();
    the_gpu_tests_order_stays_inside_its_bounds();
    printf("fwd_graph_policy_check: all rules hold\n");
    return 0;
}
