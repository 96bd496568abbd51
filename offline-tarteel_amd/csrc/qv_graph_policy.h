// qv_graph_policy.h -- which forwards of one execution context replay a graph, capture one, or run as plain launches.
// Pure host logic over an opaque key and an opaque handle (no HIP here): tools/fwd_graph_policy_check.cpp runs it on a CPU.
//
// A context keeps N graphs.  It captures the first N keys it sees straight away (a serving loop is at full speed from its
// second batch).  Once the slots are taken, a key is captured only when it comes back within the context's last N uncaptured
// keys (the ring `seen`: a loop over a few staging buffers, the three passes of the 30 s path) AND at least 2 * N forwards
// have passed since the last capture; the LEAST RECENTLY USED graph makes room.  So a loop over more recurring shapes than
// slots does not pay a capture + instantiate + stream synchronise per cycle (it keeps replaying the shapes it holds and runs
// the others plain), and a stream of ever-changing ragged batches pays for N captures over the context's lifetime.
#pragma once

#include <stdint.h>

template <typename Key, typename Handle, int N>
struct FwdGraphCache {
    enum Act { PLAIN, REPLAY, CAPTURE };
    struct Plan { Act act; int slot; bool evict; };   // evict: slot[slot].handle is live and the caller's to destroy before store()
    struct Slot { Key key; Handle handle; int64_t last_use; };
    Slot slot[N] = {};
    int n = 0;
    int64_t tick = 0, last_capture = 0;   // forwards seen by the context / the one that captured last
    bool disabled = false;                // a capture failed on this context: it never captures again (its graphs still replay)
    Key seen[N] = {};                     // the context's last few keys that neither hit nor were in this ring already
    int n_seen = 0, seen_at = 0;

    // One call per forward.  REPLAY: launch slot[slot].handle.  CAPTURE: capture, then store() -- or set `disabled` and run plain.
    Plan next(const Key &key) {
        ++tick;
        int hit = -1;
        for (int i = 0; i < n; ++i)
            if (slot[i].key == key) hit = i;
        bool was_seen = false;
        for (int i = 0; i < n_seen; ++i) was_seen = was_seen || seen[i] == key;
        if (hit < 0 && !was_seen) {
            seen[seen_at] = key;
            seen_at = (seen_at + 1) % N;
            if (n_seen < N) ++n_seen;
        }
        if (hit >= 0) { slot[hit].last_use = tick; return {REPLAY, hit, false}; }
        const bool full = n >= N;
        if (disabled || (full && !(was_seen && tick - last_capture >= 2 * N))) return {PLAIN, -1, false};
        int victim = n;
        if (full) {
            victim = 0;
            for (int i = 1; i < N; ++i)
                if (slot[i].last_use < slot[victim].last_use) victim = i;
        }
        return {CAPTURE, victim, full};
    }
    // the capture next() asked for succeeded: the slot holds `handle` from this forward on
    void store(int i, const Key &key, const Handle &handle) {
        slot[i] = {key, handle, tick};
        if (i == n) ++n;
        last_capture = tick;
    }
};
