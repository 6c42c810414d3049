// ufm_relax_resident.inc -- the resident form of k_relax (OWNK = 1 | 2): how a workgroup decides what to visit next.  Included INSIDE the kernel body
// (ufm_relax.h): these are lambdas over the kernel's locals (P, tid, lane, delta, s_best, s_gmin, s_own, own_q, own_base ...).
// DESIGN.md sections 4.7 / 4.8; the in-launch memory protocol they rely on is tabulated in 4.7.
    // The decision: s_best = {priority, slot} of my best queued tile; s_gmin bit 0 = some other owner holds something, bit 1 =
    // ... something more than an ordering band below my best (which then has to wait).  From this thread's first queue word
    // and one other owner's hint.  Opens and closes with a barrier.  (No reduction tree, no same-address atomics from whole
    // waves -- either costs more than a microsecond here: a handful of lanes have a queued word, and the hints only vote.)
    auto own_decide = [&](int v0, int hint, int skip) {   // skip: the slot of the visit in progress (its turn comes again later)
        if (tid == 0) { s_best = ~0ull; s_gmin = 0; }
        lds_barrier();
        unsigned long long best = ~0ull;
#pragma unroll 1
        for (int sl = tid; sl < P.own_slots; sl += NTH) {
            const int v = (sl == tid) ? v0 : __hip_atomic_load(&own_q[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v < INFBITS && sl != skip) best = min(best, ((unsigned long long)(unsigned int)v << 32) | (unsigned int)sl);
        }
        if (best != ~0ull) atomicMin(&s_best, best);
        lds_barrier();
        const unsigned long long b = s_best;
        const bool any = hint != INFBITS;
        const bool below = any && b != ~0ull && __int_as_float((int)(b >> 32)) > __int_as_float(hint) + delta;
        const unsigned long long ba = __ballot(any), bb = __ballot(below);
        if (lane == 0 && ba) atomicOr(&s_gmin, bb ? 3 : 1);
        lds_barrier();
    };
    // An "empty" value the word cannot have held recently (the end-of-phase test relies on it: two identical all-empty collects must be a true
    // snapshot -- a word that went empty -> queued -> visited -> empty between the two passes shows another empty value).  This workgroup's
    // visit count x workgroup, the count taken modulo 16 367: a value comes back after 16 367 visits of this workgroup, the two passes of a
    // collect lie microseconds apart.  (Round 2 let a workgroup leave the launch when it ran out of values; any job size stays in the one
    // launch now.)
    auto own_empty = [&]() -> int {
        const unsigned int c = (unsigned int)s_own[2]++ % (OWN_EMPTIES / (unsigned int)OWN_NW);
        return INFBITS + 1 + (int)(c * (unsigned int)OWN_NW + blockIdx.x);
    };
    // Taking a tile (thread 0): the queue word goes from the priority it was seen with to this workgroup's mark (compare-and-swap: a mark
    // or an empty value of somebody else is never overwritten) and the tile's lock from 0 to 1 -- two atomics issued together, looked
    // at together.  With both, the tile is this workgroup's until own_release().  With the activation but not the lock (the tile is
    // being visited: the activation landed during that visit) the activation goes back into the word; with the lock but no
    // activation (the word had changed since it was looked at) the lock is released.
    auto own_take_issue = [&](int gw, int prio, int &r_old, int &r_lk) {
        int expect = prio;
        __hip_atomic_compare_exchange_strong(&P.own_prio[gw], &expect, OWN_MARK + (int)blockIdx.x, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r_old = expect;
        r_lk = __hip_atomic_exchange(&P.own_lock[gw], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto own_take_resolve = [&](int gw, int &prio, int r_old, int r_lk) -> bool {
        bool got = r_old == prio;
        if (!got && r_lk == 0 && r_old < prio) {   // still queued, only lower meanwhile (the word was chosen from an older copy): once more
            int expect = r_old;
            got = __hip_atomic_compare_exchange_strong(&P.own_prio[gw], &expect, OWN_MARK + (int)blockIdx.x, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (got) prio = r_old;
        }
        if (got && r_lk == 0) return true;
        if (got) __hip_atomic_fetch_min(&P.own_prio[gw], prio, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // (mark -> queued again)
        else if (r_lk == 0) __hip_atomic_store(&P.own_lock[gw], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
    };
    // thread 0, after a decision: take back the mark of the visit before the last (its activations have long been performed),
    // say what this workgroup holds, mark the chosen tile.  The atomics of the take are not waited for here.
    auto own_commit = [&](unsigned long long b, bool take, bool wait, int &r_old, int &r_lk) {   // wait: that visit's activations have only just been issued
        const int own_prev = s_own[0];
        if (own_prev >= 0) {
            if (wait) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int expect = OWN_MARK + (int)blockIdx.x;
            __hip_atomic_compare_exchange_strong(&P.own_prio[own_prev], &expect, own_empty(), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_own[0] = -1;
        }
        __hip_atomic_store(&P.own_min[blockIdx.x], b != ~0ull ? (int)(b >> 32) : INFBITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (take) own_take_issue(own_base + (int)(unsigned int)b, (int)(b >> 32), r_old, r_lk);
    };
    // An idle workgroup helps out.  Ownership spreads a front over the workgroups only on average: the critical path of a 4096^2 plan
    // (tools/front_timing.py) is ~330 visits long, and on it an activation waits 45 us for its visit -- 31 us of them while its owner
    // is busy with other tiles, next to workgroups that find nothing of their own inside the band.  So a workgroup with nothing to take
    // looks at the owner that holds the smallest priority (the hints), at that owner's words, and takes its best queued tile if
    // that lies inside the ordering band -- by the same take the owner uses (own_take_issue), so a tile still has one visitor at a time.
    // All threads call; returns the word taken (its priority in s_own[3]) or -1.
    // (hint: this thread's sample of the hints, ho: the owner it belongs to.  Whose words: owners whose hint lies inside the band above the
    //  smallest hint seen -- up to UFM_STEAL_VICTIMS of them, whichever lanes get there first; every workgroup samples the hints in an order of
    //  its own --, and nobody's when there is no such owner: most looks of an idle workgroup find everything queued beyond the band, and reading
    //  four owners' words AND locks at every one of them was most of the kernel's HBM traffic (DESIGN.md section 7).  The locks are not scanned:
    //  the chosen tile's lock is looked at once, by the take itself.)
    auto own_steal = [&](int hint, int ho) -> int {
        unsigned long long hk = hint != INFBITS ? (((unsigned long long)(unsigned int)hint << 32) | (unsigned int)tid) : ~0ull;
        for (int o_ = 32; o_; o_ >>= 1) hk = min(hk, (unsigned long long)__shfl_xor((long long)hk, o_));
        if (tid == 0) { s_best = ~0ull; s_gmin = -1; s_bmin[4] = 0; }
        lds_barrier();
        if (lane == 0 && hk != ~0ull) atomicMin(&s_best, hk);
        lds_barrier();
        const unsigned long long vk = s_best;
        diag_count(SDIAG_HELP_TRIES, tid == 0);
        if (vk == ~0ull) { lds_barrier(); return -1; }
        const float band_top = __int_as_float((int)(vk >> 32)) + delta;
        if (hint != INFBITS && !(__int_as_float(hint) > band_top)) {
            const int slot = atomicAdd(&s_bmin[4], 1);
            if (slot < UFM_STEAL_VICTIMS) s_bmin[slot] = ho;
        }
        lds_barrier();
        const int nv = min(s_bmin[4], UFM_STEAL_VICTIMS);
        unsigned long long bb = ~0ull;         // {priority, which of the owners looked at, slot}
        for (int vi = 0; vi < nv; ++vi) {
            const int *vq = P.own_prio + (size_t)s_bmin[vi] * P.own_slots;
#pragma unroll 1
            for (int sl = tid; sl < P.own_slots; sl += NTH) {
                const int v = __hip_atomic_load(&vq[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v < INFBITS) bb = min(bb, ((unsigned long long)(unsigned int)v << 32) | ((unsigned int)vi << 28) | (unsigned int)sl);
            }
        }
        for (int o_ = 32; o_; o_ >>= 1) bb = min(bb, (unsigned long long)__shfl_xor((long long)bb, o_));
        lds_barrier();
        if (tid == 0) s_best = ~0ull;
        lds_barrier();
        if (lane == 0 && bb != ~0ull) atomicMin(&s_best, bb);
        lds_barrier();
        if (tid == 0) {
            const unsigned long long b2 = s_best;
            diag_count(SDIAG_HELP_FOUND, b2 != ~0ull);
            if (b2 != ~0ull && !(__int_as_float((int)(b2 >> 32)) > band_top)) {
                diag_count(SDIAG_HELP_IN_BAND, true);
                const int gw = s_bmin[((unsigned int)b2 >> 28) & 15u] * P.own_slots + (int)((unsigned int)b2 & 0x0FFFFFFFu);
                int pr = (int)(b2 >> 32);
                int r_old, r_lk;
                own_take_issue(gw, pr, r_old, r_lk);
                if (own_take_resolve(gw, pr, r_old, r_lk)) {
                    s_own[3] = pr; s_gmin = gw;
                    diag_count(SDIAG_HELP_TAKEN, true);
                    __hip_atomic_fetch_min(&P.own_min[blockIdx.x], pr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // what this workgroup holds now
                }
            }
        }
        __syncthreads();
        return s_gmin;
    };
