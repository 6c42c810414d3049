// ufm_relax_early.inc -- early hand-off of border values and in-visit refresh of the halo (resident kernel, node planners, 16 waves per visit).
// Included INSIDE the tile loop of k_relax (ufm_relax.h): lambdas over the visit's locals (gt, tx, ty, ring, Gs, Os, s_emin, s_qw, own_slot_now ...).
// DESIGN.md section 4.8.
        // the wave's early stores have to have arrived before a neighbour is told (as in the write-back: stores, wait, queue words)
        auto ew_flush = [&]() {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            int t_ = tid;
            asm volatile("" : "+v"(t_));
            const int l_ = t_ & 63;
            if (l_ < 9 && l_ != 4) {
                int *bm = s_emin + (t_ >> 6) * 9;
                const int v = __hip_atomic_exchange(&bm[l_], INFBITS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (v != INFBITS) {
                    const int ntx = tx + l_ / 3 - 1, nty = ty + l_ % 3 - 1;
                    if (ntx >= 0 && ntx < P.TX && nty >= 0 && nty < P.TY) own_push(P, m * P.NTm + ntx * P.TY + nty, v, gt);
                }
            }
            ew_pend = 0;
        };
        // In-visit refresh, the other half of the early hand-off: a neighbour that hands its border out while this tile is being
        // visited lowers this tile's queue word (MARK -> a priority).  Idle waves look at the word now and then (a load straight into
        // LDS, nobody waits for it); the one that finds it changed takes the activation back (exchange -> MARK, waited for: its values
        // are then visible), reloads the ring record into the LDS halo and wakes the border patches on the sides that changed --
        // the visit carries on with the new inputs instead of ending, being written back, queued, taken and staged again.
        auto halo_poll = [&]() {
            typedef __attribute__((address_space(3))) void *lds_ptr;
            typedef const __attribute__((address_space(1))) void *glb_ptr;
            if (lane == 0) __builtin_amdgcn_global_load_lds((glb_ptr)(P.own_prio + own_slot_now), (lds_ptr)s_qw, 4, 0, 16);
        };
        auto halo_refresh = [&]() -> bool {      // true: this wave did a refresh (it has left the idle count meanwhile)
            int seen = __hip_atomic_load(&s_qw[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (seen >= INFBITS) return false;           // (still my mark)
            int mine = 0;
            if (lane == 0) mine = atomicCAS(&s_qw[0], seen, OWN_MARK) == seen;
            if (!__builtin_amdgcn_readfirstlane(mine)) return false;
            if (lane == 0) { atomicSub(&s_idle, 1); s_qw[1] += 1; }
            diag_refresh_claimed(gt);
            int was = OWN_MARK;
            if (lane == 0) was = __hip_atomic_exchange(&P.own_prio[own_slot_now], OWN_MARK + (int)blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            was = __builtin_amdgcn_readfirstlane(was);
            UFM_STRICT_ACQUIRE();
            diag_refresh_taken(gt, P.TY, was);
            if (was < INFBITS) {                 // (an activation: its values were stored before it was queued)
                if (lane == 0) atomicMin(&s_emin[w * 9 + 4], was);   // (its priority counts for the tile's own, should the visit end at the sweep cap)
                int t_ = tid;
                asm volatile("" : "+v"(t_));
                const int l_ = t_ & 63;
                const float h0 = ld_f<true>(&ring[l_]);
                const float h1 = ld_f<true>(&ring[64 + (l_ & 3)]);
                int sides = 0;                   // 1 top, 2 bottom, 4 left, 8 right
                auto put = [&](int ht, float v) {
                    int hr, hc, sd;
                    if (ht < T) { hr = -1; hc = ht; sd = 1; }
                    else if (ht < 2 * T) { hr = T; hc = ht - T; sd = 2; }
                    else if (ht < 3 * T) { hr = ht - 2 * T; hc = -1; sd = 4; }
                    else if (ht < 4 * T) { hr = ht - 3 * T; hc = T; sd = 8; }
                    else { hr = (ht & 2) ? T : -1; hc = (ht & 1) ? T : -1; sd = ((ht & 2) ? 2 : 1) | ((ht & 1) ? 8 : 4); }
                    float *d = &Gs[(hr + 1) * GP + hc + 1];
                    if (*d != v) { *d = v; sides |= sd; }
                };
                put(l_, h0);
                if (l_ < 4) put(64 + l_, h1);
                for (int o_ = 32; o_; o_ >>= 1) sides |= __shfl_xor(sides, o_);
                UFM_SWEEP_FENCE();               // values before wake bits
                if (sides && l_ < PT * PT) {
                    const int pr_ = l_ / PT, pc_ = l_ % PT;
                    const bool hit = ((sides & 1) && pr_ == 0) || ((sides & 2) && pr_ == PT - 1) || ((sides & 4) && pc_ == 0) || ((sides & 8) && pc_ == PT - 1);
                    if (hit) {
                        int wv, bit;
                        if constexpr (SKEW) { wv = (pr_ + 2 * pc_) & 7; bit = (pc_ == (wv < 4 ? 0 : (wv >> 1) - 1)) ? 1 : 2; }
                        else { wv = (pr_ / PR) * 4 + (pc_ / PR); bit = 1 << ((pr_ % PR) * PR + (pc_ % PR)); }
                        __hip_atomic_fetch_or(&s_wake[wv], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
            return true;
        };
