// ufm_diag.h -- everything the two diagnostic builds add to the kernels: their globals, what every index of them means, and the hooks the kernels call
// (a piece of ufm_engine.hip, the engine's one translation unit: included there first, inside its anonymous namespace; the host readers of the
//  globals, ufm_debug_*, are ufm_diag_host.h)
//
//   -DUFM_TIMING     libufm_timing.so   100 MHz wall-clock stamps of tile visits, per-tile and per-visit records, an event log, launch and wave traces
//   -DUFM_SWEEPSTAT  libufm_sstat.so    what the patch sweeps of k_relax find
//
// A hook is the recording code in its diagnostic build and an EMPTY inline function in every other build: its arguments are values the kernel
// computes anyway or pure expressions the compiler drops, so the product and the checking build compile to the same instructions with and without the
// calls (held by comparing the device assembly: tools/device_code_diff.py).  A hook that contains a barrier or a ballot in its diagnostic build
// (DiagVisit::staged, DiagVisit::end, diag_sweep) is called by all threads.  Both builds are slower than the product -- every record is a same-address atomic --
// and compute the same field (tests/test_gpu_diag_builds.py).
#pragma once

// ---- the slots: the tools under tools/ decode every array below by these numbers -----------------------------------------
// g_sdiag[16] (UFM_TIMING; ufm_debug_sdiag): the looks of workgroups of the resident kernel that have no tile
enum {
    SDIAG_LOOKS = 0,          // looks
    SDIAG_LOOKS_EMPTY = 1,    // ... with nothing to take
    SDIAG_HELP_TRIES = 2,     // helping attempts (own_steal)
    SDIAG_HELP_FOUND = 3,     // ... a victim's queued word found
    SDIAG_HELP_IN_BAND = 4,   // ... inside the ordering band
    SDIAG_HELP_TAKEN = 5,     // ... taken
    SDIAG_AHEAD_FAILED = 6,   // takes ahead (chosen during the previous visit) that failed
    SDIAG_FRESH_FAILED = 7,   // takes after a fresh look that failed
};                            // 8..15 unused
// g_tdiag[64] (UFM_TIMING; ufm_debug_tdiag): lowering visits of k_relax in all its forms, times in 10 ns ticks of the constant 100 MHz counter
enum {
    TDIAG_STAGE = 0,          // sum of pop -> staged
    TDIAG_SWEEP = 1,          // sum of the sweep phases
    TDIAG_WRITEBACK = 2,      // sum of write-back and activations
    TDIAG_VISITS = 3,         // visits timed
    //          4, 5             not written (once: per-workgroup busy time, workgroups)
    TDIAG_REFRESHES = 6,      // in-visit refreshes (early hand-off form)
    TDIAG_TIME_HIST = 8,      // 8..39: histogram of visit times, 2 us bins, the last one open
    TDIAG_SWEEP_HIST = 40,    // 40..63: histogram of the largest per-wave sweep count of a visit, the last bin open
};
// g_tile[5][TILE_DIAG_MAX] (UFM_TIMING; ufm_debug_tiles), per tile of the resident kernel, 100 MHz ticks since the phase began (g_tile_t0, k_own_import)
enum {
    TILE_FIRST = 0,           // start of the first visit (0xFFFFFFFF: none)
    TILE_LAST_CHANGE = 1,     // end of the last visit that changed a value
    TILE_PUSHED = 2,          // earliest activation not yet taken (0xFFFFFFFF: none)
    TILE_VISITS = 3,          // visits
    TILE_WAIT = 4,            // sum of activation -> visit start
};
// g_push64[TILE_DIAG_MAX]: per tile {time << 32 | sender} of the earliest activation not yet taken (~0: none)
// g_vis[VIS_DIAG_MAX][5], g_nvis (ufm_debug_visits), the visits of the resident kernel, for the critical path:
//     {tile, start, end, time of the earliest activation the visit took, tile that sent it}
// g_plog[PLOG_MAX][4], g_nplog (ufm_debug_plog), events around the corner tiles (0..1, 0..1) of map 0: {time, a, b, c}; b is a tag below, or else
//     the record is an activation a -> b with priority c
enum : unsigned int {
    PLOG_VISIT_END = 0xFFFFFFFBu,   // a = tile, c = converged | largest per-wave sweep count << 8 | workgroup << 20
    PLOG_LOOK = 0xFFFFFFFDu,        // a look of workgroup 0 that did not end the phase: a = 0, c = its best priority
    PLOG_REFRESH = 0xFFFFFFFEu,     // in-visit refresh: a = tile, c = what the exchange returned
    PLOG_PHASE_END = 0xFFFFFFFFu,   // workgroup 0 saw the end: a = 1, c = its best priority
};
// g_trace[16384][4], g_ntrace (ufm_debug_trace), the lowering launches UFM_TRACE_K0 .. +7 of the launch chain: {launch | workgroup << 16 | kind << 40, t0, t1, x}
//     kind 0 = tile visit (pop .. end), x = largest per-wave sweep count | earlier visits << 8 | hint << 16 | +inf elements before << 24 | after << 40 | rank << 52
//     kind 1 = workgroup lifetime (entry .. exit), x = 0
// g_wtrace[16][256][2], g_nw[16] (ufm_debug_wtrace), the per-wave timeline of ONE visit (the first long-list visit of workgroup 0 in launch UFM_TRACE_K0):
//     {type << 32 | value, time}
enum {
    WREC_VISIT = 0,           // the sweeps begin; value = earlier visits of the tile in this step
    WREC_BURST = 1,           // bursts begin; value = the wake bits taken
    WREC_BURST_END = 2,       // ... end; value = the wave's sweeps so far
    WREC_IDLE = 3, WREC_WOKEN = 4, WREC_VOTE = 5,
};
// g_sstat[32] (UFM_SWEEPSTAT; ufm_debug_sstat): the patch sweeps of k_relax
enum {
    SSTAT_SWEEPS = 0,         // sweeps (16 node evaluations each)
    SSTAT_SWEEPS_QUIET = 1,   // ... that changed no node
    SSTAT_CHANGED = 2,        // node values changed
    SSTAT_BURSTS = 3,         // bursts
    SSTAT_BURSTS_QUIET = 4,   // ... whose first sweep changed nothing
    SSTAT_LOWERED = 5,        // node values lowered
    SSTAT_BURST_HIST = 8,     // 8..23: histogram of sweeps per burst (1..16)
};
// (s_qw[1] of k_relax, the in-visit refresh count: the timing build notes in this bit that the visit changed a value)
constexpr int DIAG_QW_CHANGED = 0x10000;

#ifdef UFM_SWEEPSTAT
__device__ unsigned long long g_sstat[32];
#endif
#ifdef UFM_TIMING
constexpr int TILE_DIAG_MAX = 1 << 19;
constexpr int VIS_DIAG_MAX = 1 << 20;
constexpr int PLOG_MAX = 1 << 14;
constexpr int UFM_TRACE_K0 = 300;
__device__ unsigned int g_tile[5][TILE_DIAG_MAX];
__device__ unsigned long long g_tile_t0;
__device__ unsigned long long g_sdiag[16];
__device__ unsigned long long g_push64[TILE_DIAG_MAX];
__device__ unsigned int g_vis[VIS_DIAG_MAX][5];
__device__ unsigned int g_nvis;
__device__ unsigned int g_plog[PLOG_MAX][4];
__device__ unsigned int g_nplog;
__device__ unsigned long long g_tdiag[64];
__device__ unsigned long long g_trace[4 * 16384];
__device__ unsigned int g_ntrace;
__device__ unsigned long long g_wtrace[16 * 256 * 2];
__device__ unsigned int g_nw[16];
__shared__ unsigned int s_diag_vi;   // k_relax, thread 0: the visit's index in g_vis (in LDS, not in a register carried through the sweeps)
__device__ __forceinline__ void plog(unsigned int a, unsigned int b, unsigned int c) {
    const unsigned int i = atomicAdd(&g_nplog, 1u);
    if (i < PLOG_MAX) { g_plog[i][0] = (unsigned int)(wall_clock64() - g_tile_t0); g_plog[i][1] = a; g_plog[i][2] = b; g_plog[i][3] = c; }
}
__device__ __forceinline__ void trace_rec(int k, int kind, unsigned long long t0, unsigned long long t1, long long sw) {
    if (k < UFM_TRACE_K0 || k >= UFM_TRACE_K0 + 8) return;
    const unsigned int i = atomicAdd(&g_ntrace, 1u);
    if (i >= 16384) return;
    g_trace[4 * i] = (unsigned long long)k | ((unsigned long long)blockIdx.x << 16) | ((unsigned long long)kind << 40);
    g_trace[4 * i + 1] = t0; g_trace[4 * i + 2] = t1; g_trace[4 * i + 3] = (unsigned long long)sw;
}
#endif

// ---- the hooks ---------------------------------------------------------------------------------------------------------------
// one more of g_sdiag[slot] where `on` holds
__device__ __forceinline__ void diag_count(int slot, bool on) {
#ifdef UFM_TIMING
    if (on) atomicAdd(&g_sdiag[slot], 1ull);
#endif
}
// k_own_import: a phase of the resident kernel begins -- its clock starts, the per-tile records, the visits and the event log are emptied
__device__ __forceinline__ void diag_phase_begin() {
#ifdef UFM_TIMING
    if (blockIdx.x == 0 && threadIdx.x == 0) g_tile_t0 = wall_clock64();
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < TILE_DIAG_MAX; t += gridDim.x * blockDim.x) {
        g_tile[TILE_FIRST][t] = 0xFFFFFFFFu; g_tile[TILE_LAST_CHANGE][t] = 0u; g_tile[TILE_PUSHED][t] = 0xFFFFFFFFu; g_tile[TILE_VISITS][t] = 0u; g_tile[TILE_WAIT][t] = 0u;
        g_push64[t] = ~0ull;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { g_nvis = 0u; g_nplog = 0u; }
#endif
}
// own_push: tile gt (of a map with TY tiles per row) has been queued with priority pbits by the visit of tile `from` (-1: by the import)
__device__ __forceinline__ void diag_pushed(int gt, int from, int pbits, int TY) {
#ifdef UFM_TIMING
    if (gt < TILE_DIAG_MAX) {
        const unsigned int now = (unsigned int)(wall_clock64() - g_tile_t0);
        atomicMin(&g_tile[TILE_PUSHED][gt], now);
        atomicMin(&g_push64[gt], ((unsigned long long)now << 32) | (unsigned int)from);
        if (gt / TY < 2 && gt % TY < 2) plog((unsigned int)from, (unsigned int)gt, (unsigned int)pbits);
    }
#endif
}
// k_relax, thread 0 of workgroup 0 after a look: `stop` = it has seen the end of the phase
__device__ __forceinline__ void diag_look(bool stop, unsigned int best_prio) {
#ifdef UFM_TIMING
    if (blockIdx.x == 0) plog(stop ? 1u : 0u, stop ? PLOG_PHASE_END : PLOG_LOOK, best_prio);
#endif
}
// in-visit refresh (halo_refresh, all lanes of the wave call): the wave has claimed the activation of tile gt ...
__device__ __forceinline__ void diag_refresh_claimed(int gt) {
#ifdef UFM_TIMING
    if ((threadIdx.x & 63) == 0 && gt < TILE_DIAG_MAX) atomicExch(&g_tile[TILE_PUSHED][gt], 0xFFFFFFFFu);
#endif
}
// ... and taken it back: `was` is what the exchange returned
__device__ __forceinline__ void diag_refresh_taken(int gt, int TY, int was) {
#ifdef UFM_TIMING
    if ((threadIdx.x & 63) == 0 && gt / TY < 2 && gt % TY < 2) plog((unsigned int)gt, PLOG_REFRESH, (unsigned int)was);
#endif
}
// the visit stores a changed value (wb_store): qw1 = &s_qw[1]
__device__ __forceinline__ void diag_value_changed(int *qw1) {
#ifdef UFM_TIMING
    *qw1 |= DIAG_QW_CHANGED;
#endif
}
// k_triage releases tile gt: where its priority lies inside the band [*lmin, *lmin + delta], 0..255, into rank[gt]
__device__ __forceinline__ void diag_rank(bool released, int *rank, int gt, int pbits, const int *lmin, float delta) {
#ifdef UFM_TIMING
    if (released) {
        const float lo = __int_as_float(*lmin);
        rank[gt] = (int)fminf(255.0f, fmaxf(0.0f, 255.0f * (__int_as_float(pbits) - lo) / fmaxf(delta, 1e-6f)));
    }
#endif
}
// one patch sweep (all lanes call): this lane's node changed / was lowered; `first` = the first sweep of its burst
__device__ __forceinline__ void diag_sweep(bool changed, bool lowered, bool first) {
#ifdef UFM_SWEEPSTAT
    const unsigned long long chg = __builtin_amdgcn_ballot_w64(changed), low = __builtin_amdgcn_ballot_w64(lowered);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&g_sstat[SSTAT_SWEEPS], 1ull);
        if (!chg) atomicAdd(&g_sstat[SSTAT_SWEEPS_QUIET], 1ull);
        atomicAdd(&g_sstat[SSTAT_CHANGED], (unsigned long long)__popcll(chg) / 4ull);
        atomicAdd(&g_sstat[SSTAT_LOWERED], (unsigned long long)__popcll(low) / 4ull);
        if (first) { atomicAdd(&g_sstat[SSTAT_BURSTS], 1ull); if (!chg) atomicAdd(&g_sstat[SSTAT_BURSTS_QUIET], 1ull); }
    }
#endif
}
// a burst of `sweeps` sweeps (1..16) is over
__device__ __forceinline__ void diag_burst(int sweeps) {
#ifdef UFM_SWEEPSTAT
    if ((threadIdx.x & 63) == 0) atomicAdd(&g_sstat[SSTAT_BURST_HIST + min(sweeps, 16) - 1], 1ull);
#endif
}

// What the timing build carries through a launch of k_relax and through each of its tile visits: an empty struct in every other build.
struct DiagVisit {
#ifdef UFM_TIMING
    unsigned long long tkb, tk0, tk1, tk2;   // workgroup entry; the visit's pop, staged, swept
    int hint, rank, ninf0;                   // the tile's P.hint and P.rank, its +inf elements as staged
    bool wtrace_on;                          // this visit is the one g_wtrace records
#endif
    __device__ __forceinline__ void launch_begin() {
#ifdef UFM_TIMING
        tkb = wall_clock64();
#endif
    }
    // the workgroup leaves (`rec`: a lowering launch, thread 0)
    __device__ __forceinline__ void launch_end(bool rec, int k) {
#ifdef UFM_TIMING
        if (rec) trace_rec(k, 1, tkb, wall_clock64(), 0);
#endif
    }
    // a tile has been popped; resident kernel (`own0`: its thread 0, gt_own its tile): the per-tile records and the visit's entry in g_vis
    __device__ __forceinline__ void begin(bool own0, int gt_own) {
#ifdef UFM_TIMING
        tk0 = wall_clock64();
        if (own0 && gt_own >= 0 && gt_own < TILE_DIAG_MAX) {
            const unsigned int now = (unsigned int)(tk0 - g_tile_t0);
            atomicMin(&g_tile[TILE_FIRST][gt_own], now);
            const unsigned int pushed = atomicExch(&g_tile[TILE_PUSHED][gt_own], 0xFFFFFFFFu);
            if (pushed != 0xFFFFFFFFu && now > pushed) atomicAdd(&g_tile[TILE_WAIT][gt_own], now - pushed);
            atomicAdd(&g_tile[TILE_VISITS][gt_own], 1u);
            const unsigned long long p64 = atomicExch(&g_push64[gt_own], ~0ull);
            const unsigned int vi = atomicAdd(&g_nvis, 1u);
            s_diag_vi = vi;
            if (vi < VIS_DIAG_MAX) { g_vis[vi][0] = gt_own; g_vis[vi][1] = now; g_vis[vi][2] = 0u; g_vis[vi][3] = (unsigned int)(p64 >> 32); g_vis[vi][4] = (unsigned int)p64; }
        }
#endif
    }
    // the tile is in LDS (all threads call: a barrier); g = what this thread staged, if it staged an element of the tile (`mine`)
    __device__ __forceinline__ void staged(const int *hints, const int *ranks, int gt, bool mine, float g) {
#ifdef UFM_TIMING
        tk1 = wall_clock64();
        hint = hints[gt];
        rank = ranks[gt];
        ninf0 = __syncthreads_count(mine && g == INFINITY);
#endif
    }
    // the sweeps begin; first_long = the first long-list visit of workgroup 0 in lowering launch k of the chain (the wave timeline records one of them)
    __device__ __forceinline__ void sweeps_begin(bool first_long, int k) {
#ifdef UFM_TIMING
        wtrace_on = first_long && k == UFM_TRACE_K0;
#endif
    }
    // one record of the wave timeline (WREC_*)
    __device__ __forceinline__ void wave_rec(int type, int val) const {
#ifdef UFM_TIMING
        const int tid = threadIdx.x, w = tid >> 6;
        if (wtrace_on && (tid & 63) == 0) {
            const unsigned int i_ = g_nw[w]++;
            if (i_ < 256) { g_wtrace[(w * 256 + i_) * 2] = ((unsigned long long)type << 32) | (unsigned int)val; g_wtrace[(w * 256 + i_) * 2 + 1] = wall_clock64(); }
        }
#endif
    }
    // the sweeps are over
    __device__ __forceinline__ void swept() {
#ifdef UFM_TIMING
        tk2 = wall_clock64();
#endif
    }
    // the visit is over (all threads call: a barrier in a lowering kernel).  own / early: the kernel's form; misc = s_misc, qw = s_qw of k_relax;
    // g = this thread's element as the visit leaves it (`mine`, as for staged())
    __device__ __forceinline__ void end(bool lower, bool own, bool early, int k, int gt, int TY, bool conv, const int *misc, const int *qw, bool mine, float g) const {
#ifdef UFM_TIMING
        if (lower) {
            const int ninf1 = __syncthreads_count(mine && g == INFINITY);
            if (threadIdx.x == 0) {
                const unsigned long long tk3 = wall_clock64();
                if (own && gt < TILE_DIAG_MAX && (!early || (qw[1] & DIAG_QW_CHANGED))) g_tile[TILE_LAST_CHANGE][gt] = (unsigned int)(tk3 - g_tile_t0);
                if (own && s_diag_vi < VIS_DIAG_MAX) g_vis[s_diag_vi][2] = (unsigned int)(tk3 - g_tile_t0);
                if (own && gt / TY < 2 && gt % TY < 2) plog((unsigned int)gt, PLOG_VISIT_END, (conv ? 1u : 0u) | ((unsigned int)misc[3] << 8) | ((unsigned int)blockIdx.x << 20));
                if (early) atomicAdd(&g_tdiag[TDIAG_REFRESHES], (unsigned long long)(qw[1] & 0xFFFF));
                atomicAdd(&g_tdiag[TDIAG_STAGE], tk1 - tk0); atomicAdd(&g_tdiag[TDIAG_SWEEP], tk2 - tk1); atomicAdd(&g_tdiag[TDIAG_WRITEBACK], tk3 - tk2);
                atomicAdd(&g_tdiag[TDIAG_VISITS], 1ull);
                const unsigned long long bin = (tk3 - tk0) / 200;
                atomicAdd(&g_tdiag[TDIAG_TIME_HIST + (bin < 31 ? bin : 31)], 1ull);
                atomicAdd(&g_tdiag[TDIAG_SWEEP_HIST + (misc[3] < 23 ? misc[3] : 23)], 1ull);
                trace_rec(k, 0, tk0, tk3, (long long)(misc[3] & 255) | ((long long)min(misc[1], 255) << 8) | ((long long)min(hint, 255) << 16) | ((long long)ninf0 << 24) | ((long long)ninf1 << 40) | ((long long)rank << 52));
            }
        }
#endif
    }
};
