// ufm_delta.h -- step deltas (ufm_track_changes / ufm_read_changes): which elements differ from what the caller was last told
// (a piece of ufm_engine.hip, the engine's one translation unit: included there, inside its anonymous namespace, behind ufm_host.h)
//
// The baseline is a second copy of a map's field in the field's own tile-major layout (same gstride), plus, for a level-1/2 planner, one
// byte per element: the key info_from_byte() returns (ufm_path.h) -- everything the element's Info pair depends on, so equal keys mean equal
// pairs.  k_delta_scan streams the field and the baseline side by side and compacts the elements that differ into records; it writes
// nothing else.  The baseline advances in k_delta_commit, a scatter over those records that the host launches once it knows that all of
// them fit the caller's buffers: one pass over the field, and a delta that does not fit leaves no trace.
#pragma once

struct DeltaRecords {        // the engine-owned record buffer (one allocation), `cap` records
    unsigned int *count;
    int32_t *xy;             // [cap][2]
    float *g;                // [cap]
    int32_t *info;           // [cap][2]
    uint8_t *key;            // [cap]: the baseline byte the record commits
    unsigned int cap;
};

constexpr int DELTA_WG = 256;                    // 4 waves; a wave takes 256 consecutive elements per pass: one float4 per lane,
constexpr int DELTA_CHUNK = 64 * 4;              // i.e. a whole 16 x 16 tile (a quarter of a 32 x 32 one)
static_assert(TT % DELTA_CHUNK == 0 && T % 4 == 0, "a lane's four elements share a tile row");

// One scan of a map's field against its baseline.  F.G / bp / base_g / base_key: this map's planes; nchunks = NTm * TT / DELTA_CHUNK.
// INFO: the planner keeps Info (level 1/2): the byte planes take part.  Values are compared as bits (+inf equals +inf, no NaN cases).
// Compaction per wave: one ballot per element slot, popcount prefixes, ONE atomicAdd by the wave's first lane if it found anything.
// Records beyond o.cap are counted, not stored.
template <bool INFO>
__global__ __launch_bounds__(DELTA_WG) void k_delta_scan(PathField F, const uint8_t *bp, const float *base_g, const uint8_t *base_key, int nchunks, DeltaRecords o) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * DELTA_WG + threadIdx.x) >> 6, nwaves = (gridDim.x * DELTA_WG) >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c = wave; c < nchunks; c += nwaves) {
        const size_t a = (size_t)c * DELTA_CHUNK + (size_t)lane * 4;
        const uint4 gv = *reinterpret_cast<const uint4 *>(F.G + a);
        const uint4 bv = *reinterpret_cast<const uint4 *>(base_g + a);
        const unsigned int gb[4] = {gv.x, gv.y, gv.z, gv.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
        const int t = (int)(a / TT), w = (int)(a - (size_t)t * TT);
        const int tx = t / F.TY, ty = t - tx * F.TY;
        const int x = tx * T + w / T, y0 = ty * T + w % T;
        unsigned int codes = 0, keys = 0;
        if constexpr (INFO) {
            codes = *reinterpret_cast<const unsigned int *>(bp + a);
            keys = *reinterpret_cast<const unsigned int *>(base_key + a);
        }
        int diff[4], key[4], i0[4], i1[4];
        unsigned long long bal[4];
        int total = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = x < F.EX && y0 + j < F.EY;          // (a tile's padding beyond the field is nobody's element)
            key[j] = 0xFF; i0[j] = -1; i1[j] = -1;
            bool d = in && gb[j] != bb[j];
            if constexpr (INFO) {
                if (in) key[j] = info_from_byte(F, (codes >> (8 * j)) & 0xFF, __uint_as_float(gb[j]), x, y0 + j, i0[j], i1[j]);
                d = d || (in && key[j] != (int)((keys >> (8 * j)) & 0xFF));
            }
            diff[j] = d;
            bal[j] = __ballot(d);
            total += __popcll(bal[j]);
        }
        if (total == 0) continue;                               // (wave-uniform: an unchanged tile costs its loads only)
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(o.count, (unsigned int)total);
        base = __shfl(base, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned int pos = base + (unsigned int)__popcll(bal[j] & below);
            base += (unsigned int)__popcll(bal[j]);
            if (!diff[j] || pos >= o.cap) continue;
            *reinterpret_cast<int2 *>(o.xy + 2 * (size_t)pos) = make_int2(x, y0 + j);
            o.g[pos] = __uint_as_float(gb[j]);
            if constexpr (INFO) {
                *reinterpret_cast<int2 *>(o.info + 2 * (size_t)pos) = make_int2(i0[j], i1[j]);
                o.key[pos] = (uint8_t)key[j];
            }
        }
    }
}
// The baseline takes the n records the caller has just been handed (distinct elements: no two threads write one address).
__global__ void k_delta_commit(DeltaRecords o, unsigned int n, int TY, float *base_g, uint8_t *base_key) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int x = o.xy[2 * (size_t)i], y = o.xy[2 * (size_t)i + 1];
        const size_t a = ((size_t)(x / T) * TY + (y / T)) * TT + (size_t)(x % T) * T + (y % T);
        base_g[a] = o.g[i];
        if (base_key) base_key[a] = o.key[i];
    }
}

// ---- host side ----
// the empty ExpandedMap: every element +inf, no Info (map m, or all maps with m < 0)
int Engine::track_reset(int m) {
    const size_t first = m < 0 ? 0 : (size_t)m * P.gstride, n = m < 0 ? P.gstride * nmaps : P.gstride;
    k_fill<<<1024, 256, 0, stream>>>(trk_g + first, n, INFINITY);
    HIPCHK(hipGetLastError());
    if (trk_key) HIPCHK(hipMemsetAsync(trk_key + first, 0xFF, n, stream));
    return UFM_OK;
}
int Engine::track_alloc() {              // (the field is allocated)
    track_free();
    int rc = trk_g.alloc(P.gstride * nmaps);
    if (rc == UFM_OK && opt_lvl >= 1) rc = trk_key.alloc(P.gstride * nmaps);
    if (rc != UFM_OK) { track_free(); return rc; }
    return track_reset(-1);
}

int engine_track_changes(Engine *e, int enable) {
    if (!e) return UFM_ERR_INVALID;
    HIPCHK(hipSetDevice(e->device));
    if (!enable) { e->track_free(); e->track = false; return UFM_OK; }
    if (e->track) return UFM_OK;
    if (e->allocated) { const int rc = e->track_alloc(); if (rc != UFM_OK) return rc; }   // (otherwise with the field, Engine::alloc)
    e->track = true;
    return UFM_OK;
}

int engine_read_changes(Engine *e, int m, int cap, int32_t *xy, float *g, int32_t *info, int *total) {
    if (!e || !e->track || !e->allocated || m < 0 || m >= e->nmaps || !total || cap < 0 || (cap > 0 && (!xy || !g))) return UFM_ERR_INVALID;
    if (info && e->opt_lvl == 0) return UFM_ERR_INVALID;          // level 0: the map has no Info member
    HIPCHK(hipSetDevice(e->device));
    { int rc = e->flush_deferred(); if (rc != UFM_OK) return rc; }   // (MS-DFM's Info pairs read the raster)
    const bool has_info = e->opt_lvl >= 1;
    const PathField F = path_field(e, m);
    const uint8_t *bp = e->P.bp + (size_t)m * e->P.gstride;
    float *base_g = e->trk_g + (size_t)m * e->P.gstride;
    uint8_t *base_key = has_info ? e->trk_key + (size_t)m * e->P.gstride : nullptr;
    const int nchunks = (int)(e->P.gstride / DELTA_CHUNK);
    const int grid = std::min((nchunks + 3) / 4, 256 * 8);       // 8 workgroups of 4 waves per CU keep the loads in flight
    if (e->profiling) { int rc = e->trk_ev.ensure(); if (rc != UFM_OK) return rc; }
    { int rc = e->track_records(65536); if (rc != UFM_OK) return rc; }   // (a replan's delta is a few thousand records; it grows below when one is larger)
    unsigned int cnt = 0;
    DeltaRecords o{};
    for (int pass = 0; pass < 2; ++pass) {
        uint8_t *q = e->trk_rec;
        const size_t rec_cap = e->trk_cap();
        o.count = reinterpret_cast<unsigned int *>(q);
        o.xy = reinterpret_cast<int32_t *>(q + 256);
        o.g = reinterpret_cast<float *>(q + 256 + rec_cap * 8);
        o.info = reinterpret_cast<int32_t *>(q + 256 + rec_cap * 12);
        o.key = q + 256 + rec_cap * 20;
        o.cap = (unsigned int)rec_cap;
        HIPCHK(hipMemsetAsync(o.count, 0, sizeof(unsigned int), e->stream));
        if (e->profiling) HIPCHK(hipEventRecord(e->trk_ev[0], e->stream));
        if (has_info) k_delta_scan<true><<<grid, DELTA_WG, 0, e->stream>>>(F, bp, base_g, base_key, nchunks, o);
        else k_delta_scan<false><<<grid, DELTA_WG, 0, e->stream>>>(F, bp, base_g, base_key, nchunks, o);
        hipError_t err = hipGetLastError();
        if (err == hipSuccess && e->profiling) err = hipEventRecord(e->trk_ev[1], e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(&cnt, o.count, sizeof(cnt), hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        HIPCHK(err);
        if (e->profiling) HIPCHK(hipEventElapsedTime(&e->trk_scan_ms, e->trk_ev[0], e->trk_ev[1]));
        *total = (int)cnt;
        if (cnt > (unsigned int)cap) return UFM_OK;              // does not fit the caller: nothing delivered, nothing committed
        if (cnt <= o.cap) break;
        // fits the caller, not the engine's buffer (which only ever grows): scan once more into a larger one -- the field has not moved
        { int rc = e->track_records(cnt); if (rc != UFM_OK) return rc; }
    }
    if (cnt == 0) return UFM_OK;
    HIPCHK(hipMemcpyAsync(xy, o.xy, (size_t)cnt * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(g, o.g, (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (info) HIPCHK(hipMemcpyAsync(info, o.info, (size_t)cnt * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    k_delta_commit<<<(unsigned)std::min<size_t>((cnt + 255) / 256, 2048), 256, 0, e->stream>>>(o, cnt, e->P.TY, base_g, base_key);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return UFM_OK;
}
