// ufm_diag_host.h -- the host readers of the diagnostic builds' globals (csrc/ufm_diag.h says what every index means): exported by
// libufm_timing.so and libufm_sstat.so only, called by the tools under tools/ and by tests/diag_probe.py
// (a piece of ufm_engine.hip: included there behind the anonymous namespace -- these are C symbols)
#pragma once

extern "C" {

#ifdef UFM_SWEEPSTAT
int ufm_debug_sstat(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sstat), sizeof(unsigned long long) * 32) != hipSuccess) return UFM_ERR_HIP_BASE;
    if (reset) { unsigned long long z[32] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_sstat), z, sizeof(z)) != hipSuccess) return UFM_ERR_HIP_BASE; }
    return UFM_OK;
}
#endif
#ifdef UFM_TIMING
int ufm_debug_trace(unsigned long long *out, int cap) {     // returns the number of records copied (4 words each)
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_ntrace), sizeof(n)) != hipSuccess) return UFM_ERR_HIP_BASE;
    if ((int)n > cap) n = cap;
    if (n > 16384) n = 16384;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), sizeof(unsigned long long) * 4 * n) != hipSuccess) return UFM_ERR_HIP_BASE;
    const unsigned int z = 0;
    hipMemcpyToSymbol(HIP_SYMBOL(g_ntrace), &z, sizeof(z));
    return (int)n;
}
int ufm_debug_visits(unsigned int *out, int cap) {   // out[cap][5]; returns the number of visits recorded
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_nvis), sizeof(n)) != hipSuccess) return UFM_ERR_HIP_BASE;
    if ((int)n > cap) n = cap;
    if (n > VIS_DIAG_MAX) n = VIS_DIAG_MAX;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vis), sizeof(unsigned int) * 5 * n) != hipSuccess) return UFM_ERR_HIP_BASE;
    return (int)n;
}
int ufm_debug_plog(unsigned int *out, int cap) {     // out[cap][4]
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_nplog), sizeof(n)) != hipSuccess) return UFM_ERR_HIP_BASE;
    if ((int)n > cap) n = cap;
    if (n > PLOG_MAX) n = PLOG_MAX;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_plog), sizeof(unsigned int) * 4 * n) != hipSuccess) return UFM_ERR_HIP_BASE;
    return (int)n;
}
int ufm_debug_sdiag(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sdiag), sizeof(unsigned long long) * 16) != hipSuccess) return UFM_ERR_HIP_BASE;
    if (reset) { unsigned long long z[16] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_sdiag), z, sizeof(z)) != hipSuccess) return UFM_ERR_HIP_BASE; }
    return UFM_OK;
}
int ufm_debug_tiles(unsigned int *out, int n) {     // out[5][n]
    if (n > TILE_DIAG_MAX) n = TILE_DIAG_MAX;
    for (int r = 0; r < 5; ++r)
        if (hipMemcpyFromSymbol(out + (size_t)r * n, HIP_SYMBOL(g_tile), sizeof(unsigned int) * n, sizeof(unsigned int) * (size_t)r * TILE_DIAG_MAX) != hipSuccess) return UFM_ERR_HIP_BASE;
    return n;
}
int ufm_debug_wtrace(unsigned long long *out, unsigned int *counts) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wtrace), sizeof(unsigned long long) * 16 * 256 * 2) != hipSuccess) return UFM_ERR_HIP_BASE;
    if (hipMemcpyFromSymbol(counts, HIP_SYMBOL(g_nw), sizeof(unsigned int) * 16) != hipSuccess) return UFM_ERR_HIP_BASE;
    unsigned int z[16] = {};
    hipMemcpyToSymbol(HIP_SYMBOL(g_nw), z, sizeof(z));
    return UFM_OK;
}
int ufm_debug_tdiag(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tdiag), sizeof(unsigned long long) * 64) != hipSuccess) return UFM_ERR_HIP_BASE;
    if (reset) { unsigned long long z[64] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_tdiag), z, sizeof(z)) != hipSuccess) return UFM_ERR_HIP_BASE; }
    return UFM_OK;
}
#endif

}  // extern "C"
