// ufm_cspace_graded.h -- C-space inflation by a graded footprint on the device (ufm_set_cspace_graded): grey-scale dilation, a max of
// raw - drop, where ufm_cspace.h's kernel takes a plain max (ufm_cspace_graded_rect.h has the definition, the grouping into levels and
// why it is exact)
// (a piece of ufm_engine.hip, the engine's one translation unit: included there behind ufm_cspace.h, inside its anonymous namespace)
#pragma once

#include "ufm_cspace.h"
#include "ufm_cspace_graded_rect.h"

// The flat kernel's tile, threads, LDS row pitch and staging (the notes at the top of ufm_cspace.h hold here word for word: the support
// of a graded footprint is staged exactly as a flat mask of the same cells would be; zero outside the map is still the identity, since
// max(0 - d, 0) = 0).  What differs is the loop behind the barrier: once per level, the flat loop over that level's rows and set bits
// into a maximum of its own, then one saturating subtract of the level's drop and one max into the result -- per level and cell, not
// per footprint cell.  Every LDS byte of the support is read once, as by the flat kernel over the same support.
struct CspaceGradedJob {
    const uint8_t *raw;      // [L][W]
    uint8_t *out;
    int L, W;
    int x0, y0, h, w;
    int pitch;
    int mh, mw, ar, ac;
    int nl;                                           // levels, 2 .. 16 (one level is a flat footprint: k_cspace_dilate)
    int drop[CSPACE_MAX_LEVELS];                      // wave-uniform like the rows: kernel arguments, read through scalar loads
    uint32_t rows[CSPACE_MAX_LEVELS][CSPACE_MAX];     // the loops over levels, rows and set bits are scalar-controlled
};
static_assert(sizeof(CspaceGradedJob) <= 4096, "the job travels as kernel arguments");

__global__ __launch_bounds__(256) void k_cspace_dilate_graded(CspaceGradedJob J) {
    __shared__ uint32_t lds[CS_ROWS * CS_PITCH / 4];
    const int r0 = J.x0 + (int)blockIdx.y * CS_TR, c0 = J.y0 + (int)blockIdx.x * CS_TC;   // the tile's first output cell
    const int vr = min(CS_TR, J.x0 + J.h - r0), vc = min(CS_TC, J.y0 + J.w - c0);         // outputs of the tile inside the rectangle
    const int sr0 = r0 - J.ar;                  // output (i, j) reads raw rows i - ar .. i + mh-1 - ar, columns j - ac .. j + mw-1 - ac
    const int sc = c0 - J.ac;
    const int sc0 = sc & ~3;                    // staged from the dword boundary at or below (two's complement: below 0 as well)
    const int off = sc - sc0;
    const int nrows = vr + J.mh - 1;            // <= CS_ROWS
    const int ndw = (off + vc + J.mw - 1 + 3) >> 2;      // <= 25 dwords of a 48-dword row
    // dword loads where every staged dword is aligned in HBM and lies wholly inside or wholly outside a raster row
    const bool dw_ok = (J.W & 3) == 0 && (reinterpret_cast<uintptr_t>(J.raw) & 3) == 0;
    for (int i = threadIdx.x; i < nrows * ndw; i += 256) {
        const int lr = i / ndw, d = i - lr * ndw;
        const int gr = sr0 + lr, gc = sc0 + 4 * d;
        uint32_t v = 0;
        if (gr >= 0 && gr < J.L) {
            const uint8_t *row = J.raw + (size_t)gr * J.W;
            if (dw_ok) {
                if (gc >= 0 && gc < J.W) v = *reinterpret_cast<const uint32_t *>(row + gc);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (gc + k >= 0 && gc + k < J.W) v |= (uint32_t)row[gc + k] << (8 * k);
            }
        }
        lds[lr * (CS_PITCH / 4) + d] = v;
    }
    __syncthreads();
    const int lr = threadIdx.x >> 4, lc = 4 * (threadIdx.x & 15);
    const int nv = min(4, vc - lc);             // cells of this thread's run inside the rectangle
    if (lr >= vr || nv <= 0) return;
    const uint8_t *lb = reinterpret_cast<const uint8_t *>(lds) + lr * CS_PITCH + lc + off;
    int M0 = 0, M1 = 0, M2 = 0, M3 = 0;
    for (int l = 0; l < J.nl; ++l) {
        int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
        for (int a = 0; a < J.mh; ++a) {
            const uint8_t *q = lb + a * CS_PITCH;
            for (uint32_t bits = J.rows[l][a]; bits; bits &= bits - 1) {
                const int b = __builtin_ctz(bits);
                m0 = max(m0, (int)q[b]); m1 = max(m1, (int)q[b + 1]);
                m2 = max(m2, (int)q[b + 2]); m3 = max(m3, (int)q[b + 3]);
            }
        }
        const int d = J.drop[l];                // (M >= 0 is the saturation: a difference below zero loses the max)
        M0 = max(M0, m0 - d); M1 = max(M1, m1 - d);
        M2 = max(M2, m2 - d); M3 = max(M3, m3 - d);
    }
    uint8_t *o = J.out + (size_t)(r0 + lr - J.x0) * J.pitch + (c0 + lc - J.y0);
    if (nv == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t *>(o) = (uint32_t)M0 | ((uint32_t)M1 << 8) | ((uint32_t)M2 << 16) | ((uint32_t)M3 << 24);
    } else {
        o[0] = (uint8_t)M0;
        if (nv > 1) o[1] = (uint8_t)M1;
        if (nv > 2) o[2] = (uint8_t)M2;
        if (nv > 3) o[3] = (uint8_t)M3;
    }
}
