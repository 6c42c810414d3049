// ufm_cspace.h -- C-space inflation on the device (ufm_set_cspace): the engine keeps the caller's raw raster and plans on its dilation
// by the vehicle's footprint (ufm_cspace_rect.h has the definition and the host-side arithmetic)
// (a piece of ufm_engine.hip, the engine's one translation unit: included there, inside its anonymous namespace)
#pragma once

#include "ufm_cspace_rect.h"

// An output tile of 16 rows x 64 columns per workgroup of 256 threads: thread t makes the 4 adjacent cells 4 * (t & 15) .. + 3 of row
// t >> 4.  The raw tile and its apron -- up to 30 rows, and 30 columns plus the 0..3 that align its first column to a dword -- is staged
// once into LDS as bytes; cells outside the map are staged as 0, the identity of the max over uint8 ("ignored", include/ufm.h).
// LDS row pitch 192 B = 48 dwords: a byte read is banked like ds_read_b32, (a / 4) mod 32 within each half of the wave, and a half is two
// tile rows of 16 threads whose dwords are adjacent -- 48 mod 32 = 16 puts the second row on the other 16 banks: no conflict.
constexpr int CS_TR = 16, CS_TC = 64;
constexpr int CS_ROWS = CS_TR + CSPACE_MAX - 1;           // 46
constexpr int CS_PITCH = 192;
static_assert(CS_PITCH >= 3 + CS_TC + CSPACE_MAX - 1 + 3 && CS_PITCH % 4 == 0 && (CS_PITCH / 4) % 32 == 16, "LDS row holds tile + apron, rows alternate bank halves");

// One dilation: the rectangle (x0, y0, h, w) of the planning raster of a map, from that map's raw raster, written to
// out[(i - x0) * pitch + (j - y0)] -- the whole map into P.cost (pitch W), or a grown patch rectangle into the engine's scratch patch.
struct CspaceJob {
    const uint8_t *raw;      // [L][W]
    uint8_t *out;
    int L, W;
    int x0, y0, h, w;
    int pitch;
    int mh, mw, ar, ac;
    uint32_t rows[CSPACE_MAX];   // the mask: wave-uniform, read through scalar loads; the loop over its set bits is scalar-controlled
};

__global__ __launch_bounds__(256) void k_cspace_dilate(CspaceJob J) {
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
    uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    for (int a = 0; a < J.mh; ++a) {
        const uint8_t *q = lb + a * CS_PITCH;
        for (uint32_t bits = J.rows[a]; bits; bits &= bits - 1) {
            const int b = __builtin_ctz(bits);
            m0 = max(m0, (uint32_t)q[b]); m1 = max(m1, (uint32_t)q[b + 1]);
            m2 = max(m2, (uint32_t)q[b + 2]); m3 = max(m3, (uint32_t)q[b + 3]);
        }
    }
    uint8_t *o = J.out + (size_t)(r0 + lr - J.x0) * J.pitch + (c0 + lc - J.y0);
    if (nv == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t *>(o) = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
    } else {
        o[0] = (uint8_t)m0;
        if (nv > 1) o[1] = (uint8_t)m1;
        if (nv > 2) o[2] = (uint8_t)m2;
        if (nv > 3) o[3] = (uint8_t)m3;
    }
}

// a raw patch [h][w] into the raw raster of a map, first element at cell (x, y): a plain copy, in front of the dilation on the same stream
__global__ void k_raw_store(uint8_t *raw, int W, const uint8_t *patch, int x, int y, int w, int h) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= w * h) return;
    const int i = e / w, j = e - i * w;
    raw[(size_t)(x + i) * W + (y + j)] = patch[e];
}
