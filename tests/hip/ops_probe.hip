// ops_probe.hip -- TEST INFRASTRUCTURE ONLY: the device functions of csrc/ufm_ops.h, one by one, on inputs a test constructs
// (libufm_ops_probe.so; loaded by tests/test_gpu_operators.py, its export list held by tests/test_operator_cases.py).
//
// The engine's kernels only ever show these functions through whole fields.  Here each one is called from a kernel that does nothing else:
// the headers are included exactly as ufm_engine.hip includes them (same flags, same anonymous namespace), so what runs is the text the hot
// kernels inline.  Nothing of the product is defined or changed; libufm.so does not know this file.
//
// Every entry point takes host arrays, allocates, launches on the null stream, copies back, frees and returns the HIP error code (0 = ok).
// No state survives a call.  Every kernel checks its index against n; the quad kernels keep whole quads running (a DPP read of a lane that has
// left is undefined) and only guard the loads and stores.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ufm.h"

namespace {

#include "ufm_diag.h"
#include "ufm_defs.h"
#include "ufm_ops.h"

constexpr int PROBE_THREADS = 256;
constexpr int QUADS_PER_BLOCK = PROBE_THREADS / 4;

__global__ __launch_bounds__(PROBE_THREADS) void k_probe_sqrt(const float *x, float *y, long n) {
    const long i = (long)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (i < n) y[i] = sqrt_rn(x[i]);
}

// one triangle per thread.  Field D*: tri_fd three times -- with the constants of TriFD::set (k_finalize_bp's siblings k_check_info and the
// back-pointer code), and with those of TriFD::set2 in either of its two slots (the sweeps); the slot not under test gets the cell's own cost
// as its b.  Shifted Grid: tri_sg, written to all three outputs.
template <int ALGO>
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_tri(const float *g1, const float *g2, const float *c, const float *b, long n,
                                                             float *v_set, float *v_set2v, float *v_set2h, int *dep) {
    const long i = (long)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (i >= n) return;
    const float a1 = g1[i], a2 = g2[i], cc = c[i], bb = b[i];
    if constexpr (ALGO == UFM_ALGO_SG) {
        CellSG k;
        k.set(cc);
        const float v = tri_sg(a1, a2, k);
        v_set[i] = v; v_set2v[i] = v; v_set2h[i] = v;
        dep[i] = dep_sg(a1, a2, k);
    } else {
        const CellFD k = {cc, cc * cc, cc * SQRT2F};
        TriFD t, tv, th, ov, oh;
        t.set(cc, bb);
        TriFD::set2(tv, oh, cc, bb, cc);
        TriFD::set2(ov, th, cc, cc, bb);
        v_set[i] = tri_fd(a1, a2, k, t);
        v_set2v[i] = tri_fd(a1, a2, k, tv);
        v_set2h[i] = tri_fd(a1, a2, k, th);
        dep[i] = dep_fd(a1, a2, k, t);
    }
}

__global__ __launch_bounds__(PROBE_THREADS) void k_probe_qdfm(const float *a, const float *b, const float *th, long n, float *v, int *dep) {
    const long i = (long)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (i >= n) return;
    v[i] = q_dfm(a[i], b[i], th[i]);
    dep[i] = dep_dfm(a[i], b[i], th[i]);
}

// One DPP quad per case, 16 cases per wave.  g9: the case's 3 x 3 elements, row-major, the centre in the middle; costs: node planners the four
// cells around the centre node, [dx][dy] (cell (x - 1 + dx, y - 1 + dy)), MS-DFM the centre cell's cost in [0]; +inf = lethal.  The elements
// are staged in LDS with pitch PITCH (the centre is element (0, 0) of a tile whose halo is the ring around it), the costs come through load_at.
template <int ALGO, int PITCH>
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_quad(const float *g9, const float *costs, long n, float *rhs, float *rhs_w, int *byte, float *via) {
    __shared__ float s_g[QUADS_PER_BLOCK * 3 * PITCH];
    __shared__ float s_c[QUADS_PER_BLOCK * 4];
    const int tid = threadIdx.x, q = tid & 3, lc = tid >> 2;
    const long cs = (long)blockIdx.x * QUADS_PER_BLOCK + lc;
    const bool live = cs < n;
    const long src = live ? cs : n - 1;                  // a quad beyond n re-evaluates the last case and stores nothing
    float *blk = s_g + lc * 3 * PITCH;
    for (int e = q; e < 3 * PITCH; e += 4) {
        const int r = e / PITCH, col = e - r * PITCH;
        blk[e] = (col < 3) ? g9[src * 9 + r * 3 + col] : INFINITY;
    }
    s_c[lc * 4 + q] = costs[src * 4 + q];
    __syncthreads();
    const float *cc = s_c + lc * 4;
    const float *ctr = blk + PITCH + 1;
    QuadConsts<ALGO> C;
    C.load_at([=](int r, int col) { return cc[r * 2 + col]; }, 0, 0, q, PITCH);
    const float r0 = quad_min(eval_quad<ALGO, PITCH>(ctr, q, C));
    const LaneEval le = eval_quad_w<ALGO, PITCH>(ctr, q, C);
    const float nv = quad_min(le.r);
    const int bq = quad_min_int(bp_byte<ALGO>(le, q, C, le.r == nv)), bpb = bp_of_key<ALGO>(bq);      // as k_finalize_bp (tile_bp)
    const float v = quad_min(eval_quad_bp<ALGO, PITCH>(ctr, q, C, bpb));
    if (live && q == 0) { rhs[cs] = r0; rhs_w[cs] = nv; byte[cs] = bpb; via[cs] = v; }
}

// full waves: lanes beyond n take part with +inf / INT_MAX and store nothing
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_quad_min(const float *v, const int *vi, long n, float *out, int *outi) {
    const long i = (long)blockIdx.x * PROBE_THREADS + threadIdx.x;
    const bool live = i < n;
    const float m = quad_min(live ? v[i] : INFINITY);
    const int mi = quad_min_int(live ? vi[i] : INT_MAX);
    if (live) { out[i] = m; outi[i] = mi; }
}

// device copies of a call's arrays: freed when the call returns, whatever it returns
struct ProbeBufs {
    static constexpr int CAP = 12;
    void *ptr[CAP];
    int used = 0;
    hipError_t err = hipSuccess;
    void *in(const void *host, size_t bytes) {
        void *d = out(bytes);
        if (d && err == hipSuccess) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        return d;
    }
    void *out(size_t bytes) {
        if (err != hipSuccess || used == CAP) { if (err == hipSuccess) err = hipErrorInvalidValue; return nullptr; }
        void *d = nullptr;
        err = hipMalloc(&d, bytes ? bytes : 1);
        if (err != hipSuccess) return nullptr;
        ptr[used++] = d;
        return d;
    }
    void back(void *host, const void *dev, size_t bytes) {
        if (err == hipSuccess) err = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
    }
    // after a launch: its launch error, then its execution error
    void ran() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    ~ProbeBufs() { for (int i = 0; i < used; ++i) (void)hipFree(ptr[i]); }
};
unsigned blocks_for(long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }
bool bad_n(long n) { return n <= 0 || n > (1L << 28); }

template <int ALGO, int PITCH>
int run_quad(const float *g9, const float *costs, long n, float *rhs, float *rhs_w, int *byte, float *via) {
    ProbeBufs B;
    const size_t f = (size_t)n * sizeof(float);
    const float *dg = (const float *)B.in(g9, 9 * f), *dc = (const float *)B.in(costs, 4 * f);
    float *d0 = (float *)B.out(f), *d1 = (float *)B.out(f), *d3 = (float *)B.out(f);
    int *d2 = (int *)B.out((size_t)n * sizeof(int));
    if (B.err != hipSuccess) return (int)B.err;
    k_probe_quad<ALGO, PITCH><<<blocks_for(n, QUADS_PER_BLOCK), PROBE_THREADS>>>(dg, dc, n, d0, d1, d2, d3);
    B.ran();
    B.back(rhs, d0, f); B.back(rhs_w, d1, f); B.back(byte, d2, (size_t)n * sizeof(int)); B.back(via, d3, f);
    return (int)B.err;
}
template <int ALGO>
int run_quad_pitch(int pitch, const float *g9, const float *costs, long n, float *rhs, float *rhs_w, int *byte, float *via) {
    if (pitch == 3) return run_quad<ALGO, 3>(g9, costs, n, rhs, rhs_w, byte, via);
    if (pitch == 0) return run_quad<ALGO, GP>(g9, costs, n, rhs, rhs_w, byte, via);
    return (int)hipErrorInvalidValue;
}

}  // namespace

extern "C" {

// y[i] = sqrt_rn(x[i])
int ufm_probe_sqrt(const float *x, float *y, long n) {
    if (bad_n(n)) return (int)hipErrorInvalidValue;
    ProbeBufs B;
    const size_t f = (size_t)n * sizeof(float);
    const float *dx = (const float *)B.in(x, f);
    float *dy = (float *)B.out(f);
    if (B.err != hipSuccess) return (int)B.err;
    k_probe_sqrt<<<blocks_for(n, PROBE_THREADS), PROBE_THREADS>>>(dx, dy, n);
    B.ran();
    B.back(y, dy, f);
    return (int)B.err;
}

// algo: UFM_ALGO_FD or UFM_ALGO_SG (include/ufm.h); c, b: cell costs as floats, +inf = lethal
int ufm_probe_tri(int algo, const float *g1, const float *g2, const float *c, const float *b, long n,
                  float *v_set, float *v_set2v, float *v_set2h, int *dep) {
    if (bad_n(n) || (algo != UFM_ALGO_FD && algo != UFM_ALGO_SG)) return (int)hipErrorInvalidValue;
    ProbeBufs B;
    const size_t f = (size_t)n * sizeof(float);
    const float *d1 = (const float *)B.in(g1, f), *d2 = (const float *)B.in(g2, f), *dc = (const float *)B.in(c, f), *db = (const float *)B.in(b, f);
    float *o0 = (float *)B.out(f), *o1 = (float *)B.out(f), *o2 = (float *)B.out(f);
    int *od = (int *)B.out((size_t)n * sizeof(int));
    if (B.err != hipSuccess) return (int)B.err;
    if (algo == UFM_ALGO_FD) k_probe_tri<UFM_ALGO_FD><<<blocks_for(n, PROBE_THREADS), PROBE_THREADS>>>(d1, d2, dc, db, n, o0, o1, o2, od);
    else k_probe_tri<UFM_ALGO_SG><<<blocks_for(n, PROBE_THREADS), PROBE_THREADS>>>(d1, d2, dc, db, n, o0, o1, o2, od);
    B.ran();
    B.back(v_set, o0, f); B.back(v_set2v, o1, f); B.back(v_set2h, o2, f); B.back(dep, od, (size_t)n * sizeof(int));
    return (int)B.err;
}

int ufm_probe_qdfm(const float *a, const float *b, const float *th, long n, float *v, int *dep) {
    if (bad_n(n)) return (int)hipErrorInvalidValue;
    ProbeBufs B;
    const size_t f = (size_t)n * sizeof(float);
    const float *da = (const float *)B.in(a, f), *db = (const float *)B.in(b, f), *dt = (const float *)B.in(th, f);
    float *ov = (float *)B.out(f);
    int *od = (int *)B.out((size_t)n * sizeof(int));
    if (B.err != hipSuccess) return (int)B.err;
    k_probe_qdfm<<<blocks_for(n, PROBE_THREADS), PROBE_THREADS>>>(da, db, dt, n, ov, od);
    B.ran();
    B.back(v, ov, f); B.back(dep, od, (size_t)n * sizeof(int));
    return (int)B.err;
}

// algo: UFM_ALGO_FD, UFM_ALGO_SG, or 3 (the kernels' one MS-DFM operator, ALGO_DFM1); pitch: 3, or 0 for the kernels' own LDS pitch GP
int ufm_probe_quad(int algo, int pitch, const float *g9, const float *costs, long n, float *rhs, float *rhs_w, int *byte, float *via) {
    if (bad_n(n)) return (int)hipErrorInvalidValue;
    if (algo == UFM_ALGO_FD) return run_quad_pitch<UFM_ALGO_FD>(pitch, g9, costs, n, rhs, rhs_w, byte, via);
    if (algo == UFM_ALGO_SG) return run_quad_pitch<UFM_ALGO_SG>(pitch, g9, costs, n, rhs, rhs_w, byte, via);
    if (algo == ALGO_DFM1) return run_quad_pitch<ALGO_DFM1>(pitch, g9, costs, n, rhs, rhs_w, byte, via);
    return (int)hipErrorInvalidValue;
}

// out[i] = quad_min(v[i]), outi[i] = quad_min_int(vi[i]): every lane its quad's minimum
int ufm_probe_quad_min(const float *v, const int *vi, long n, float *out, int *outi) {
    if (bad_n(n)) return (int)hipErrorInvalidValue;
    ProbeBufs B;
    const size_t f = (size_t)n * sizeof(float), fi = (size_t)n * sizeof(int);
    const float *dv = (const float *)B.in(v, f);
    const int *di = (const int *)B.in(vi, fi);
    float *of = (float *)B.out(f);
    int *oi = (int *)B.out(fi);
    if (B.err != hipSuccess) return (int)B.err;
    k_probe_quad_min<<<blocks_for(n, PROBE_THREADS), PROBE_THREADS>>>(dv, di, n, of, oi);
    B.ran();
    B.back(out, of, f); B.back(outi, oi, fi);
    return (int)B.err;
}

}  // extern "C"
