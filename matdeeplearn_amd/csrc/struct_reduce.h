// struct_reduce.h — the workgroup-per-structure reduction of the integrators (csrc/relax.hip, csrc/md.hip, csrc/neb.hip): one
// workgroup of 256 lanes owns one structure; its sums are formed by a wave64 shuffle tree, then the four waves through LDS in wave
// order — no atomics, the same bits on every run and in every batch.  Also what relax.hip and neb.hip share: the 3x3 adjugate and
// the operands of the band-force launch that mdl_fire_step makes in band mode.
#pragma once
#include "mdl_common.h"

namespace mdl {

constexpr int STRUCT_THREADS = 256;
constexpr int STRUCT_WAVES = STRUCT_THREADS / WAVE;

// v[0 .. NSUM) summed and v[NSUM .. K) maximised over the workgroup; every lane returns with the same totals in v.
// `red` is used once per call site (no barrier behind the read).
template <int K, int NSUM>
__device__ __forceinline__ void block_reduce(double* v, double (*red)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const double o = __shfl_down(v[k], off, WAVE);
            v[k] = k < NSUM ? v[k] + o : (o > v[k] ? o : v[k]);
        }
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = red[0][k];
#pragma unroll
        for (int w = 1; w < STRUCT_WAVES; ++w) t = k < NSUM ? t + red[w][k] : (red[w][k] > t ? red[w][k] : t);
        v[k] = t;
    }
}

// row-major 3x3: the adjugate (inverse times determinant) and the determinant
__device__ __forceinline__ double adjugate3(const double* m, double* adj) {
#pragma clang fp contract(off)
    adj[0] = m[4] * m[8] - m[5] * m[7];
    adj[1] = m[2] * m[7] - m[1] * m[8];
    adj[2] = m[1] * m[5] - m[2] * m[4];
    adj[3] = m[5] * m[6] - m[3] * m[8];
    adj[4] = m[0] * m[8] - m[2] * m[6];
    adj[5] = m[2] * m[3] - m[0] * m[5];
    adj[6] = m[3] * m[7] - m[4] * m[6];
    adj[7] = m[1] * m[6] - m[0] * m[7];
    adj[8] = m[0] * m[4] - m[1] * m[3];
    return m[0] * adj[0] + m[1] * adj[3] + m[2] * adj[6];
}

// the band mode of mdl_fire_step (include/mdl_hip.h): csrc/neb.hip checks these operands and launches the band-force kernel
struct NebArgs {
    const double* pos;
    const float* force;
    const uint8_t* fixed;
    const int64_t *image_ptr, *band_ptr;
    int64_t N, I, B;
    const float* energy;
    const double* cell;
    const int32_t* pbc;
    const double* spring;
    const uint8_t* climb;
    float* band_force;
    double *tangent_force, *seg_len;
    int32_t* climber;
};
int neb_band_force(const char* fn, const NebArgs& a, hipStream_t stream);

}  // namespace mdl
