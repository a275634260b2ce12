// struct_reduce.h — the workgroup-per-structure reduction of the integrators (csrc/relax.hip, csrc/md.hip): one workgroup of 256
// lanes owns one structure; its sums are formed by a wave64 shuffle tree, then the four waves through LDS in wave order — no
// atomics, the same bits on every run and in every batch.
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

}  // namespace mdl
