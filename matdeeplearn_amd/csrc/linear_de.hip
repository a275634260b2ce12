// linear_de.hip — the distance gradient of a dense layer that reads the Gaussian expansion: forces for MEGNet and MPNN.
// No reference counterpart: matdeeplearn/models/megnet.py:222-247 and mpnn.py:83-88 feed their first edge layer constant edge
// features; upstream autograd would form this through an [E, G] input gradient (dx = gp W, then the expansion's backward).
//
// Layer  y = act(W r(d) + b),  r_k(d) = exp(coeff (d - mu_k)^2),  W [M, G].  With gp = dL/d(pre-activation):
//     u_e[k] = sum_c gp[e, c] W[c, k]                                   (the layer's input gradient, kept in registers)
//     dd[e] (+)= scale * sum_k u_e[k] * 2 coeff (d_e - mu_k) exp(coeff (d_e - mu_k)^2)
// gp = g (the chain behind the layer handed the activation derivative down) or g * (act_y > 0) (ReLU mask from the layer's
// output, applied while the row is staged).  The exponential is recomputed from d: neither the expansion nor any [E, G] tensor
// is read or written.  Compulsory traffic per edge: M s (+ M s with the mask) + 8 bytes.
//
// Lane = EDGE, as in cfconv_de.hip: the product is the transposed layer D[k][edge] = W^T[k][c] . gp^T[c][edge], so a lane's
// B fragment is 16 consecutive bytes of ITS edge's gradient row, read straight from global memory, and the accumulator holds
// the edge's u[k] in registers (the lanes l and l + 32 share an edge and hold disjoint k).  W^T, zero-padded to [64][MP], is
// staged in LDS once per workgroup.  A wave owns a tile of 32 consecutive edges; the epilogue multiplies by r'_k(d_e), sums
// inside the lane and across the pair with one shuffle, and the lower lane of the pair writes or adds dd[e].  Purely per edge:
// no CSR, no order, no atomics — the same bits on every run.  Rows past E are never read or written (the last tile's spare
// lanes re-read row E - 1 and discard the result).
// bf16: v_mfma_f32_32x32x16_bf16 (fp32 accumulation, hardware exp2 in the epilogue as the forward expansion uses for bf16).
// fp32: exact v_mfma_f32_32x32x2_f32 and the precise expf (parity mode; bf16x3 models keep fp32 tensors and take this path).
// Rows are read as 16-byte chunks where base and leading dimension allow, as dwords for even widths like 100 / 150, element
// by element otherwise; a chunk that straddles column M is read element by element under a guard.
#include <algorithm>

#include "mdl_common.h"

namespace mdl {
namespace lde {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int NW = 4, NT = NW * WAVE, TE = 32, GP = 64, UN = 4;
constexpr int MAX_M = 256, MAX_G = 64;

struct Params {
    const void* g;           // [E, M] leading dimension ld_g
    const void* y;           // [E, M] leading dimension ld_y: the layer's ReLU output, or nullptr
    const void* w;           // [M, G]
    const float* d;          // [E]
    const float* offsets;    // [G]
    float* dd;               // [E]
    int64_t ld_g, ld_y, E;
    float coeff, scale;
    int M, G, accumulate;
};

template <typename T> struct Tr;
template <> struct Tr<bf16_t> {
    static constexpr int CH = 8;                             // elements of a 16-byte chunk = a lane's share of one k-step
    typedef bf16x8 frag;
};
template <> struct Tr<float> {
    static constexpr int CH = 4;
    typedef f32x4 frag;
};

// padded width (whole groups of UN k-steps) and the row stride of W^T in LDS (elements; 16 bytes of padding per row)
template <typename T> __host__ __device__ inline int padded_m(int M) {
    constexpr int GRP = UN * 2 * Tr<T>::CH;
    return (M + GRP - 1) / GRP * GRP;
}
template <typename T> __host__ __device__ inline int lds_bytes(int M) {
    return GP * (int)sizeof(float) + GP * (padded_m<T>(M) + Tr<T>::CH) * (int)sizeof(T);
}

// 16 bytes of a row from column c on; AL = what base and leading dimension guarantee (bytes).  Columns >= M read as zero.
template <typename T, int AL>
__device__ __forceinline__ typename Tr<T>::frag load_chunk(const T* row, int c, int M) {
    constexpr int CH = Tr<T>::CH;
    typename Tr<T>::frag v;
#pragma unroll
    for (int j = 0; j < CH; ++j) v[j] = 0;
    if (c + CH <= M) {
        if constexpr (AL == 16) {
            v = *reinterpret_cast<const typename Tr<T>::frag*>(row + c);
        } else if constexpr (AL == 4 && sizeof(T) == 2) {
            const unsigned* q = reinterpret_cast<const unsigned*>(row + c);
            v = __builtin_bit_cast(bf16x8, u32x4{q[0], q[1], q[2], q[3]});
        } else {
#pragma unroll
            for (int j = 0; j < CH; ++j) v[j] = row[c + j];
        }
    } else if (c < M) {
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (c + j < M) v[j] = row[c + j];
    }
    return v;
}

// gp = g where the ReLU output is positive (signed compare of the bf16 pattern: +0, -0 and negatives are not)
__device__ __forceinline__ bf16x8 relu_mask(bf16x8 g, bf16x8 y) { return g & (y > (short)0); }
__device__ __forceinline__ f32x4 relu_mask(f32x4 g, f32x4 y) {
    return f32x4{y[0] > 0.0f ? g[0] : 0.0f, y[1] > 0.0f ? g[1] : 0.0f, y[2] > 0.0f ? g[2] : 0.0f, y[3] > 0.0f ? g[3] : 0.0f};
}

__device__ __forceinline__ f32x16 mma(bf16x8 a, bf16x8 b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}
// one 16-byte chunk of fp32 = four k-steps of the 32x32x2 product; step j contracts the columns c0 + j and c0 + 4 + j
__device__ __forceinline__ f32x16 mma(f32x4 a, f32x4 b, f32x16 acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    return acc;
}

template <typename T, int AL>
__global__ __launch_bounds__(NT) void linear_de_kernel(Params p) {
    constexpr int CH = Tr<T>::CH, KS = 2 * CH;               // columns of one k-step group of the wave (both lane halves)
    constexpr bool FAST = sizeof(T) == 2;
    typedef typename Tr<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = p.M, G = p.G, MP = padded_m<T>(M), LA = MP + CH;
    float* const offl = reinterpret_cast<float*>(smem);      // [64] centres (entries >= G repeat the last one)
    T* const wt = reinterpret_cast<T*>(smem + GP * sizeof(float));   // W^T [64][LA]; rows >= G and columns >= M zero

    {
        const T* const w = static_cast<const T*>(p.w);
        for (int q = tid; q < GP; q += NT) offl[q] = p.offsets[min(q, G - 1)];
        for (int q = tid; q < GP * MP; q += NT) {
            const int c = q >> 6, k = q & 63;
            wt[k * LA + c] = (k < G && c < M) ? w[c * G + k] : (T)0;
        }
    }
    __syncthreads();

    const int64_t E = p.E, n_tiles = (E + TE - 1) / TE;
    const T* const gg = static_cast<const T*>(p.g);
    const T* const yy = static_cast<const T*>(p.y);
    const bool two = G > 32;                                 // Gaussians 32 .. 63 exist
    const float c2 = FAST ? p.coeff * LOG2E_F : p.coeff;
    const float post = p.scale * 2.0f * p.coeff;

    for (int64_t tile = (int64_t)blockIdx.x * NW + wv; tile < n_tiles; tile += (int64_t)gridDim.x * NW) {
        const int64_t e = tile * TE + i;
        const bool valid = e < E;
        const int64_t ec = valid ? e : E - 1;
        const T* const grow = gg + ec * p.ld_g;
        const T* const yrow = yy ? yy + ec * p.ld_y : nullptr;
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;

        for (int c0 = 0; c0 < M; c0 += UN * KS) {
            frag b[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) b[u] = load_chunk<T, AL>(grow, c0 + u * KS + CH * h, M);
            if (yrow) {
#pragma unroll
                for (int u = 0; u < UN; ++u) b[u] = relu_mask(b[u], load_chunk<T, AL>(yrow, c0 + u * KS + CH * h, M));
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int c = c0 + u * KS;
                if (c < M) {                                 // (uniform; the padded columns of W^T and of the row are zero)
                    acc0 = mma(*reinterpret_cast<const frag*>(wt + i * LA + c + CH * h), b[u], acc0);
                    if (two) acc1 = mma(*reinterpret_cast<const frag*>(wt + (32 + i) * LA + c + CH * h), b[u], acc1);
                }
            }
        }

        // register r of block gt, lane half h = Gaussian 32 gt + d_row(r, h)
        const float dn = p.d[ec];
        float s = 0.0f;
#pragma unroll
        for (int gt = 0; gt < 2; ++gt) {
            if (gt == 1 && !two) break;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = 32 * gt + d_row(r, h);
                const float diff = dn - offl[k];
                const float q = c2 * (diff * diff);
                const float t = diff * (FAST ? __builtin_amdgcn_exp2f(q) : expf(q));
                const float uk = gt == 0 ? acc0[r] : acc1[r];
                s = fmaf(k < G ? uk : 0.0f, t, s);
            }
        }
        s += __shfl_xor(s, 32);
        if (h == 0 && valid) {
            const float v = post * s;
            p.dd[e] = p.accumulate ? p.dd[e] + v : v;
        }
    }
}

template <typename T, int AL>
static int launch(const Params& p, hipStream_t st, const char* name) {
    auto kf = linear_de_kernel<T, AL>;
    const int lds = lds_bytes<T>(p.M);
    hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(kf), lds);
    if (e != hipSuccess) { set_error("%s: LDS attribute (%d B): %s", name, lds, hipGetErrorString(e)); return MDL_E_LAUNCH; }
    // (a workgroup stages W^T once and then walks tiles: enough workgroups to fill the chip a few times over, no more)
    const int64_t grid = std::min<int64_t>(2048, std::max<int64_t>(1, cdiv(cdiv(p.E, TE), NW)));
    hipLaunchKernelGGL(kf, dim3((unsigned)grid), dim3(NT), lds, st, p);
    return check_launch(name);
}

// what base pointer and leading dimension guarantee for every row start (bytes)
static int row_align(const void* base, int64_t ld, int esize) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(base) | (uintptr_t)(ld * esize);
    return a % 16 == 0 ? 16 : (a % 4 == 0 ? 4 : esize);
}

}  // namespace lde
}  // namespace mdl

using namespace mdl;

extern "C" int mdl_linear_rbf_dist_grad_supported(int M, int G, int dtype) {
    return (dtype == MDL_F32 || dtype == MDL_BF16) && M >= 1 && M <= lde::MAX_M && G >= 1 && G <= lde::MAX_G;
}

extern "C" int mdl_linear_rbf_dist_grad(const void* g, int64_t ld_g, const void* act_y, int64_t ld_y, const void* w, int dtype,
                                        const float* d, const float* offsets, float coeff, float scale, float* dd, int accumulate,
                                        int64_t E, int M, int G, mdlStream_t stream) {
    const char* name = "mdl_linear_rbf_dist_grad";
    MDL_REQUIRE(mdl_linear_rbf_dist_grad_supported(M, G, dtype), MDL_E_UNSUPP, "%s: fp32 or bf16, M in [1, %d], G in [1, %d] only (M = %d, G = %d, dtype %d)",
                name, lde::MAX_M, lde::MAX_G, M, G, dtype);
    MDL_REQUIRE(E >= 0 && E < (1ll << 40), MDL_E_ARG, "%s: bad E=%lld", name, (long long)E);
    MDL_REQUIRE(ld_g >= M && ld_g < (1ll << 20), MDL_E_ARG, "%s: ld_g %lld out of range (M = %d)", name, (long long)ld_g, M);
    MDL_REQUIRE(!act_y || (ld_y >= M && ld_y < (1ll << 20)), MDL_E_ARG, "%s: ld_y %lld out of range (M = %d)", name, (long long)ld_y, M);
    if (E == 0) return MDL_OK;
    MDL_REQUIRE(g && w && d && offsets && dd, MDL_E_ARG, "%s: null pointer", name);
    const int es = dtype == MDL_BF16 ? 2 : 4;
    MDL_REQUIRE(((uintptr_t)g % es) == 0 && ((uintptr_t)w % es) == 0 && (!act_y || ((uintptr_t)act_y % es) == 0), MDL_E_ARG,
                "%s: misaligned tensor", name);
    lde::Params p{g, act_y, w, d, offsets, dd, ld_g, act_y ? ld_y : 0, E, coeff, scale, M, G, accumulate ? 1 : 0};
    int al = lde::row_align(g, ld_g, es);
    if (act_y) al = std::min(al, lde::row_align(act_y, ld_y, es));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MDL_BF16) {
        if (al == 16) return lde::launch<bf16_t, 16>(p, st, name);
        if (al == 4) return lde::launch<bf16_t, 4>(p, st, name);
        return lde::launch<bf16_t, 2>(p, st, name);
    }
    if (al == 16) return lde::launch<float, 16>(p, st, name);
    return lde::launch<float, 4>(p, st, name);
}
