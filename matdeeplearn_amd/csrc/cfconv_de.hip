// cfconv_de.hip — K4d: the gradients of SchNet's continuous-filter convolution with respect to its two PER-EDGE inputs, the
// Gaussian expansion that feeds the filter network and the cosine cutoff that scales the message.  No reference counterpart:
// matdeeplearn/models/schnet.py:131-145 feeds CFConv constant edge features; upstream autograd would form these through the
// materialised [E, F] filter.  Together with edge_geom.hip this is what turns SchNet into an interatomic potential (forces).
//
// Edge e: j -> i, g = dL/dout, h = lin1(x), c = cutoff factor:
//     a_e  = ssp(W1 r_e + b1)        W_e = W2 a_e + b2         out_i = sum_e h_j * W_e * c_e            (K4, cfconv.hip)
//     q_e  = g_i * h_j               dc_e = sum_f q_e[f] W_e[f]                                          -> dcut [E]
//     da_e = (W2^T (c_e q_e)) * sigmoid(W1 r_e + b1)           dr_e = W1^T da_e                          -> drbf [E, G]  (general)
//     r_e[k] = exp(coeff (dn_e - mu_k)^2):   dd_e += scale * sum_k dr_e[k] * 2 coeff (dn_e - mu_k) r_e[k]               (distance)
// One pass over the edges in CSR order that RECOMPUTES a_e and W_e (as K4 and K4b do: nothing per edge is read back from a forward).
//
// Lane = EDGE through the whole chain, as in the forward kernel: every product is the transposed layer (A = weights, B =
// activations), so the accumulator registers of one product ARE the B operand of the next and no activation passes through
// memory.  A wave owns a tile of 32 consecutive CSR slots; the only per-wave LDS is the tile's rbf rows (B operand of the first
// product, and the r_e[k] of the distance epilogue).  Per tile:
//     D1[unit][edge] = W1 . r^T           -> a (storage-rounded), kept in registers
//     D2[f][edge]    = W2 . a             -> W (storage-rounded), times q: dc (summed in the lane) and c q (registers)
//     D3[unit][edge] = W2^T . (c q)       times sigmoid (from a: 1 - exp(-(a + ln 2))) -> da, in the registers of a
//     D4[k][edge]    = W1^T . da          -> dr, registers [k]; the two lanes that share an edge (lane, lane + 32) hold disjoint k
// Epilogues: dcut and dd are summed inside the lane and across the pair with one shuffle, and the lower lane of the pair writes
// (dd: read-modify-write, the blocks of a model add into one buffer).  No atomics anywhere: the same bits on every run.
//
// bf16 storage: v_mfma_f32_32x32x16_bf16 on the packed weights of mdl_cfconv_pack_weights (rows permuted so that a lane half
// owns 8 + 8 consecutive units per block, W1 pre-scaled by log2 e, biases in the constant-1 slots), a, W, c q and da rounded to
// bf16 exactly where K4 / K4b round them; W2p, and transposed copies of W2p and W1p made once per workgroup, live in LDS, W1p's
// 20 fragments per tile are read from global memory.  G = 50, even F in [64, 158] (mdl_cfconv_supported).
// fp32 storage: exact v_mfma_f32_32x32x2_f32 on the fp32 masters, W1 [F][G] and W2 [F][F] in LDS (read in place for the
// transposed products too: a fragment is one float).  Run-time F in [33, 160] and G in [1, 64] while the weights fit the LDS
// (F = 150, G = 50: 151 KB).
// Four waves per workgroup, one workgroup per CU (allocated for one wave per SIMD: the chain holds a, c q and an accumulator).
#include <algorithm>

#include "mdl_common.h"

namespace mdl {
namespace cfd {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int NW = 4, NT = NW * WAVE, TE = 32;
constexpr int LDS_CAP = 160 * 1024;
constexpr int G16 = 50, KE16 = 64, ES16 = KE16 + 8;         // bf16: Gaussians; K of the first product (G + bias slot, padded); row stride (halfwords)

struct Params {
    const void* rbf;         // [E, G] edge features, CSR order
    const float* cut;        // [E]
    const void* h;           // [N, F] lin1(x)
    const void* g;           // [N, F] gradient w.r.t. the aggregated messages
    const int32_t* rowptr;   // [N + 1] (rowptr[N] = number of edges that exist)
    const int32_t* src;      // [E]
    const int32_t* tgt;      // [E]
    const bf16_t* wpack;     // bf16: W1p | W2p (mdl_cfconv_pack_weights)
    const float* w1;         // fp32: [F, G]
    const float* b1;         // fp32: [F] or nullptr
    const float* w2;         // fp32: [F, F]
    const float* b2;         // fp32: [F] or nullptr
    float* dcut;             // [E] or nullptr
    void* drbf;              // general: [E, G] storage dtype, or nullptr
    const float* dnorm;      // distance: [E]
    const float* offsets;    // distance: [G]
    float* dd;               // distance: [E] fp32, added into, or nullptr
    float coeff2, scale;     // distance: 2 coeff; chain-rule factor of the caller's normalisation
    int N, F, G;
};

// The fp32 chain is fully unrolled (the activations are indexed as registers): without a fence per group of 16 MFMAs the
// scheduler hoists hundreds of weight reads and their addresses in front of the products and spills
#define GROUP_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ int pi32(int r) { return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1); }

// ------------------------------------------------------------------------------------------------
// fp32
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline int f32_ke(int G) { return (G + 1) & ~1; }
__host__ __device__ inline int f32_lds_bytes(int F, int G, int NB) {
    const int S1 = f32_ke(G) + 1, S2 = 32 * NB + 1;
    return 4 * (F * S1 + F * S2 + 2 * 32 * NB + NW * TE * S1);
}

template <int NB>
__global__ __launch_bounds__(NT, 1) void cfconv_de_f32_kernel(Params p) {
    typedef Gate<false> GT;
    constexpr int FP = 32 * NB, S2 = FP + 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F = p.F, G = p.G, KE = f32_ke(G), S1 = KE + 1;
    float* const w1l = reinterpret_cast<float*>(smem);      // [F][S1], columns >= G zero
    float* const w2l = w1l + F * S1;                         // [F][S2], columns >= F zero
    float* const b1l = w2l + F * S2;                         // [FP]
    float* const b2l = b1l + FP;                             // [FP]
    float* const rt = b2l + FP + wv * (TE * S1);             // this wave's rbf tile [32][S1]

    for (int q = tid; q < F * S1; q += NT) {
        const int u = q / S1, k = q - u * S1;
        w1l[q] = k < G ? p.w1[u * G + k] : 0.0f;
    }
    for (int q = tid; q < F * S2; q += NT) {
        const int f = q / S2, k = q - f * S2;
        w2l[q] = k < F ? p.w2[f * F + k] : 0.0f;
    }
    for (int q = tid; q < FP; q += NT) {
        b1l[q] = (q < F && p.b1) ? p.b1[q] : 0.0f;
        b2l[q] = (q < F && p.b2) ? p.b2[q] : 0.0f;
    }
    __syncthreads();

    const int Et = __builtin_amdgcn_readfirstlane(p.rowptr[p.N]);
    const int n_tiles = (Et + TE - 1) / TE;
    const float* const rbf = static_cast<const float*>(p.rbf);
    const float* const hh = static_cast<const float*>(p.h);
    const float* const gg = static_cast<const float*>(p.g);
    const bool chain = p.drbf != nullptr || p.dd != nullptr;

    for (int tile = blockIdx.x * NW + wv; tile < n_tiles; tile += gridDim.x * NW) {
        // (per-tile copies of the lane coordinates: the hundreds of weight addresses that depend on the lane only would
        // otherwise be hoisted out of the tile loop, kept live across it and spilled — cfconv.hip does the same)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int i = lane_t & 31, h = lane_t >> 5;
        const int eb = tile * TE, nv = min(TE, Et - eb);
        const bool valid = i < nv;
        const int ec = min(eb + i, Et - 1);
        const float* const hrow = hh + (int64_t)p.src[ec] * F;
        const float* const grow = gg + (int64_t)p.tgt[ec] * F;
        const float c = valid ? p.cut[ec] : 0.0f;
        wave_lds_fence();                                    // the previous tile's reads of rt are done
        for (int q = lane; q < TE * S1; q += WAVE) {
            const int row = q / S1, k = q - row * S1;
            rt[q] = (row < nv && k < G) ? rbf[(int64_t)(eb + row) * G + k] : 0.0f;
        }
        wave_lds_fence();

        // ---- D1 = W1 . r^T + b1, a = ssp(D1): register r of block b, lane half h = unit 32 b + d_row(r, h)
        f32x16 a[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) a[b][r] = b1l[32 * b + d_row(r, h)];
        for (int k0 = 0; k0 < KE; k0 += 2) {
            const float bfrag = rt[i * S1 + k0 + h];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int u = 32 * b + i;
                const float wv1 = w1l[min(u, F - 1) * S1 + k0 + h];
                a[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(u < F ? wv1 : 0.0f, bfrag, a[b], 0, 0, 0);
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) a[b][r] = GT::softplus_u(a[b][r]) - LN2_F;

        // ---- D2 = W2 . a + b2 (the filter); q = g[tgt] * h[src]; dc = sum q W; cq = c q.  The k-step (b, r) of a product
        // contracts the two units the register pair (lane, lane + 32) holds: 32 b + d_row(r, 0) and 32 b + d_row(r, 1)
        f32x16 cq[NB];
        float dc = 0.0f;
#pragma unroll
        for (int bo = 0; bo < NB; ++bo) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = b2l[32 * bo + d_row(r, h)];
            const int fo = 32 * bo + i;
            const float* const wrow = w2l + min(fo, F - 1) * S2;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                GROUP_FENCE();
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float wv2 = wrow[32 * b + d_row(r, h)];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fo < F ? wv2 : 0.0f, a[b][r], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * bo + d_row(r, h), fc = min(f, F - 1);
                const float qv = f < F ? grow[fc] * hrow[fc] : 0.0f;
                dc = fmaf(qv, acc[r], dc);
                cq[bo][r] = c * qv;
            }
        }
        dc += __shfl_xor(dc, 32);
        if (p.dcut && h == 0 && valid) p.dcut[eb + i] = dc;
        if (!chain) continue;

        // ---- D3 = W2^T . cq; da = D3 * sigmoid(pre) with sigmoid(pre) = 1 - exp(-(a + ln 2)); da replaces a
#pragma unroll
        for (int bo = 0; bo < NB; ++bo) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            const int uo = 32 * bo + i;                      // (< FP <= S2 - 1: inside the row; columns >= F hold zeros)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                GROUP_FENCE();
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int fk = 32 * b + d_row(r, h);
                    const float wv2 = w2l[min(fk, F - 1) * S2 + uo];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fk < F ? wv2 : 0.0f, cq[b][r], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) a[bo][r] = acc[r] * (1.0f - 0.5f * expf(-a[bo][r]));
        }

        // ---- D4 = W1^T . da: register r of block gt, lane half h = Gaussian 32 gt + d_row(r, h)
        f32x16 dr[2];
#pragma unroll
        for (int gt = 0; gt < 2; ++gt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dr[gt][r] = 0.0f;
            if (32 * gt < G) {
                const int go = 32 * gt + i, goc = min(go, G - 1);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    GROUP_FENCE();
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int uk = 32 * b + d_row(r, h);
                        const float wv1 = w1l[min(uk, F - 1) * S1 + goc];
                        dr[gt] = __builtin_amdgcn_mfma_f32_32x32x2f32((uk < F && go < G) ? wv1 : 0.0f, a[b][r], dr[gt], 0, 0, 0);
                    }
                }
            }
        }

        if (p.drbf) {
            float* const out = static_cast<float*>(p.drbf) + (int64_t)(eb + i) * G;
#pragma unroll
            for (int gt = 0; gt < 2; ++gt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * gt + d_row(r, h);
                    if (valid && k < G) out[k] = dr[gt][r];
                }
        } else {
            const float dn = p.dnorm[ec];
            float s = 0.0f;
#pragma unroll
            for (int gt = 0; gt < 2; ++gt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * gt + d_row(r, h), kc = min(k, G - 1);
                    const float t = (dn - p.offsets[kc]) * rt[i * S1 + kc];
                    s = fmaf(k < G ? dr[gt][r] : 0.0f, t, s);
                }
            s += __shfl_xor(s, 32);
            if (h == 0 && valid) p.dd[eb + i] += (p.scale * p.coeff2) * s;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// bf16
// ------------------------------------------------------------------------------------------------
template <int NB> struct Shape16 {
    static constexpr int FP = 32 * NB, LA = FP + 8;          // padded width; row stride of W2p / W2^T / W1^T (halfwords)
    static constexpr int OFF_W2 = 0;                         // W2p  [FP][LA]   verbatim
    static constexpr int OFF_WT = OFF_W2 + FP * LA * 2;      // W2^T [FP][LA]   row rho of a block = unit pi(rho), columns f natural
    static constexpr int OFF_W1T = OFF_WT + FP * LA * 2;     // W1^T [64][LA]   row = Gaussian, columns = units natural
    static constexpr int OFF_RT = OFF_W1T + 64 * LA * 2;     // per wave: rbf tile [32][ES16]
    static constexpr int LDS = OFF_RT + NW * TE * ES16 * 2;
    static_assert(LDS <= LDS_CAP, "LDS budget");
    static_assert(OFF_WT % 16 == 0 && OFF_W1T % 16 == 0 && OFF_RT % 16 == 0 && (LA * 2) % 16 == 0 && (ES16 * 2) % 16 == 0, "alignment");
};

__device__ __forceinline__ bf16x8 ld_frag16(const bf16_t* base, int row, int ld, int k0, int h) {
    return *reinterpret_cast<const bf16x8*>(base + row * ld + k0 + 8 * h);
}
__device__ __forceinline__ float lo16(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float hi16(unsigned v) { return __uint_as_float(v & 0xffff0000u); }

template <int NB>
__global__ __launch_bounds__(NT, 1) void cfconv_de_bf16_kernel(Params p) {
    typedef Gate<true> GT;
    typedef Shape16<NB> S;
    constexpr int FP = S::FP, LA = S::LA;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F = p.F;
    const bf16_t* const w1g = p.wpack;                       // W1p [FP][ES16] in global memory
    const bf16_t* const w2g = p.wpack + FP * ES16;           // W2p [FP][LA]
    bf16_t* const w2l = reinterpret_cast<bf16_t*>(smem + S::OFF_W2);
    bf16_t* const wt = reinterpret_cast<bf16_t*>(smem + S::OFF_WT);
    bf16_t* const w1t = reinterpret_cast<bf16_t*>(smem + S::OFF_W1T);
    bf16_t* const rt = reinterpret_cast<bf16_t*>(smem + S::OFF_RT) + wv * (TE * ES16);

    {
        const u32x4* gsrc = reinterpret_cast<const u32x4*>(w2g);
        u32x4* l = reinterpret_cast<u32x4*>(smem + S::OFF_W2);
        for (int q = tid; q < FP * LA * 2 / 16; q += NT) l[q] = gsrc[q];
        // W2p[prow][pos]: output unit f = pi(prow), input unit pos (slot FP - 1: the bias, not a unit)
        for (int q = tid; q < FP * FP; q += NT) {
            const int R = q / FP, f = q - R * FP;
            const int u = (R & ~31) | pi32(R & 31), prow = (f & ~31) | pi32(f & 31);
            wt[R * LA + f] = u == FP - 1 ? (bf16_t)0 : w2g[prow * LA + u];
        }
        // W1p[prow][k]: unit pi(prow), Gaussian k (slot G: the bias)
        for (int q = tid; q < 64 * FP; q += NT) {
            const int k = q / FP, u = q - k * FP;
            w1t[k * LA + u] = k < G16 ? w1g[((u & ~31) | pi32(u & 31)) * ES16 + k] : (bf16_t)0;
        }
    }
    __syncthreads();

    const int Et = __builtin_amdgcn_readfirstlane(p.rowptr[p.N]);
    const int n_tiles = (Et + TE - 1) / TE;
    const unsigned* const rbf32 = static_cast<const unsigned*>(p.rbf);
    const bf16_t* const hh = static_cast<const bf16_t*>(p.h);
    const bf16_t* const gg = static_cast<const bf16_t*>(p.g);
    const bool chain = p.drbf != nullptr || p.dd != nullptr;

    for (int tile = blockIdx.x * NW + wv; tile < n_tiles; tile += gridDim.x * NW) {
        const int eb = tile * TE, nv = min(TE, Et - eb);
        const bool valid = i < nv;
        const int ec = min(eb + i, Et - 1);
        const unsigned* const hrow = reinterpret_cast<const unsigned*>(hh + (int64_t)p.src[ec] * F);
        const unsigned* const grow = reinterpret_cast<const unsigned*>(gg + (int64_t)p.tgt[ec] * F);
        const float c = valid ? p.cut[ec] : 0.0f;
        wave_lds_fence();
        {
            // rows of G16 / 2 = 25 dwords; dword 25 = the constant 1 of the bias slot; the rest of the 32 dwords zero
            unsigned* rt32 = reinterpret_cast<unsigned*>(rt);
            for (int q = lane; q < TE * 32; q += WAVE) {
                const int row = q >> 5, kd = q & 31;
                unsigned v = kd == G16 / 2 ? 0x00003F80u : 0u;
                if (kd < G16 / 2 && row < nv) v = rbf32[(int64_t)(eb + row) * (G16 / 2) + kd];
                rt32[row * (ES16 / 2) + kd] = v;
            }
        }
        wave_lds_fence();

        // ---- D1 = W1p . r^T, a = ssp: registers 8 t .. 8 t + 7 of lane half h = units 32 b + 16 t + 8 h .. + 7 (cfconv.hip)
        unsigned ad[NB][8];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int k = 0; k < KE16 / 16; ++k)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ld_frag16(w1g, 32 * b + i, ES16, 16 * k, h), ld_frag16(rt, i, ES16, 16 * k, h), acc, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 8; ++q)
                ad[b][q] = pk_bf16(LN2_F * (GT::softplus_u(acc[2 * q]) - 1.0f), LN2_F * (GT::softplus_u(acc[2 * q + 1]) - 1.0f));
        }
        bf16x8 af[2 * NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            af[2 * b] = __builtin_bit_cast(bf16x8, u32x4{ad[b][0], ad[b][1], ad[b][2], ad[b][3]});
            af[2 * b + 1] = __builtin_bit_cast(bf16x8, u32x4{ad[b][4], ad[b][5], ad[b][6], ad[b][7]});
        }
        // unit FP - 1 (lane half 1, the last register) is the constant 1 that carries the bias of layer 2
        if (h == 1) af[2 * NB - 1][7] = (short)0x3F80;

        // ---- D2 = W2p . a -> W rounded to bf16 (what the forward multiplies); q = g[tgt] h[src]; dc; cq = bf16(q c)
        unsigned cd[NB][8];
        float dc = 0.0f;
#pragma unroll
        for (int bo = 0; bo < NB; ++bo) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 2 * NB; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ld_frag16(w2l, 32 * bo + i, LA, 16 * ks, h), af[ks], acc, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int f = 32 * bo + 16 * (q >> 2) + 8 * h + 2 * (q & 3);      // even; F even: f < F covers the pair
                const int fd = min(f, F - 2) >> 1;
                const unsigned gv = grow[fd], hv = hrow[fd];
                const float q0 = f < F ? lo16(gv) * lo16(hv) : 0.0f, q1 = f < F ? hi16(gv) * hi16(hv) : 0.0f;
                const unsigned wd = pk_bf16(acc[2 * q], acc[2 * q + 1]);
                dc = fmaf(q0, lo16(wd), dc);
                dc = fmaf(q1, hi16(wd), dc);
                cd[bo][q] = pk_bf16(q0 * c, q1 * c);
            }
        }
        dc += __shfl_xor(dc, 32);
        if (p.dcut && h == 0 && valid) p.dcut[eb + i] = dc;
        if (!chain) continue;

        bf16x8 cf[2 * NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            cf[2 * b] = __builtin_bit_cast(bf16x8, u32x4{cd[b][0], cd[b][1], cd[b][2], cd[b][3]});
            cf[2 * b + 1] = __builtin_bit_cast(bf16x8, u32x4{cd[b][4], cd[b][5], cd[b][6], cd[b][7]});
        }
        // ---- D3 = W2^T . cq (rows permuted like W1p's: the same register -> unit map as a); da = D3 * sigmoid, from the
        // rounded a as K4b does; replaces a
#pragma unroll
        for (int bo = 0; bo < NB; ++bo) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 2 * NB; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ld_frag16(wt, 32 * bo + i, LA, 16 * ks, h), cf[ks], acc, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned y = ad[bo][q];
                const float s0 = 1.0f - 0.5f * __builtin_amdgcn_exp2f(-LOG2E_F * lo16(y));
                const float s1 = 1.0f - 0.5f * __builtin_amdgcn_exp2f(-LOG2E_F * hi16(y));
                ad[bo][q] = pk_bf16(acc[2 * q] * s0, acc[2 * q + 1] * s1);
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            af[2 * b] = __builtin_bit_cast(bf16x8, u32x4{ad[b][0], ad[b][1], ad[b][2], ad[b][3]});
            af[2 * b + 1] = __builtin_bit_cast(bf16x8, u32x4{ad[b][4], ad[b][5], ad[b][6], ad[b][7]});
        }
        // ---- D4 = W1^T . da (W1p carries log2 e: undone in the epilogue); register r of block gt, half h = Gaussian 32 gt + d_row(r, h)
        f32x16 dr[2];
#pragma unroll
        for (int gt = 0; gt < 2; ++gt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dr[gt][r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 2 * NB; ++ks)
                dr[gt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ld_frag16(w1t, 32 * gt + i, LA, 16 * ks, h), af[ks], dr[gt], 0, 0, 0);
        }

        if (p.drbf) {
            bf16_t* const out = static_cast<bf16_t*>(p.drbf) + (int64_t)(eb + i) * G16;
#pragma unroll
            for (int gt = 0; gt < 2; ++gt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * gt + d_row(r, h);
                    if (valid && k < G16) out[k] = f2bf(dr[gt][r] * LN2_F);
                }
        } else {
            const float dn = p.dnorm[ec];
            float s = 0.0f;
#pragma unroll
            for (int gt = 0; gt < 2; ++gt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * gt + d_row(r, h), kc = min(k, G16 - 1);
                    const float t = (dn - p.offsets[kc]) * bf2f(rt[i * ES16 + kc]);
                    s = fmaf(k < G16 ? dr[gt][r] : 0.0f, t, s);
                }
            s += __shfl_xor(s, 32);
            if (h == 0 && valid) p.dd[eb + i] += (p.scale * p.coeff2 * LN2_F) * s;
        }
    }
}

template <typename K>
static int launch(K kf, const Params& p, int lds, int64_t E, hipStream_t st, const char* name) {
    hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(kf), lds);
    if (e != hipSuccess) { set_error("%s: LDS attribute (%d B): %s", name, lds, hipGetErrorString(e)); return MDL_E_LAUNCH; }
    const int64_t grid = std::min<int64_t>(256, std::max<int64_t>(1, cdiv(cdiv(E, TE), NW)));
    hipLaunchKernelGGL(kf, dim3((unsigned)grid), dim3(NT), lds, st, p);
    return check_launch(name);
}

}  // namespace cfd
}  // namespace mdl

using namespace mdl;

extern "C" int mdl_cfconv_bwd_edge_supported(int F, int G, int dtype) {
    if (dtype == MDL_BF16) return mdl_cfconv_supported(F, G, dtype);
    if (dtype != MDL_F32 || F < 33 || F > 160 || G < 1 || G > 64) return 0;
    return cfd::f32_lds_bytes(F, G, (F + 31) / 32) <= cfd::LDS_CAP;
}

extern "C" int mdl_cfconv_bwd_edge(const void* rbf, const float* cut, const void* h, const void* g, const int32_t* rowptr,
                                   const int32_t* src, const int32_t* tgt, const void* wpack, const float* w1, const float* b1,
                                   const float* w2, const float* b2, int64_t N, int64_t E, int F, int G, int dtype, float* dcut,
                                   void* drbf, const float* d_norm, const float* offsets, float coeff, float scale, float* dd,
                                   mdlStream_t stream) {
    const char* name = "mdl_cfconv_bwd_edge";
    MDL_REQUIRE(mdl_cfconv_bwd_edge_supported(F, G, dtype), MDL_E_UNSUPP,
                "%s: bf16 (G = 50, even F in [64, 158]) or fp32 (F in [33, 160], G <= 64, weights within the LDS) only (F = %d, G = %d, dtype %d)",
                name, F, G, dtype);
    MDL_REQUIRE(N >= 0 && E >= 0 && N < (1ll << 31) && E < (1ll << 31) - 64, MDL_E_ARG, "%s: sizes out of range", name);
    MDL_REQUIRE(!(drbf && dd), MDL_E_ARG, "%s: give drbf (general epilogue) or dd (distance epilogue), not both", name);
    if (N == 0 || E == 0) return MDL_OK;                     // (no edges: nothing to write, and the per-edge pointers may be null)
    MDL_REQUIRE(dcut || drbf || dd, MDL_E_ARG, "%s: no output requested", name);
    MDL_REQUIRE(!dd || (d_norm && offsets), MDL_E_ARG, "%s: the distance epilogue needs d_norm and offsets", name);
    MDL_REQUIRE(rbf && cut && h && g && rowptr && src && tgt, MDL_E_ARG, "%s: null argument", name);
    cfd::Params p{rbf, cut, h, g, rowptr, src, tgt, static_cast<const bf16_t*>(wpack), w1, b1, w2, b2, dcut, drbf, d_norm, offsets, dd,
                  2.0f * coeff, scale, (int)N, F, G};
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MDL_BF16) {
        MDL_REQUIRE(wpack && ((uintptr_t)wpack % 16) == 0 && ((uintptr_t)rbf % 4) == 0 && ((uintptr_t)h % 4) == 0 && ((uintptr_t)g % 4) == 0,
                    MDL_E_ARG, "%s: bf16 needs the packed weights (16-byte aligned) and 4-byte aligned tensors", name);
        switch ((F + 2 + 31) / 32) {                          // the padded width of the packed weights (cfconv.hip: nbk_for)
            case 3: return cfd::launch(cfd::cfconv_de_bf16_kernel<3>, p, cfd::Shape16<3>::LDS, E, st, name);
            case 4: return cfd::launch(cfd::cfconv_de_bf16_kernel<4>, p, cfd::Shape16<4>::LDS, E, st, name);
            default: return cfd::launch(cfd::cfconv_de_bf16_kernel<5>, p, cfd::Shape16<5>::LDS, E, st, name);
        }
    }
    MDL_REQUIRE(w1 && w2, MDL_E_ARG, "%s: fp32 needs the weights W1 [F, G] and W2 [F, F]", name);
    const int NB = (F + 31) / 32, lds = cfd::f32_lds_bytes(F, G, NB);
    switch (NB) {
        case 2: return cfd::launch(cfd::cfconv_de_f32_kernel<2>, p, lds, E, st, name);
        case 3: return cfd::launch(cfd::cfconv_de_f32_kernel<3>, p, lds, E, st, name);
        case 4: return cfd::launch(cfd::cfconv_de_f32_kernel<4>, p, lds, E, st, name);
        default: return cfd::launch(cfd::cfconv_de_f32_kernel<5>, p, lds, E, st, name);
    }
}
