// cgconv_tiles.inc — what the CGConv edge kernels share: build-time switches, CgParams / CgDims, the MFMA fragment types (bf16, exact
// fp32, split bf16), the per-wave tile machinery (edge-tile staging, x-row fragments, weight fragments, one-hot operands, node ranges
// and groups) and the packed bf16 atomics of the by-source sums.  Included by cgconv.hip (K2 + the per-wave K3 + launchers + C ABI) and by
// cgconv_ep.hip (the edge-per-lane K3, its own translation unit with other compiler flags).  Leaves no namespace open.
#pragma once
#include <stdlib.h>
#include <type_traits>

#include "mdl_common.h"

#ifndef MDL_EXPERIMENTS
#define MDL_EXPERIMENTS 0   // 1: the experiments build (experiments/build.py): measured-negative kernel variants and their
                            // environment switches are compiled in; libmdl_hip.so itself never reads the environment
#endif

#ifdef MDL_CG_EP_TU      // compiled a second time as cgconv_ep.hip (see the include of cgconv_ep.inc below): own debug symbols
#define mdl_debug_life mdl_debug_life_ep
#define mdl_debug_read mdl_debug_read_ep
#define mdl_debug_reset mdl_debug_reset_ep
#endif
#ifdef MDL_CG_TIMING   // experiment builds only: per-phase cycle counters of wave 0 (kept in SGPRs, flushed at the end)
__device__ long long g_cg_dbg[48];
__device__ long long g_cg_life[2][4096][3];     // [fwd|bwd][wave] = wall start, wall end, tiles (last launch)
extern "C" int mdl_debug_life(long long* host, int which) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_cg_life), sizeof(long long) * 4096 * 3, sizeof(long long) * 4096 * 3 * which);
}
extern "C" int mdl_debug_read(long long* host48) {
    return (int)hipMemcpyFromSymbol(host48, HIP_SYMBOL(g_cg_dbg), 48 * sizeof(long long));
}
extern "C" int mdl_debug_reset() {
    long long z[48] = {0};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_cg_dbg), z, sizeof(z));
}
#define TDECL const long long tstart = clock64(), wstart = wall_clock64(); long long tprev = tstart; long long tacc[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; long long tcount = 0
#define TMARK(k) do { __builtin_amdgcn_sched_barrier(0); const long long _t = clock64(); tacc[k] += _t - tprev; tprev = _t; __builtin_amdgcn_sched_barrier(0); } while (0)
#define TPIN16(v) do { _Pragma("unroll") for (int _r = 0; _r < 16; ++_r) asm volatile("" : "+v"(v[_r])); } while (0)
#define TTILE() (tcount += 1)
#define TRESET() TMARK(10)
#define TFLUSH(base) do { if (gw == 0 && lane == 0) { for (int _k = 0; _k < 13; ++_k) g_cg_dbg[(base) + _k] += tacc[_k]; g_cg_dbg[(base) + 15] += tcount; g_cg_dbg[(base) + 14] += clock64() - tstart; g_cg_dbg[(base) + 13] += wall_clock64() - wstart; } if (lane == 0 && gw < 4096) { g_cg_life[(base) / 16][gw][0] = wstart; g_cg_life[(base) / 16][gw][1] = wall_clock64(); g_cg_life[(base) / 16][gw][2] = tcount; } } while (0)
#else
#define TDECL do { } while (0)
#define TMARK(k) do { } while (0)
#define TPIN16(v) do { } while (0)
#define TTILE() do { } while (0)
#define TRESET() do { } while (0)
#define TFLUSH(base) do { } while (0)
#endif


namespace mdl {

struct CgParams {
    const void* x;
    const void* ea;
    const int32_t* rowptr;
    const int32_t* src;
    const int32_t* tgt;
    const int32_t* eperm;
    const void* wpack;
    const float* bpack;
    void* out;          // fwd
    const void* gout;   // bwd
    void* r_tgt;        // bwd [N, 2Cp] in the compute dtype (written once per node)
    float* r_src;       // bwd [N, 2Cp]
    float* dwe;         // bwd [2Cp, GP]
    float* db;          // bwd [2Cp] bias gradient = column sums of r_tgt (may be null)
    unsigned* ctr;      // bwd, optional: NS zeroed work counters (caller workspace) -> dynamic group scheduling
    void* ab;           // saved gate factors [E][Cp][2] bf16 (A | B per channel): written by the training forward, read by
                        // the saved-gate backward (cgconv_bwd_ab_kernel)
    const int32_t* balance;   // bwd, optional: [N + 1] non-decreasing cost prefix the workgroups' node ranges are balanced on
                              // (mdl_cgconv_balance); null: edges + nodes in front of a node
    int dwe_combine;    // bwd, per-wave kernel: the two waves of a workgroup that share a channel slice combine their dwe sums in LDS
    int rs16;           // bwd, bf16: r_src is a bf16 array accumulated with packed bf16 atomics (mdl_cgconv_bwd_h)
    int flags;          // host side: MDL_DETERMINISTIC / MDL_K3_* bits the caller OR-ed into `dtype`
    const void* pt;     // W-split kernels: per-node projections P_t = x [W_f,tgt ; W_s,tgt]^T and P_s = x [W_f,src ; W_s,src]^T,
    const void* ps;     // [N, 2Cp] each in the compute dtype (columns f | s), scaled like the packed weights
    int64_t N, E;
    int C, G, Cp, KE, KT, WS, EKS, NS, GP, aggr;
    int GW;             // staging words per e row
    unsigned gw_inv;    // ceil(2^32 / GW)
    int n_groups;
    int g_full;         // bwd, dynamic scheduling: group ids < g_full are 32-node groups, the rest 16-node half groups (tail)
    int w_elems;        // 2*Cp*WS (w_slice: 64*WS)
    int w_slice;        // 1: the workgroup's LDS copy of W holds only the 64 rows of its channel slice (all its waves share the
                        // slice) — wide layers whose packed weights do not fit 160 KB (C = 100: 168 KB) still read them from LDS
    int wave_lds_bytes; // per-wave LDS region
    int bias_col;       // 1: bias lives in K column G of wpack (e tile column G holds 1.0)
};

struct CgDims {
    int Cp, KE, KT, WS, EKS, NS, GP;
};

static inline int rup(int a, int b) { return (a + b - 1) / b * b; }

// x3 (MDL_SPLIT_BF16, fp32 storage): the K = 2C + G product runs as three bf16 MFMAs on split operands, whose fragments are
// 16-byte LDS reads — rows padded by FOUR dwords (an odd number of 16-byte slots) instead of one
static CgDims cg_dims(int C, int G, int dtype, bool x3 = false) {
    CgDims d;
    d.Cp = rup(C, 32);
    d.KE = rup(G, 16);
    d.KT = d.KE + 2 * d.Cp;
    const int pad = dtype == MDL_BF16 ? 8 : (x3 ? 4 : 1);   // bf16: odd number of 16-B slots; f32: odd dword stride
    d.WS = d.KT + pad;
    d.EKS = d.KE + pad;
    d.NS = d.Cp / 32;
    d.GP = rup(G, 64);
    return d;
}

// ------------------------------------------------------------------------------------------
// MFMA traits
// ------------------------------------------------------------------------------------------
template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    static constexpr int KSTEP = 16;
    static constexpr bool FAST = true;
    typedef bf16x8 frag_t;
    __device__ static __forceinline__ f32x16 mma(frag_t a, frag_t b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    __device__ static __forceinline__ frag_t zero() { return frag_t{0, 0, 0, 0, 0, 0, 0, 0}; }
};
template <> struct Mma<float> {
    static constexpr int KSTEP = 2;
    static constexpr bool FAST = false;
    typedef float frag_t;
    __device__ static __forceinline__ f32x16 mma(frag_t a, frag_t b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    }
    __device__ static __forceinline__ frag_t zero() { return 0.0f; }
};

// A/B fragment of a row-major [rows][ld] matrix held in LDS or global memory:
// lane (i = lane&31, h = lane>>5) takes row i, columns k0 + KSTEP/2*h .. (8 bf16 / 1 float).
__device__ __forceinline__ bf16x8 ld_frag(const bf16_t* base, int row, int ld, int k0, int h) {
    return *reinterpret_cast<const bf16x8*>(base + row * ld + k0 + 8 * h);
}
__device__ __forceinline__ float ld_frag(const float* base, int row, int ld, int k0, int h) {
    return base[row * ld + k0 + h];
}

// x-row fragment gathered from global memory with column bound C (columns >= C read as 0).
template <int VEC>
__device__ __forceinline__ bf16x8 ld_xfrag(const bf16_t* rowp, int c0, int h, int C) {
    const int c = c0 + 8 * h;
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (VEC == 9) {            // 16-byte loads, channel count == padded count: no column mask
        v = *reinterpret_cast<const bf16x8*>(rowp + c);
    } else if (VEC == 8) {
        if (c < C) v = *reinterpret_cast<const bf16x8*>(rowp + c);
    } else if (VEC == 4) {
        bf16x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (c < C) lo = *reinterpret_cast<const bf16x4*>(rowp + c);
        if (c + 4 < C) hi = *reinterpret_cast<const bf16x4*>(rowp + c + 4);
        v = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c + j < C) v[j] = (short)rowp[c + j];
    }
    return v;
}
template <int VEC>
__device__ __forceinline__ float ld_xfrag(const float* rowp, int c0, int h, int C) {
    const int c = c0 + h;
    if (VEC == 9) return rowp[c];
    return c < C ? rowp[c] : 0.0f;
}

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
__device__ __forceinline__ bf16x8 pack_bf16x8(const float* v) {
    u32x4 r = {pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7])};
    return __builtin_bit_cast(bf16x8, r);
}

// ------------------------------------------------------------------------------------------
// x3: fp32 values as (hi, lo) bf16 pairs — v = hi + lo to 16 significant bits (both parts rounded to nearest), so that
// a * b ~ a_hi b_hi + a_lo b_hi + a_hi b_lo on the bf16 matrix core at 1/5 of the cost of the exact-fp32 MFMA
// (3 x 32 cycles per 16 k-values against 8 x 64): relative error 2^-16 per product, fp32 accumulation.
// ------------------------------------------------------------------------------------------
struct SplitFrag { bf16x8 hi, lo; };
__device__ __forceinline__ void split_pair(float v0, float v1, unsigned& hi, unsigned& lo) {
    hi = pk_bf16(v0, v1);
    const float r0 = v0 - __builtin_bit_cast(float, hi << 16);
    const float r1 = v1 - __builtin_bit_cast(float, hi & 0xffff0000u);
    lo = pk_bf16(r0, r1);
}
__device__ __forceinline__ SplitFrag split8(const f32x4& a, const f32x4& b) {
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    split_pair(a[0], a[1], h0, l0);
    split_pair(a[2], a[3], h1, l1);
    split_pair(b[0], b[1], h2, l2);
    split_pair(b[2], b[3], h3, l3);
    return SplitFrag{__builtin_bit_cast(bf16x8, u32x4{h0, h1, h2, h3}), __builtin_bit_cast(bf16x8, u32x4{l0, l1, l2, l3})};
}
// eight consecutive fp32 values of a row (16-byte aligned: LDS tile rows of EKS = KE + 4 dwords, or a global x row)
__device__ __forceinline__ SplitFrag split8_at(const float* p) {
    return split8(*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + 4));
}
__device__ __forceinline__ f32x16 mma_x3(const SplitFrag& a, const SplitFrag& b, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, c, 0, 0, 0);
}
// B fragment of the x3 weight pack: a row holds, per group of eight k-values, [8 x hi bf16 | 8 x lo bf16] (32 bytes, the
// footprint of the eight floats it replaces); lane half h of k-step k0 / 16 takes group k0 / 8 + h
__device__ __forceinline__ SplitFrag ld_wfrag_x3(const float* wbase, int row, int ld, int k0, int h) {
    const char* g = reinterpret_cast<const char*>(wbase + row * ld) + (k0 / 8 + h) * 32;
    return SplitFrag{*reinterpret_cast<const bf16x8*>(g), *reinterpret_cast<const bf16x8*>(g + 16)};
}

// ------------------------------------------------------------------------------------------
// Shared per-tile machinery
// ------------------------------------------------------------------------------------------
// Problem dimensions: compile-time when the kernel is instantiated for a fixed (CP_, G_) — loops
// unroll fully, so all loads of a tile are issued before the first MFMA that needs them — or
// run-time (CP_ = 0 / G_ = 0) for the generic fallback.
template <typename T, int CP_, int G_, int EW, int WSP = 0, bool X3 = false>
struct Dims {
    static constexpr bool STATIC = (CP_ != 0) && (G_ != 0);
    static constexpr int PADW = std::is_same<T, bf16_t>::value ? 8 : (X3 ? 4 : 1);
    static_assert(!X3 || (std::is_same<T, float>::value && STATIC && WSP == 0), "x3: fp32 storage, static shapes");
    int C, Cp, G, KE, WS, EKS, GW;
    __device__ __forceinline__ Dims(const CgParams& p) {
        C = p.C;
        Cp = CP_ ? CP_ : p.Cp;
        G = G_ ? G_ : p.G;
        KE = G_ ? ((G_ + 15) / 16 * 16) : p.KE;
        WS = KE + (WSP ? 0 : 2 * Cp) + PADW;      // W-split: the packed weights hold the edge-feature part only
        EKS = KE + PADW;
        GW = G / EW;
    }
};

template <typename T>
struct WaveCtx {
    T* et;              // per-wave e tile  [32][EKS]
    unsigned* tsl;      // per-wave target-slot bytes (32 B) viewed as 8 dwords
    int* srcl;          // per-wave source ids (32 ints)   (backward only)
    unsigned* ssl;      // per-wave source-window slot bytes (32 B) (backward only)
    bf16_t* oh_t;       // one-hot tables (bf16 kernels), see oh_update()
    bf16_t* oh_e;
    bf16_t* oh_w;
    unsigned long long* touched;  // per-wave bitmap of window slots that received an edge (saved-gate kernel)
    unsigned char* touched_b;     // the same as 64 bytes (one per window slot: plain idempotent byte writes, read back with a ballot)
    int* dummy;                   // 64 dwords: where a lane's table writes go when it has nothing to write (branch-free updates)
    const T* wbase;     // packed weights (LDS or global)
};

template <typename T, int EW> struct StageWord {
    typedef typename std::conditional<EW * sizeof(T) == 4, unsigned, unsigned short>::type type;
};

// Generic (run-time G) staging of the 32 x G edge-feature tile: load -> LDS, word by word.
template <typename T, int EW, typename D>
__device__ __forceinline__ void stage_e_tile(const CgParams& p, const D& dm, const WaveCtx<T>& w, int lane, int eb,
                                             int nv, int my_ep) {
    typedef typename StageWord<T, EW>::type word_t;
    const int total = 32 * dm.GW;
    const T* ea = static_cast<const T*>(p.ea);
    for (int q0 = 0; q0 < total; q0 += WAVE) {
        const int q = q0 + lane;
        const bool act = q < total;
        const int row = act ? (int)__umulhi((unsigned)q, p.gw_inv) : 0;
        const int cw = q - row * dm.GW;
        const int ep = p.eperm ? __shfl(my_ep, row) : eb + row;
        if (act && row < nv) {
            const word_t v = *reinterpret_cast<const word_t*>(ea + (int64_t)ep * dm.G + cw * EW);
            *reinterpret_cast<word_t*>(w.et + row * dm.EKS + cw * EW) = v;
        }
    }
}

// Static-G staging, split in two halves so the HBM latency of tile t+1 hides under the compute of
// tile t: prefetch() issues the loads into registers, commit() writes them to the wave's LDS tile
// at the top of the next iteration.
template <typename T, int G_, int EW>
struct EWords {
    typedef typename StageWord<T, EW>::type word_t;
    static constexpr int GW = G_ ? G_ / EW : 1;
    static constexpr int NW = G_ ? (32 * GW + WAVE - 1) / WAVE : 1;
    word_t w[NW];

    // The static kernels are only launched for target-sorted edge features (no eperm; the host permutes
    // once).  Buffer loads: a fresh resource per tile (uniform base in SGPRs, range = the bytes that remain in
    // the array), ONE per-lane 32-bit offset, the word index j in the instruction's 12-bit immediate.  The constant is
    // written as part of the VOFFSET expression (the compiler splits it into register + immediate): the hardware range
    // check covers voffset + immediate only — an SGPR soffset is added AFTER the check, so rows addressed through it
    // would read (or, for stores, write) past the end of the array instead of being dropped.  No predication and no second
    // code path: rows past the end of the group belong to later edges (finite data, multiplied by exact zeros
    // downstream), words past the end of the array fail the range check and read as zeros.  (A clamped second
    // path for the last tile costs more than its instructions: every control-flow join in the tile loop makes
    // hipcc's wait-count bookkeeping assume the worse of the two paths.)
    __device__ __forceinline__ void prefetch(const CgParams& p, int lane, int eb, int /*nv*/, int /*my_ep*/) {
        constexpr int WB = EW * (int)sizeof(T);
        static_assert(WB == 4 || WB == 2, "staging word");
        const char* tb = reinterpret_cast<const char*>(p.ea) + (int64_t)eb * (G_ * (int)sizeof(T));
        const int64_t rem = (p.E - (int64_t)eb) * (G_ * (int)sizeof(T));
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(tb), 0, (int)(rem < 0 ? 0 : (rem < 0x7fffffffLL ? rem : 0x7fffffffLL)), 0x00020000);
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            if constexpr (WB == 4) w[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, lane * WB + j * (WAVE * WB), 0, 0);
            else w[j] = __builtin_amdgcn_raw_buffer_load_b16(rs, lane * WB + j * (WAVE * WB), 0, 0);
        }
    }
    __device__ __forceinline__ void commit(T* et, int EKS, int lane) const {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int q = j * WAVE + lane;
            const int row = q / GW, cw = q - row * GW;
            if (row < 32) *reinterpret_cast<word_t*>(et + row * EKS + cw * EW) = w[j];
        }
    }
};

// x-row A fragments of one tile (target rows and source rows), all issued up front when the
// channel count is static.
template <typename T, int CP_, int VEC, bool X3 = false>
struct XFrags {
    typedef Mma<T> M;
    static constexpr int NF = CP_ ? CP_ / M::KSTEP : 1;
    typename M::frag_t t[NF], s[NF];
    __device__ __forceinline__ void load(const T* x, int C, int my_tgt, int my_src, int h) {
        const T* xt = x + (int64_t)my_tgt * C;
        const T* xs = x + (int64_t)my_src * C;
#pragma unroll
        for (int f = 0; f < NF; ++f) t[f] = ld_xfrag<VEC>(xt, f * M::KSTEP, h, C);
#pragma unroll
        for (int f = 0; f < NF; ++f) s[f] = ld_xfrag<VEC>(xs, f * M::KSTEP, h, C);
    }
};
// x3: the raw fp32 chunks of the two rows (16-byte loads; same 2 x CP_ / 2 registers as the k-pair fragments of the exact
// form): chunk f of a row = columns 16 f + 8 h .. + 7, split into (hi, lo) where it is used
template <int CP_, int VEC>
struct XFrags<float, CP_, VEC, true> {
    static constexpr int NF = CP_ / 16;
    f32x4 t[NF][2], s[NF][2];
    __device__ __forceinline__ void load(const float* x, int C, int my_tgt, int my_src, int h) {
        const float* xt = x + (int64_t)my_tgt * C + 8 * h;
        const float* xs = x + (int64_t)my_src * C + 8 * h;
#pragma unroll
        for (int f = 0; f < NF; ++f) { t[f][0] = *reinterpret_cast<const f32x4*>(xt + 16 * f); t[f][1] = *reinterpret_cast<const f32x4*>(xt + 16 * f + 4); }
#pragma unroll
        for (int f = 0; f < NF; ++f) { s[f][0] = *reinterpret_cast<const f32x4*>(xs + 16 * f); s[f][1] = *reinterpret_cast<const f32x4*>(xs + 16 * f + 4); }
    }
};

// W-split (SURVEY section 7, VERDICT round 2 item 2): z W^T = e W_e^T + P_t[tgt] + P_s[src] with per-node projections
// P = x [W_tgt | W_src]^T from ONE dense launch per layer, so that per edge only the K = 64 edge-feature product remains.
// The gathered projection rows enter the accumulators through the matrix core: they ARE A fragments (lane = edge, eight
// consecutive columns = 16 bytes, exactly like the x rows they replace) of a product with an IDENTITY B operand —
// D[edge][ch] += sum_k P[edge][k] (k == ch) — two k-steps per 32-channel block instead of the K = 64 (four k-steps) of the
// x part, no unpack / add VALU, no weight-fragment LDS reads.
// Fragment f of a slice: column (f >> 1) * Cp + 32 * slice + 16 * (f & 1) of the [f | s] row, i.e. (part f / s, k-step).
template <int CP_, int NSLF>
struct PFrags {
    bf16x8 t[4 * NSLF], s[4 * NSLF];
    __device__ __forceinline__ void load(const void* pt, const void* ps, int my_tgt, int my_src, int h, int sl0) {
        const bf16_t* a = static_cast<const bf16_t*>(pt) + (int64_t)my_tgt * (2 * CP_) + 8 * h + 32 * sl0;
        const bf16_t* b = static_cast<const bf16_t*>(ps) + (int64_t)my_src * (2 * CP_) + 8 * h + 32 * sl0;
#pragma unroll
        for (int q = 0; q < 4 * NSLF; ++q) t[q] = *reinterpret_cast<const bf16x8*>(a + ((q >> 1) & 1) * CP_ + 32 * (q >> 2) + 16 * (q & 1));
#pragma unroll
        for (int q = 0; q < 4 * NSLF; ++q) s[q] = *reinterpret_cast<const bf16x8*>(b + ((q >> 1) & 1) * CP_ + 32 * (q >> 2) + 16 * (q & 1));
    }
};
// identity B fragments of the 32 x 32 product in two k-steps: B[k][n] = (k == n), lane n, k = 16 ks + 8 h + q
__device__ __forceinline__ void identity_frags(int i, int h, bf16x8 (&idf)[2]) {
    typedef __attribute__((ext_vector_type(4))) unsigned u4_t;
    const bool mine = ((i >> 3) & 1) == h;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const unsigned one = (mine && (i >> 4) == ks) ? (0x3F80u << (16 * (i & 1))) : 0u;
        const int d = (i & 7) >> 1;
        const u4_t v = {d == 0 ? one : 0u, d == 1 ? one : 0u, d == 2 ? one : 0u, d == 3 ? one : 0u};
        idf[ks] = __builtin_bit_cast(bf16x8, v);
    }
}
// pre-activation tile of slice `sl` (global) whose projection fragments sit at local slice `sll` of pf
template <int CP_, int NSLF, int DEPTH, typename D>
__device__ __forceinline__ void pre_tile_wsp(const D& dm, const WaveCtx<bf16_t>& w, int lane, int sl, int sll,
                                             const PFrags<CP_, NSLF>& pf, const bf16x8 (&idf)[2], f32x16& accf, f32x16& accs) {
    const int i = lane & 31, h = lane >> 5;
    const int rowf = sl * 32 + i, rows = dm.Cp + sl * 32 + i;
#pragma unroll
    for (int k0 = 0; k0 < dm.KE; k0 += 16) {
        const bf16x8 a = ld_frag(w.et, i, dm.EKS, k0, h);
        accf = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ld_frag(w.wbase, rowf, dm.WS, k0, h), accf, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ld_frag(w.wbase, rows, dm.WS, k0, h), accs, 0, 0, 0);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        accf = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf.t[4 * sll + ks], idf[ks], accf, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf.t[4 * sll + 2 + ks], idf[ks], accs, 0, 0, 0);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        accf = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf.s[4 * sll + ks], idf[ks], accf, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf.s[4 * sll + 2 + ks], idf[ks], accs, 0, 0, 0);
    }
    if constexpr (DEPTH > 0) {      // weight-fragment reads of the edge-feature part a few deep ahead of the chain
        __builtin_amdgcn_sched_group_barrier(0x100, DEPTH, 0);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
    }
}

// pre-activation tile: accf/accs (32 edge slots x 32 channels of slice s), bias pre-loaded.
template <typename T, int CP_, int VEC, int WM, int DEPTH = 0, bool X3 = false, typename D>
__device__ __forceinline__ void pre_tile(const CgParams& p, const D& dm, const WaveCtx<T>& w, int lane, int s,
                                         int my_tgt, int my_src, const XFrags<T, CP_, VEC, X3>& xf,
                                         f32x16& accf, f32x16& accs) {
    typedef Mma<T> M;
    const int i = lane & 31, h = lane >> 5;
    const bool wsl = (CP_ == 0 || CP_ > 64) && p.w_slice;    // (never for the static shapes whose W fits LDS: folds away there)
    const int rowf = (wsl ? 0 : s * 32) + i, rows = (wsl ? 32 : dm.Cp + s * 32) + i;
    if constexpr (X3) {
        // fp32 storage, split-bf16 products: z fragments split where they are read (e tile: 2 ds_read_b128 per fragment; x
        // chunks: registers), weight fragments pre-split by the pack kernel (no arithmetic here)
        static_assert(WM == 1 && CP_ != 0, "x3: static shapes, W in LDS");
#pragma unroll
        for (int k0 = 0; k0 < dm.KE; k0 += 16) {
            const SplitFrag a = split8_at(w.et + i * dm.EKS + k0 + 8 * h);
            accf = mma_x3(a, ld_wfrag_x3(w.wbase, rowf, dm.WS, k0, h), accf);
            accs = mma_x3(a, ld_wfrag_x3(w.wbase, rows, dm.WS, k0, h), accs);
        }
        constexpr int NF = CP_ / 16;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const SplitFrag a = split8(xf.t[f][0], xf.t[f][1]);   // (both channel slices of a tile split the same chunks: the compiler merges them)
            accf = mma_x3(a, ld_wfrag_x3(w.wbase, rowf, dm.WS, dm.KE + 16 * f, h), accf);
            accs = mma_x3(a, ld_wfrag_x3(w.wbase, rows, dm.WS, dm.KE + 16 * f, h), accs);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const SplitFrag a = split8(xf.s[f][0], xf.s[f][1]);
            accf = mma_x3(a, ld_wfrag_x3(w.wbase, rowf, dm.WS, dm.KE + dm.Cp + 16 * f, h), accf);
            accs = mma_x3(a, ld_wfrag_x3(w.wbase, rows, dm.WS, dm.KE + dm.Cp + 16 * f, h), accs);
        }
        return;
    } else {
    // edge features (LDS tile)
#pragma unroll
    for (int k0 = 0; k0 < dm.KE; k0 += M::KSTEP) {
        typename M::frag_t a = ld_frag(w.et, i, dm.EKS, k0, h);
        accf = M::mma(a, ld_frag(w.wbase, rowf, dm.WS, k0, h), accf);
        accs = M::mma(a, ld_frag(w.wbase, rows, dm.WS, k0, h), accs);
    }
    if constexpr (CP_ != 0) {
        constexpr int NF = XFrags<T, CP_, VEC>::NF;
#pragma unroll
        for (int f = 0; f < NF; ++f) {      // target-node features (x_i)
            accf = M::mma(xf.t[f], ld_frag(w.wbase, rowf, dm.WS, dm.KE + f * M::KSTEP, h), accf);
            accs = M::mma(xf.t[f], ld_frag(w.wbase, rows, dm.WS, dm.KE + f * M::KSTEP, h), accs);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {      // source-node features (x_j)
            accf = M::mma(xf.s[f], ld_frag(w.wbase, rowf, dm.WS, dm.KE + dm.Cp + f * M::KSTEP, h), accf);
            accs = M::mma(xf.s[f], ld_frag(w.wbase, rows, dm.WS, dm.KE + dm.Cp + f * M::KSTEP, h), accs);
        }
        // Pin the schedule of the chain: DEPTH fragment reads up front, then one read behind every MFMA, so
        // that the LDS latency of a weight fragment hides under the MFMAs issued before it.  (Left alone, hipcc keeps
        // one or two reads in flight and every MFMA waits out a full LDS round trip.)
        if constexpr (DEPTH > 0 && std::is_same<T, bf16_t>::value) {
            constexpr int NMMA = 2 * (D::STATIC ? ((50 + 15) / 16 + 2 * NF) : 0);
            __builtin_amdgcn_sched_group_barrier(0x100, DEPTH, 0);
#pragma unroll
            for (int q = 0; q < NMMA; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
        }
    } else {
        const T* xt = static_cast<const T*>(p.x) + (int64_t)my_tgt * dm.C;
        const T* xs = static_cast<const T*>(p.x) + (int64_t)my_src * dm.C;
        for (int k0 = 0; k0 < dm.Cp; k0 += M::KSTEP) {
            typename M::frag_t a = ld_xfrag<VEC>(xt, k0, h, dm.C);
            accf = M::mma(a, ld_frag(w.wbase, rowf, dm.WS, dm.KE + k0, h), accf);
            accs = M::mma(a, ld_frag(w.wbase, rows, dm.WS, dm.KE + k0, h), accs);
        }
        for (int k0 = 0; k0 < dm.Cp; k0 += M::KSTEP) {
            typename M::frag_t a = ld_xfrag<VEC>(xs, k0, h, dm.C);
            accf = M::mma(a, ld_frag(w.wbase, rowf, dm.WS, dm.KE + dm.Cp + k0, h), accf);
            accs = M::mma(a, ld_frag(w.wbase, rows, dm.WS, dm.KE + dm.Cp + k0, h), accs);
        }
    }
    }   // (!X3)
}

// acc[node slot][ch] += sum over the tile's edge slots of onehot(slot -> node slot) * v[edge slot][ch]
// v is in D layout (lane = channel, register r = edge slot d_row(r, h)); t4 = the lane's 4 dwords of
// target-slot bytes (byte r&3 of t4[r>>2] is the node slot of edge slot d_row(r,h), 0xff = invalid).
template <typename T>
__device__ __forceinline__ void seg_reduce_mma(const f32x16& v, const unsigned t4[4], int ns, f32x16& acc) {
    if constexpr (std::is_same<T, bf16_t>::value) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a;
            float vv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = 8 * ks + q;
                const unsigned slot = (t4[r >> 2] >> (8 * (r & 3))) & 0xffu;
                a[q] = (slot == (unsigned)ns) ? (short)0x3F80 : (short)0;
                vv[q] = v[r];
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pack_bf16x8(vv), acc, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned slot = (t4[r >> 2] >> (8 * (r & 3))) & 0xffu;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32((slot == (unsigned)ns) ? 1.0f : 0.0f, v[r], acc, 0, 0, 0);
        }
    }
}

// x3: the same reduction on the bf16 matrix core with the values split into (hi, lo) — the one-hot operand is exact in bf16, so
// the sums carry the values' 16 bits: 4 MFMAs of 32 cycles instead of 16 exact-fp32 MFMAs of 64
__device__ __forceinline__ void seg_reduce_mma_x3(const f32x16& v, const unsigned t4[4], int ns, f32x16& acc) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 a;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 8 * ks + q;
            const unsigned slot = (t4[r >> 2] >> (8 * (r & 3))) & 0xffu;
            a[q] = (slot == (unsigned)ns) ? (short)0x3F80 : (short)0;
        }
        const SplitFrag b = split8(f32x4{v[8 * ks], v[8 * ks + 1], v[8 * ks + 2], v[8 * ks + 3]},
                                   f32x4{v[8 * ks + 4], v[8 * ks + 5], v[8 * ks + 6], v[8 * ks + 7]});
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b.lo, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b.hi, acc, 0, 0, 0);
    }
}

// One-hot operand tables in LDS (bf16 kernels).  Building a one-hot MFMA operand in registers costs
// ~3 VALU per element (extract, compare, select, pack); instead every edge-slot lane keeps ONE 1.0 in
// a small per-wave LDS table up to date (clear the old position, set the new one: 2 ds_write_b16) and
// the consumers read their operand fragments with ds_read_b128.
//   oh_t [32 node slots ][OHS]  column pos(edge slot): 1 where the edge's target is the row's node slot
//   oh_e [32 edge slots ][OHS]  column node slot     : 1 at the edge's target slot   (grad_out expansion)
//   oh_w [64 window slot][OHS]  column pos(edge slot): 1 where the edge's source is the row's window slot
// pos() is the K order in which the D-layout registers of a lane map onto MFMA K slots.
constexpr int OHS = 40;                                   // row stride in bf16 (80 B: odd number of 16-B slots)
__device__ __forceinline__ int oh_pos(int slot) {         // inverse of slot = d_row(8*ks + q, h), pos = 16*ks + 8*h + q
    const int hh = (slot >> 2) & 1, r = (slot & 3) + 4 * (slot >> 3);
    return 16 * (r >> 3) + 8 * hh + (r & 7);
}
__device__ __forceinline__ void oh_update(bf16_t* tab, int old_row, int new_row, int colpos) {
    if (old_row != new_row) {
        if (old_row >= 0) tab[old_row * OHS + colpos] = 0;
        if (new_row >= 0) tab[new_row * OHS + colpos] = 0x3F80;
    }
}
__device__ __forceinline__ bf16x8 oh_frag(const bf16_t* tab, int row, int ks, int h) {
    return *reinterpret_cast<const bf16x8*>(tab + row * OHS + 16 * ks + 8 * h);
}

// dpre fragments of one tile, packed once and used three times (B operand of the two segmented
// reductions, A operand of the dwe product).  bf16: 2 K-steps of 8 values; f32: the 16 registers.
template <typename T> struct DFrags;
template <> struct DFrags<bf16_t> {
    bf16x8 f[2], s[2];
    __device__ __forceinline__ void pack(const f32x16& af, const f32x16& as) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            float a[8], b[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { a[q] = af[8 * ks + q]; b[q] = as[8 * ks + q]; }
            f[ks] = pack_bf16x8(a);
            s[ks] = pack_bf16x8(b);
        }
    }
};
template <> struct DFrags<float> {
    f32x16 f, s;
    __device__ __forceinline__ void pack(const f32x16& af, const f32x16& as) { f = af; s = as; }
};

// x3: dpre of one tile as (hi, lo) bf16 fragments, split ONCE and used by the three segmented reductions and the dwe product
struct DFragsX3 {
    SplitFrag f[2], s[2];
    __device__ __forceinline__ void pack(const f32x16& af, const f32x16& as) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f[ks] = split8(f32x4{af[8 * ks], af[8 * ks + 1], af[8 * ks + 2], af[8 * ks + 3]},
                           f32x4{af[8 * ks + 4], af[8 * ks + 5], af[8 * ks + 6], af[8 * ks + 7]});
            s[ks] = split8(f32x4{as[8 * ks], as[8 * ks + 1], as[8 * ks + 2], as[8 * ks + 3]},
                           f32x4{as[8 * ks + 4], as[8 * ks + 5], as[8 * ks + 6], as[8 * ks + 7]});
        }
    }
};
__device__ __forceinline__ void seg_reduce2_x3(const DFragsX3& d, const unsigned b4[4], unsigned row_id, f32x16& accF, f32x16& accS) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 a;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 8 * ks + q;
            const unsigned slot = (b4[r >> 2] >> (8 * (r & 3))) & 0xffu;
            a[q] = (slot == row_id) ? (short)0x3F80 : (short)0;
        }
        accF = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, d.f[ks].lo, accF, 0, 0, 0);
        accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, d.s[ks].lo, accS, 0, 0, 0);
        accF = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, d.f[ks].hi, accF, 0, 0, 0);
        accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, d.s[ks].hi, accS, 0, 0, 0);
    }
}

// accF/accS[slot row][ch] += onehot(byte(edge slot) == row_id) x dpre   (see seg_reduce_mma)
template <typename T>
__device__ __forceinline__ void seg_reduce2(const DFrags<T>& d, const unsigned b4[4], unsigned row_id, f32x16& accF,
                                            f32x16& accS) {
    if constexpr (std::is_same<T, bf16_t>::value) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = 8 * ks + q;
                const unsigned slot = (b4[r >> 2] >> (8 * (r & 3))) & 0xffu;
                a[q] = (slot == row_id) ? (short)0x3F80 : (short)0;
            }
            accF = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, d.f[ks], accF, 0, 0, 0);
            accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, d.s[ks], accS, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned slot = (b4[r >> 2] >> (8 * (r & 3))) & 0xffu;
            const float a = (slot == row_id) ? 1.0f : 0.0f;
            accF = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d.f[r], accF, 0, 0, 0);
            accS = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d.s[r], accS, 0, 0, 0);
        }
    }
}

// bf16: one-hot A fragments come from an LDS table (oh_t / oh_w) instead of being built in registers
__device__ __forceinline__ void seg_reduce2_tab(const DFrags<bf16_t>& d, const bf16_t* tab, int row, int h,
                                                f32x16& accF, f32x16& accS) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 a = oh_frag(tab, row, ks, h);
        accF = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, d.f[ks], accF, 0, 0, 0);
        accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, d.s[ks], accS, 0, 0, 0);
    }
}

template <typename T, typename D>
__device__ __forceinline__ void setup_wave(const CgParams& p, const D& dm, char* smem, bool w_lds, WaveCtx<T>& w) {
    const int wave = threadIdx.x >> 6;
    const int w_bytes = w_lds ? ((p.w_elems * (int)sizeof(T) + 15) & ~15) : 0;
    char* base = smem + w_bytes + wave * p.wave_lds_bytes;
    w.et = reinterpret_cast<T*>(base);
    const int et_bytes = (32 * dm.EKS * (int)sizeof(T) + 15) & ~15;
    w.tsl = reinterpret_cast<unsigned*>(base + et_bytes);
    w.srcl = reinterpret_cast<int*>(base + et_bytes + 32);
    w.ssl = reinterpret_cast<unsigned*>(base + et_bytes + 32 + 128);
    w.touched = reinterpret_cast<unsigned long long*>(base + et_bytes + 32 + 128 + 32);
    w.oh_t = reinterpret_cast<bf16_t*>(base + et_bytes + 32 + 128 + 32 + 16);
    w.oh_e = w.oh_t + 32 * OHS;
    w.oh_w = w.oh_e + 32 * OHS;
    w.touched_b = reinterpret_cast<unsigned char*>(w.oh_w + 64 * OHS);
    w.dummy = reinterpret_cast<int*>(w.touched_b + 64);
    w.wbase = w_lds ? reinterpret_cast<const T*>(smem) : static_cast<const T*>(p.wpack);
    if (w_lds && p.w_slice) {
        // rows [32 s, +32) of the f part and of the s part -> LDS rows [0, 32) and [32, 64)   (WS * sizeof(T) % 16 == 0)
        const int sl = (int)blockIdx.x % p.NS;
        const int row16 = dm.WS * (int)sizeof(T) / 16;
        const f32x4* g = reinterpret_cast<const f32x4*>(p.wpack);
        f32x4* l = reinterpret_cast<f32x4*>(smem);
        for (int q = threadIdx.x; q < 64 * row16; q += blockDim.x) {
            const int r = q / row16, c = q - r * row16;
            const int gr = (r < 32 ? 32 * sl + r : dm.Cp + 32 * sl + (r - 32));
            l[q] = g[(int64_t)gr * row16 + c];
        }
    } else if (w_lds) {
        const f32x4* g = reinterpret_cast<const f32x4*>(p.wpack);
        f32x4* l = reinterpret_cast<f32x4*>(smem);
        const int n16 = w_bytes / 16;
        for (int q = threadIdx.x; q < n16; q += blockDim.x) l[q] = g[q];
    }
    // zero the e tile once: padded columns [G, KE) stay 0 forever, rows never hold garbage bits
    unsigned* z = reinterpret_cast<unsigned*>(base);
    for (int q = threadIdx.x & 63; q < p.wave_lds_bytes / 4; q += WAVE) z[q] = 0u;
    wave_lds_fence();
    // bias column: e-tile column G is a constant 1 whose weight row holds the bias
    if (p.bias_col && (threadIdx.x & 63) < 32) Elem<T>::st(w.et + (threadIdx.x & 63) * dm.EKS + dm.G, 1.0f);
    __syncthreads();
}

// per-lane indices of one edge tile (lane i and lane i+32 hold the same edge slot i)
struct TileIdx {
    int src, tgt, ep;
    template <bool WITH_EP = true, bool GUARD_EMPTY = true>
    __device__ __forceinline__ void load(const CgParams& p, int eb, int e1, int i, int n0) {
        // RAW loads on a clamped index, nothing else.  Slots past the end of the group (eb + i >= e1) get
        // the indices of the group's last edge: valid rows whose contribution every consumer masks by
        // slot validity (i < nv).  No select / arithmetic on the loaded values here: this is called
        // inside `if (more tiles)` blocks, and any use of a loaded value inside the block makes hipcc
        // wait for it (and for every older load, i.e. the x gathers issued just before) at that point.
        // Likewise never `cond ? load : x`: hipcc branches around the load and waits at the join.
        if (GUARD_EMPTY && p.E == 0) { src = tgt = n0; ep = 0; return; }   // uniform: graph without edges (callers inside
                                                                           // a tile loop know e1 > 0 and drop the branch)
        const int ec = max(min(eb + i, e1 - 1), 0);
        src = p.src[ec];
        tgt = p.tgt[ec];
        ep = 0;
        if (WITH_EP && p.eperm) ep = p.eperm[ec];
    }
};

// ------------------------------------------------------------------------------------------
// Forward
// ------------------------------------------------------------------------------------------
// seg_reduce_mma + in-degree count: cnt[node slot][*] += number of edge slots of the tile that map to
// the node slot (one-hot x all-ones), so the epilogue needs no rowptr loads.
template <typename T>
__device__ __forceinline__ void seg_reduce_cnt(const f32x16& v, const unsigned t4[4], int ns, f32x16& acc,
                                               f32x16& cnt) {
    if constexpr (std::is_same<T, bf16_t>::value) {
        const bf16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a;
            float vv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = 8 * ks + q;
                const unsigned slot = (t4[r >> 2] >> (8 * (r & 3))) & 0xffu;
                a[q] = (slot == (unsigned)ns) ? (short)0x3F80 : (short)0;
                vv[q] = v[r];
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pack_bf16x8(vv), acc, 0, 0, 0);
            cnt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, cnt, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned slot = (t4[r >> 2] >> (8 * (r & 3))) & 0xffu;
            const float a = (slot == (unsigned)ns) ? 1.0f : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v[r], acc, 0, 0, 0);
            cnt = __builtin_amdgcn_mfma_f32_32x32x2f32(a, 1.0f, cnt, 0, 0, 0);
        }
    }
}

// Work partition: wave `wi` of `W` owns the contiguous NODE range [na, nb) whose incoming edges are the
// wi-th of W equal shares of the edge array (boundaries rounded to node boundaries), found with a wave-wide
// 64-ary search on rowptr.  Ranges partition [0, N); a node's edges are never split, so no cross-wave
// combination is needed, every wave carries the same number of edge tiles (+-1) whatever N is, and small
// batches still spread over the whole chip.  Inside its range a wave walks groups of up to 32 nodes.
// The balanced quantity is w(n) = rowptr[n] + n (edges + nodes in front of node n): strictly increasing, so nodes WITHOUT
// edges are spread over the waves too — the padding nodes of a static batch (thousands of empty rows behind the last real
// node) would otherwise all fall to the last wave, which then walks them group by group while the chip idles.
__device__ __forceinline__ int wave_lower_bound(const int32_t* __restrict__ rowptr, int N, int64_t b, int lane) {
    int lo = 0, hi = N;                        // answer = first n in [lo, hi] with w(n) >= b  (w(N) = E + N >= b)
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;  // >= 1
        const int n = min(lo + lane * step, hi);
        const unsigned long long ge = __ballot((int64_t)rowptr[n] + n >= b);   // monotone in lane
        if (ge == 0ull) { lo = min(lo + 63 * step, hi) + 1; continue; }   // all probes below b
        const int fl = __builtin_ctzll(ge);
        if (fl == 0) { hi = lo; break; }
        hi = min(lo + fl * step, hi);
        lo = lo + (fl - 1) * step + 1;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}
// the same search on an explicit non-decreasing key array key[0..N]
__device__ __forceinline__ int wave_lower_bound_key(const int32_t* __restrict__ key, int N, int64_t b, int lane) {
    int lo = 0, hi = N;
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;
        const int n = min(lo + lane * step, hi);
        const unsigned long long ge = __ballot((int64_t)key[n] >= b);
        if (ge == 0ull) { lo = min(lo + 63 * step, hi) + 1; continue; }
        const int fl = __builtin_ctzll(ge);
        if (fl == 0) { hi = lo; break; }
        hi = min(lo + fl * step, hi);
        lo = lo + (fl - 1) * step + 1;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}
struct NodeRange {
    int na, nb;
    __device__ __forceinline__ NodeRange(int a, int b) : na(a), nb(b) {}
    __device__ __forceinline__ NodeRange(const CgParams& p, int wi, int W, int lane) {
        // the edges that exist = rowptr[N], which may be fewer than the p.E slots of the edge arrays (padded static
        // batches of the HIP-graph path): balancing on p.E would search for edge counts rowptr never reaches
        const int64_t Et = (int64_t)p.rowptr[p.N] + p.N;
        const int64_t b0 = Et * (int64_t)wi / W, b1 = Et * (int64_t)(wi + 1) / W;
        na = (wi == 0) ? 0 : wave_lower_bound(p.rowptr, (int)p.N, b0, lane);
        nb = (wi == W - 1) ? (int)p.N : wave_lower_bound(p.rowptr, (int)p.N, b1, lane);
    }
};
// scalars of one group of <= 32 nodes [n0, n1) inside a wave's node range
struct GroupInfo {
    int n0, n1, e0, e1;
    __device__ __forceinline__ void load(const CgParams& p, int n0_, int nb) {
        n0 = n0_;                                 // wave-uniform: the two loads become s_load
        n1 = min(n0 + 32, nb);
        e0 = p.rowptr[n0];
        e1 = p.rowptr[n1];
    }
};

// By-source sums in bf16 (p.rs16): two fp32 atomics per (row, lane) become ONE packed bf16 atomic per TWO rows.  A lane holds
// column c of rows R (value va) and R + 1 (vb); neighbouring lanes hold neighbouring columns.  Even lanes take the pair
// (c, c + 1) of row R, odd lanes the pair (c - 1, c) of row R + 1: each lane hands its partner (lane ^ 1) the value the partner
// needs with one DPP quad permute, packs with one v_cvt_pk_bf16_f32 and issues global_atomic_pk_add_bf16 on a 4-byte
// aligned column pair — half the atomic operations AND half the bytes of the fp32 form (atomic throughput at the L2 is what the
// window flush costs: ablated, 45 of 585 us).  ca / cb: whether row R / R + 1 is to be added at all.
__device__ __forceinline__ void rsrc16_add2(bf16_t* base_even_col, int64_t rowa_elems, int64_t rowb_elems, float va, float vb,
                                            bool ca, bool cb, int odd) {
    typedef __bf16 __attribute__((ext_vector_type(2))) bf2v;
    typedef __attribute__((address_space(1))) bf2v* gptr_t;
    const float send = odd ? va : vb;
    const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, false));
    const float lo = odd ? recv : va, hi = odd ? vb : recv;
    if (odd ? cb : ca) {
        const unsigned pk = pk_bf16(lo, hi);
        __builtin_amdgcn_global_atomic_fadd_v2bf16((gptr_t)(base_even_col + (odd ? rowb_elems : rowa_elems)), __builtin_bit_cast(bf2v, pk));
    }
}

}  // namespace mdl
