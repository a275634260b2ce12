// cgconv_ep2.inc — edge-per-lane CGConv backward with SPECIALISED waves (included by cgconv.hip in the cgconv_ep.hip unit).
//
// What the ablations of the first edge-per-lane kernel (cgconv_ep.inc) showed on the bench batch: its phase A alone takes
// 366 us, its phase B 282 us, gate arithmetic + pre-activation MFMAs together only 150 us — both phases are bound by
// dependent latencies (LDS round trips, MFMA results, atomics, barriers) that one wave per SIMD cannot hide, and they run one
// after the other.  Here they run BESIDE each other: a 512-thread workgroup has four PRODUCER waves (phase A: one tile each,
// all 2C gate columns, nothing persistent) and four REDUCER waves (phase B: one 32-column block each over the four tiles of
// the PREVIOUS round, 96 accumulator registers, no transient state).  A workgroup's waves are dealt to the SIMDs cyclically,
// so every SIMD hosts one producer and one reducer: the VALU-heavy gate arithmetic of one fills the LDS / MFMA / atomic
// latencies of the other.  Both fit 256 registers (two waves per SIMD), the tile buffers are double-buffered (the set the
// producers fill in round r is reduced in round r + 1) and ONE barrier per round orders everything.
// To fit two buffer sets beside the weights in 160 KB the one-hot operand tables of cgconv_ep.inc are gone: the producers
// leave two bytes per edge (target slot, window slot) and the reducers build the one-hot MFMA fragments from them with
// integer arithmetic (a zero-byte test on four slots at a time) — VALU work on waves that are otherwise idle on that pipe.

namespace ep {

template <int C_>
struct Cfg2 {
    static constexpr int NB = 2 * C_ / 32;              // gate column blocks = reducer waves
    static constexpr int NA = 4;                        // producer waves = tiles per round
    static constexpr int NT = (NA + NB) * WAVE;
    static constexpr int G = 50, KE = 64, EKS = KE + 8;
    static constexpr int KT = KE + 2 * C_;
    static constexpr int WS = KT + 8;
    static constexpr int NKX = C_ / 16;
    static constexpr int NWT = 4;                       // 32-row blocks of the by-source window
    static constexpr int WOFF = 48;                     // rows of the window in front of the group's first node
    static constexpr int NCH = 2 * C_ / 4;
    static constexpr int DCS = 32 * 8 + 32;
    static constexpr int W_BYTES = 2 * C_ * WS * 2;
    static constexpr int OFF_ET = 0;
    static constexpr int OFF_DP = OFF_ET + 32 * EKS * 2;
    static constexpr int OFF_TSL = OFF_DP + NCH * DCS;   // 32 halfwords: target slot of every edge slot (0xffff = none)
    static constexpr int OFF_SSL = OFF_TSL + 64;         // 32 halfwords: window slot (0xffff = none / outside)
    static constexpr int OFF_META = OFF_SSL + 64;
    static constexpr int BUF = OFF_META + 32;
    static constexpr int LDS = W_BYTES + 2 * NA * BUF;
    static_assert(NB == 4 && NA == 4, "written for C = 64");
    static_assert(WOFF >= 0 && WOFF < 32 * NWT, "window layout");
    static_assert(W_BYTES % 16 == 0 && BUF % 16 == 0 && OFF_DP % 16 == 0 && OFF_TSL % 16 == 0 && OFF_META % 16 == 0, "alignment");
    static_assert(LDS <= 160 * 1024, "LDS budget");
};

// one dword (two bf16 one-hot values) for two consecutive k-slots whose row ids are the halfwords of D, nonzero where the
// halfword equals the row id replicated in rsplat.  The slots travel shifted left by 7 (the exponent field of a bf16), so the
// xor of two different slots is >= 0x0080 and ONE saturating 0x0080 - x leaves 0x0080 (= 2^-126, the smallest normal bf16)
// where they are equal and 0 elsewhere: two packed 16-bit instructions per pair.  The products stay normal fp32 numbers
// because the producers scale dpre by 2^64 on the way into the tile (folded into the 1 / deg factor: no instruction); the
// flushes divide it out (folded into their scale factor).
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
constexpr int OHK_SH = 7;
constexpr float OHK_UP = 18446744073709551616.0f;            // 2^64: what the producers multiply dpre by
constexpr float OHK_DOWN = 1.0f / 18446744073709551616.0f;   // 2^-64: the dwe sums and the out-of-window atomics
constexpr float OHK_RW = 4611686018427387904.0f;             // 2^62 = 2^126 / 2^64: the one-hot sums (r_tgt, r_src)
__device__ __forceinline__ unsigned oh2x(unsigned x) {
    const u16x2 k = {0x0080, 0x0080};
    return __builtin_bit_cast(unsigned, (u16x2)__builtin_elementwise_sub_sat(k, __builtin_bit_cast(u16x2, x)));
}

template <int C_>
__global__ __launch_bounds__(Cfg2<C_>::NT, 2) void bwd2_kernel(CgParams p) {
    typedef Cfg2<C_> F;
    typedef Gate<true> GT;
    constexpr int NB = F::NB, NA = F::NA, NWT = F::NWT, HB = NB / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5, t16 = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int C2 = 2 * C_;

    // ---- one-time setup: weights -> LDS, tile buffers zeroed, bias column of the e tiles = 1
    {
        const f32x4* gsrc = reinterpret_cast<const f32x4*>(p.wpack);
        f32x4* ldst = reinterpret_cast<f32x4*>(smem);
        for (int q = tid; q < F::W_BYTES / 16; q += F::NT) ldst[q] = gsrc[q];
        unsigned* z = reinterpret_cast<unsigned*>(smem + F::W_BYTES);
        for (int q = tid; q < 2 * NA * F::BUF / 4; q += F::NT) z[q] = 0u;
    }
    __syncthreads();
    if (tid < 2 * NA * 32) {
        bf16_t* e0 = reinterpret_cast<bf16_t*>(smem + F::W_BYTES + (tid >> 5) * F::BUF + F::OFF_ET);
        e0[(tid & 31) * F::EKS + F::G] = 0x3F80;
    }
    const bf16_t* const wl = reinterpret_cast<const bf16_t*>(smem);

    // ---- work distribution: a static, cost-balanced node range per workgroup (Walk)
    Walk wk;
    {
        const int N = (int)p.N;
        // cost in front of node n: the caller's prefix (mdl_cgconv_balance: far sources cost more) or edges + nodes
        const int32_t* const key = p.balance;
        auto cost_at = [&](int n) -> int64_t { return key ? (int64_t)key[n] : (int64_t)p.rowptr[n] + n; };
        auto bound = [&](int64_t b) { return key ? wave_lower_bound_key(key, N, b, lane) : wave_lower_bound(p.rowptr, N, b, lane); };
        const int64_t Et = cost_at(N);
        const int W = (int)gridDim.x, wi = (int)blockIdx.x;
        const int na = (wi == 0) ? 0 : min(bound(Et * wi / W), N);
        const int nb = (wi == W - 1) ? N : min(bound(Et * (wi + 1) / W), N);
        wk.init(p, na, nb);
    }
    __syncthreads();

    if (wv < NA) {
        // ======================================= producer waves: phase A =======================================
        const int gw = blockIdx.x * NA + wv;
        (void)gw;
        TDECL;
        bf16x8 idf[2];
        {
            const bool mine = ((i >> 3) & 1) == h;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 v = {0u, 0u, 0u, 0u};
                const unsigned one = (mine && (i >> 4) == ks) ? (0x3F80u << (16 * (i & 1))) : 0u;
                const int d = (i & 7) >> 1;
                v[0] = d == 0 ? one : 0u;
                v[1] = d == 1 ? one : 0u;
                v[2] = d == 2 ? one : 0u;
                v[3] = d == 3 ? one : 0u;
                idf[ks] = __builtin_bit_cast(bf16x8, v);
            }
        }
        bool rh0, rh1, rh2, rh3;
        Tile m0 = take<NA>(p, wk, wv, rh0);
        Tile m1 = take<NA>(p, wk, wv, rh1);
        Tile m2 = take<NA>(p, wk, wv, rh2);
        Tile m3 = m2;
        rh3 = rh2;
        Idx id0, id1, id2;
        id0.load(p, m0, i);
        id1.load(p, m1, i);
        id2 = id1;
        EWords<bf16_t, F::G, 2> ew;
        ew.prefetch(p, lane, m0.eb, 32, 0);
        Gathers<C_> ga;
        ga.load(p, id0, h);
        for (int t = 0;; ++t) {
            const bool have = rh0;
            TMARK(0);
            if (have) {
                m3 = take<NA>(p, wk, wv, rh3);
                char* const mybuf = smem + F::W_BYTES + ((t & 1) * NA + wv) * F::BUF;
                bf16_t* const et = reinterpret_cast<bf16_t*>(mybuf + F::OFF_ET);
                if (m0.valid) {
                    const int nv = m0.nv();
                    const bool valid_i = i < nv;
                    const int wb = max(m0.n0 - F::WOFF, 0);
                    const unsigned my_ss = (unsigned)(id0.src - wb);
                    const bool in_win = valid_i && my_ss < (unsigned)(32 * NWT);
                    const bool oob = valid_i && !in_win;
                    ew.commit(et, F::EKS, lane);
                    // two halfwords per edge slot for the reducers' one-hot operands; lanes h = 0 write the target slot, h = 1 the
                    // window slot (both halves hold the indices of edge slot i)
                    reinterpret_cast<unsigned short*>(mybuf + (h ? F::OFF_SSL : F::OFF_TSL))[i] =
                        h ? (in_win ? (unsigned short)(my_ss << OHK_SH) : (unsigned short)0xffff)
                          : (valid_i ? (unsigned short)((id0.tgt - m0.n0) << OHK_SH) : (unsigned short)0xffff);
                    // out-of-window edges: their by-source sums leave from HERE (below, after the gate): a lane owns an edge, so
                    // ONE pass of packed atomics serves every such edge of the tile at once, whatever their number — the
                    // reducers (lane = column) would walk them one by one through the dpre tile (measured: 79 of 625 us)
                    const bool any_oob = __any(oob);
                    // which 32-row blocks of the window this tile's sources touch: the reducers skip the others
                    unsigned touched = 0;
#pragma unroll
                    for (int mt = 0; mt < NWT; ++mt) touched |= __any(in_win && (my_ss >> 5) == (unsigned)mt) ? (1u << mt) : 0u;
                    if (lane == 0) {
                        int* meta = reinterpret_cast<int*>(mybuf + F::OFF_META);
                        meta[0] = m0.n0;
                        meta[1] = m0.n1;
                        meta[2] = 1 | (nv << 8);
                        meta[3] = (int)touched;
                    }
                    wave_lds_fence();
                    TMARK(1);
                    id2.load(p, m2, i);
                    ew.prefetch(p, lane, m1.eb, 32, 0);
                    TMARK(2);

                    f32x16 acc[NB], dmv[HB];
                    const int deg = ga.rp1 - ga.rp0;
                    const float sc = valid_i ? ((p.aggr == MDL_MEAN) ? OHK_UP / (float)max(deg, 1) : OHK_UP) : 0.0f;
                    char* const dpt = mybuf + F::OFF_DP + i * 8;
                    bf16x8 zf[F::KE / 16];
#pragma unroll
                    for (int k = 0; k < F::KE / 16; ++k) zf[k] = ld_frag(et, i, F::EKS, 16 * k, h);
                    auto mfma_pair = [&](int bc) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) { acc[bc][r] = 0.0f; acc[HB + bc][r] = 0.0f; dmv[bc][r] = 0.0f; }
#pragma unroll
                        for (int k = 0; k < F::KE / 16; ++k)
#pragma unroll
                            for (int u = 0; u < 2; ++u) {
                                const int b = bc + HB * u;
                                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ld_frag(wl, 32 * b + i, F::WS, 16 * k, h), zf[k], acc[b], 0, 0, 0);
                            }
#pragma unroll
                        for (int f = 0; f < F::NKX; ++f)
#pragma unroll
                            for (int u = 0; u < 2; ++u) {
                                const int b = bc + HB * u;
                                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ld_frag(wl, 32 * b + i, F::WS, F::KE + 16 * f, h), ga.t[f], acc[b], 0, 0, 0);
                            }
#pragma unroll
                        for (int f = 0; f < F::NKX; ++f)
#pragma unroll
                            for (int u = 0; u < 2; ++u) {
                                const int b = bc + HB * u;
                                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ld_frag(wl, 32 * b + i, F::WS, F::KE + C_ + 16 * f, h), ga.s[f], acc[b], 0, 0, 0);
                            }
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks)
                            dmv[bc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(idf[ks], ga.g[bc][ks], dmv[bc], 0, 0, 0);
                    };
                    auto gate_pair = [&](int bc) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float sf, sp_u, ss;
                            GT::deriv2(acc[bc][r], acc[HB + bc][r], sf, sp_u, ss);
                            const float tt = (dmv[bc][r] * sc) * sf;
                            acc[bc][r] = fmaf(-tt, sf, tt) * sp_u;           // the ln2 of the softplus is applied by the reducers
                            acc[HB + bc][r] = tt * ss;
                        }
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int b = bc + HB * u;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const u32x2 v = {pk_bf16(acc[b][4 * q], acc[b][4 * q + 1]), pk_bf16(acc[b][4 * q + 2], acc[b][4 * q + 3])};
                                *reinterpret_cast<u32x2*>(dpt + (8 * b + 2 * q + h) * F::DCS) = v;
                            }
                        }
                    };
#pragma unroll
                    for (int bc = 0; bc < HB; ++bc) {
                        mfma_pair(bc);
                        if (bc == HB - 1) ga.load(p, id1, h);      // the gathers of my next tile reuse the consumed fragment registers
                        gate_pair(bc);
                        if (any_oob) {
                            // registers 4q .. 4q+3 of block b = columns 32 b + 8 q + 4 h + (0..3) of this lane's edge: two
                            // packed pairs per quad; the f blocks carry the ln2 the reducers apply to everything else
                            if (oob) {
                                typedef __bf16 __attribute__((ext_vector_type(2))) bf2v;
                                typedef __attribute__((address_space(1))) bf2v* gptr_t;
                                bf16_t* dst = reinterpret_cast<bf16_t*>(p.r_src) + (int64_t)id0.src * C2 + 4 * h;
#pragma unroll
                                for (int u = 0; u < 2; ++u) {
                                    const int bb = bc + HB * u;
                                    const float sc2 = (u == 0 ? GT::M_SCALE : 1.0f) * OHK_DOWN;
#pragma unroll
                                    for (int q = 0; q < 4; ++q)
#pragma unroll
                                        for (int k2 = 0; k2 < 2; ++k2) {
                                            const unsigned pk = pk_bf16(acc[bb][4 * q + 2 * k2] * sc2, acc[bb][4 * q + 2 * k2 + 1] * sc2);
                                            __builtin_amdgcn_global_atomic_fadd_v2bf16((gptr_t)(dst + 32 * bb + 8 * q + 2 * k2), __builtin_bit_cast(bf2v, pk));
                                        }
                                }
                            }
                        }
                    }
                } else if (lane == 0) {
                    reinterpret_cast<int*>(mybuf + F::OFF_META)[2] = 0;
                }
            }
            TMARK(3);
            // the reducers do not walk the tile sequence (four Walk::next per round, 630 cycles of their critical path):
            // whether round t + 1 exists travels in the header of tile 0 of the set they reduce in round t + 1
            if (have && wv == 0 && lane == 0)
                reinterpret_cast<int*>(smem + F::W_BYTES + ((t & 1) * NA) * F::BUF + F::OFF_META)[6] = rh1 ? 1 : 0;
            lds_barrier();
            TMARK(4);
            TTILE();
            if (!have) break;
            m0 = m1; m1 = m2; m2 = m3; rh0 = rh1; rh1 = rh2; rh2 = rh3;
            id0 = id1; id1 = id2;
        }
        TFLUSH(16);
        return;
    }

    // ========================================= reducer waves: phase B =========================================
    const int cb = wv - NA;                              // gate column block [32 cb, 32 cb + 32)
    const int gw = (blockIdx.x == 0 && cb == 0) ? 0 : 1000000;   // (timing builds: reducer 0 of workgroup 0 reports)
    (void)gw;
    TDECL;
    const int col = 32 * cb + i;
    const float fscale0 = (cb < HB) ? GT::M_SCALE : 1.0f; // dpre of the f columns lacks the ln2 of the base-2 softplus
    const float fscale = fscale0 * OHK_RW, escale = fscale0 * OHK_DOWN;   // (one-hot sums / dwe sums: see oh2x)
    f32x16 Racc, Wacc[NWT], dwe[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        Racc[r] = 0.0f; dwe[0][r] = 0.0f; dwe[1][r] = 0.0f;
#pragma unroll
        for (int mt = 0; mt < NWT; ++mt) Wacc[mt][r] = 0.0f;
    }
    int cn0 = -1, cn1 = 0, cwb = 0;                      // current group [cn0, cn1), first row of the window the W blocks hold
    typedef __attribute__((address_space(1))) char* gbytes_t;
    const int odd = i & 1;
    // Both flushes write two rows per instruction: the lanes of a pair exchange one value, the even lane takes columns
    // (c, c + 1) of row a, the odd lane those of row a + 1; uniform base + 32-bit byte offset (the scalar-base form of the
    // instruction: no 64-bit address arithmetic per row).  The accumulators were last written by MFMAs inside an asm
    // statement: the wait states for the reads are spelled out.
    auto flush_r = [&]() {
        asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" : "+v"(Racc));
        const gbytes_t rt = (gbytes_t)p.r_tgt;
        const unsigned off0 = ((unsigned)(cn0 + 4 * h + odd) * C2 + (unsigned)(col & ~1)) * 2u;
        const int nrow = cn1 - cn0 - 4 * h - odd;
        if (cn1 - cn0 == 32) {                            // a full group (all but a workgroup's last): no per-row guards
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float va = Racc[r] * fscale, vb = Racc[r + 1] * fscale;
                const float send = odd ? va : vb;
                const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, false));
                const unsigned pk = pk_bf16(odd ? recv : va, odd ? vb : recv);
                *reinterpret_cast<__attribute__((address_space(1))) unsigned*>(rt + (off0 + (unsigned)(d_row(r, 0) * C2 * 2))) = pk;
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float va = Racc[r] * fscale, vb = Racc[r + 1] * fscale;
            const float send = odd ? va : vb;
            const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, false));
            const unsigned pk = pk_bf16(odd ? recv : va, odd ? vb : recv);
            if (d_row(r, 0) < nrow)
                *reinterpret_cast<__attribute__((address_space(1))) unsigned*>(rt + (off0 + (unsigned)(d_row(r, 0) * C2 * 2))) = pk;
        }
    };
    // by-source sums of one 32-row block in bf16 (packed atomics); rows past the last node are skipped
    auto flush_w = [&](f32x16& W, int row0) {
        asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" : "+v"(W));
        typedef __bf16 __attribute__((ext_vector_type(2))) bf2v;
        typedef __attribute__((address_space(1))) bf2v* gptr_t;
        const gbytes_t rs = (gbytes_t)p.r_src;
        const int grow0 = row0 + 4 * h + odd;
        const unsigned off0 = ((unsigned)grow0 * C2 + (unsigned)(col & ~1)) * 2u;
        const int nleft = p.N - grow0;
        if (row0 + 32 <= (int)p.N) {                      // the block lies inside the node array: no per-row guards
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float va = W[r] * fscale, vb = W[r + 1] * fscale;
                const float send = odd ? va : vb;
                const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, false));
                const unsigned pk = pk_bf16(odd ? recv : va, odd ? vb : recv);
                __builtin_amdgcn_global_atomic_fadd_v2bf16((gptr_t)(rs + (off0 + (unsigned)(d_row(r, 0) * C2 * 2))), __builtin_bit_cast(bf2v, pk));
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float va = W[r] * fscale, vb = W[r + 1] * fscale;
            const float send = odd ? va : vb;
            const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, false));
            const unsigned pk = pk_bf16(odd ? recv : va, odd ? vb : recv);
            if (d_row(r, 0) < nleft)
                __builtin_amdgcn_global_atomic_fadd_v2bf16((gptr_t)(rs + (off0 + (unsigned)(d_row(r, 0) * C2 * 2))), __builtin_bit_cast(bf2v, pk));
        }
    };
    auto zero16 = [](f32x16& A) {
#pragma unroll
        for (int r = 0; r < 16; ++r) A[r] = 0.0f;
    };
    const unsigned rsplat = (unsigned)(i << OHK_SH) * 0x00010001u;

    // operands a tile step starts with (k-major dpre fragments of my column block, slot halfwords): requested one tile ahead
    bf16x8 dpf[2];
    u32x2 tq[2][2], sq[2][2];
    auto request = [&](const char* bj) {
        const char* a = bj + F::OFF_DP + (8 * cb + 4 * (i >> 4) + (t16 & 3)) * F::DCS + (4 * h + (t16 >> 2)) * 8;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(a + 128 * ks));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(a + 128 * ks + 64));
            dpf[ks] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
        // k-slot q of k-step ks is edge slot 16 ks + 8 (q >> 2) + 4 h + (q & 3): halfword pairs = dwords 8 ks + 4 g + 2 h + (0, 1)
        const u32x2* tw = reinterpret_cast<const u32x2*>(bj + F::OFF_TSL) + h;
        const u32x2* sw = reinterpret_cast<const u32x2*>(bj + F::OFF_SSL) + h;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            tq[ks][0] = tw[4 * ks]; tq[ks][1] = tw[4 * ks + 2];
            sq[ks][0] = sw[4 * ks]; sq[ks][1] = sw[4 * ks + 2];
        }
    };

    auto tile_step = [&](const char* bj, int jn0, int jn1, int jfl, unsigned touched, const char* bnext) {
        const bool valid = (jfl & 1) != 0;
        const bool act = valid && ((jfl >> 8) & 0xff) != 0;
        const bool newg = valid && jn0 != cn0;
        TMARK(0);
        if (newg) {
            // ROLLING window: consecutive groups of a workgroup advance by 32 nodes, so only the rows that leave the window are
            // flushed (one 32-row block per group instead of all NWT) and the other blocks move down by one
            const int nwb = max(jn0 - F::WOFF, 0);
            if (cn0 >= 0) {
                TMARK(7);
                flush_r();
                TMARK(8);
                if (act && nwb == cwb + 32) {
                    flush_w(Wacc[0], cwb);
                    TMARK(9);
#pragma unroll
                    for (int mt = 0; mt + 1 < NWT; ++mt) Wacc[mt] = Wacc[mt + 1];
                    zero16(Wacc[NWT - 1]);
                    TMARK(10);
                } else if (!act || nwb != cwb) {
#pragma unroll
                    for (int mt = 0; mt < NWT; ++mt) {
                        flush_w(Wacc[mt], cwb + 32 * mt);
                        zero16(Wacc[mt]);
                    }
                }
            }
            zero16(Racc);
            cwb = nwb;
        }
        if (valid && !act) {
            bf16_t* rt = static_cast<bf16_t*>(p.r_tgt);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = jn0 + d_row(r, h);
                if (n < jn1) rt[(int64_t)n * C2 + col] = 0;
            }
        }
        cn0 = valid ? (act ? jn0 : -1) : cn0;
        cn1 = valid ? jn1 : cn1;
        TMARK(1);
        if (!act) {
            request(bnext);
            return;
        }
        // One asm statement per accumulator group (by-target sums, each window block, dwe): the one-hot arithmetic of the next
        // group issues while the matrix core works on the previous one, and a window block none of the tile's sources falls
        // into costs nothing (on the bench batch a tile touches 2.2 blocks on average, whatever the window size).
        // (one MFMA per statement, the one-hot arithmetic of the NEXT k-step between them: the second MFMA of a group needs the
        // first one's result, and the 12 packed instructions of a fragment cover its 32 cycles)
        unsigned xs[2][4];
        const bf16x8 d0 = dpf[0], d1 = dpf[1];
        {
            const u32x2 t0 = tq[0][0], t1 = tq[0][1];
            const bf16x8 tf0 = __builtin_bit_cast(bf16x8, u32x4{oh2x(t0[0] ^ rsplat), oh2x(t0[1] ^ rsplat), oh2x(t1[0] ^ rsplat), oh2x(t1[1] ^ rsplat)});
            asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %[R], %[t0], %[d0], %[R]" : [R] "+v"(Racc) : [t0] "v"(tf0), [d0] "v"(d0));
            const u32x2 u0 = tq[1][0], u1 = tq[1][1];
            const bf16x8 tf1 = __builtin_bit_cast(bf16x8, u32x4{oh2x(u0[0] ^ rsplat), oh2x(u0[1] ^ rsplat), oh2x(u1[0] ^ rsplat), oh2x(u1[1] ^ rsplat)});
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const u32x2 s0 = sq[ks][0], s1 = sq[ks][1];
                xs[ks][0] = s0[0] ^ rsplat; xs[ks][1] = s0[1] ^ rsplat; xs[ks][2] = s1[0] ^ rsplat; xs[ks][3] = s1[1] ^ rsplat;
            }
            asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %[R], %[t1], %[d1], %[R]\n\ts_nop 3" : [R] "+v"(Racc) : [t1] "v"(tf1), [d1] "v"(d1));
        }
        TMARK(2);
        // the e-tile fragments of this tile and the operands of the next one travel while the window blocks are worked on
        bf16x8 ebf[2][2];
        {
            const bf16_t* const etj = reinterpret_cast<const bf16_t*>(bj + F::OFF_ET);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16_t* base = etj + (16 * ks + 4 * h + (t16 >> 2)) * F::EKS + nt * 32 + (i & 16) + 4 * (t16 & 3);
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(base));
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(base + 8 * F::EKS));
                    ebf[nt][ks] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
        }
        request(bnext);
#pragma unroll
        for (int mt = 0; mt < NWT; ++mt) {
            if (touched & (1u << mt)) {
                const unsigned m = (unsigned)((32 * mt) << OHK_SH) * 0x00010001u;      // row 32 mt + i = i | 32 mt: the xor splits
                const bf16x8 w0 = __builtin_bit_cast(bf16x8, u32x4{oh2x(xs[0][0] ^ m), oh2x(xs[0][1] ^ m), oh2x(xs[0][2] ^ m), oh2x(xs[0][3] ^ m)});
                asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %[W], %[w0], %[d0], %[W]" : [W] "+v"(Wacc[mt]) : [w0] "v"(w0), [d0] "v"(d0));
                const bf16x8 w1 = __builtin_bit_cast(bf16x8, u32x4{oh2x(xs[1][0] ^ m), oh2x(xs[1][1] ^ m), oh2x(xs[1][2] ^ m), oh2x(xs[1][3] ^ m)});
                asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %[W], %[w1], %[d1], %[W]\n\ts_nop 3" : [W] "+v"(Wacc[mt]) : [w1] "v"(w1), [d1] "v"(d1));
            }
        }
        TMARK(3);
        asm volatile(
            "v_mfma_f32_32x32x16_bf16 %[E0], %[d0], %[e00], %[E0]\n\t"
            "v_mfma_f32_32x32x16_bf16 %[E1], %[d0], %[e10], %[E1]\n\t"
            "v_mfma_f32_32x32x16_bf16 %[E0], %[d1], %[e01], %[E0]\n\t"
            "v_mfma_f32_32x32x16_bf16 %[E1], %[d1], %[e11], %[E1]\n\t"
            "s_nop 7"
            : [E0] "+v"(dwe[0]), [E1] "+v"(dwe[1])
            : [d0] "v"(d0), [d1] "v"(d1), [e00] "v"(ebf[0][0]), [e01] "v"(ebf[0][1]), [e10] "v"(ebf[1][0]), [e11] "v"(ebf[1][1]));
        TMARK(4);
    };

    {
        // the reducers take the first rounds of the tile sequence like the producers (scalar work only): whether round 0 exists
        bool rh0, rh1, rh2;
        (void)take<NA>(p, wk, 0, rh0);
        (void)take<NA>(p, wk, 0, rh1);
        (void)take<NA>(p, wk, 0, rh2);
        bool have = rh0;                                  // (later rounds: from the header, below)
        for (int t = 0;; ++t) {
            if (t > 0) {
                const char* set = smem + F::W_BYTES + (((t - 1) & 1) * NA) * F::BUF;
                have = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(set + F::OFF_META)[6]) != 0;
                // the headers of the round's four tiles in one read: lane j holds tile j's
                TMARK(11);
                const i32x4 hd = *reinterpret_cast<const i32x4*>(set + (lane & (NA - 1)) * F::BUF + F::OFF_META);
                request(set);
                TMARK(12);
#pragma unroll 1
                // (the last tile of a round requests operands too — tile 0 of the set again, unused: with ONE code path the wait
                // in front of the dwe product counts the requests in flight (lgkmcnt(8)) instead of draining them (lgkmcnt(0)
                // at the join of the two paths): K3 483 -> 476 us)
                for (int j = 0; j < NA; ++j)
                    tile_step(set + j * F::BUF, __builtin_amdgcn_readlane(hd[0], j), __builtin_amdgcn_readlane(hd[1], j),
                              __builtin_amdgcn_readlane(hd[2], j), (unsigned)__builtin_amdgcn_readlane(hd[3], j),
                              set + ((j + 1) & (NA - 1)) * F::BUF);
            }
            TMARK(5);
            lds_barrier();
            TMARK(6);
            TTILE();
            if (!have) break;
        }
    }
    if (cn0 >= 0) {
        flush_r();
#pragma unroll
        for (int mt = 0; mt < NWT; ++mt) flush_w(Wacc[mt], cwb + 32 * mt);
    }
    TFLUSH(32);
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" : "+v"(dwe[0]), "+v"(dwe[1]));
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int gcol = nt * 32 + i;
        if (gcol < F::G) {
#pragma unroll
            for (int r = 0; r < 16; ++r) unsafeAtomicAdd(p.dwe + (int64_t)(32 * cb + d_row(r, h)) * p.GP + gcol, dwe[nt][r] * escale);
        } else if (gcol == F::G && p.db) {
            // column G of the e tiles is the constant 1: its dwe column is the bias gradient
#pragma unroll
            for (int r = 0; r < 16; ++r) unsafeAtomicAdd(p.db + 32 * cb + d_row(r, h), dwe[nt][r] * escale);
        }
    }
}

}  // namespace ep
