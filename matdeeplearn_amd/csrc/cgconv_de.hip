// cgconv_de.hip — K3d: the CGConv gradient with respect to the EDGE FEATURES, the gradient the backward edge pass (cgconv_bwd.inc,
// cgconv_ep2.inc) does not form.  No reference counterpart as a kernel: upstream torch_geometric.nn.CGConv gets it from autograd
// through the materialised z = [x_i | x_j | e_ij] (the reference model never asks for it, cgcnn.py:136-145).
//
// With pre_f = W_f z + b_f, pre_s = W_s z + b_s, m = sigmoid(pre_f) softplus(pre_s), dm_e = grad_out[tgt(e)] (/ deg for mean):
//   dpre_f = dm softplus(pre_s) sigmoid(pre_f)(1 - sigmoid(pre_f))        dpre_s = dm sigmoid(pre_f) sigmoid(pre_s)
//   de[e, :] = dpre_f[e, :] W_f[:, 2C:] + dpre_s[e, :] W_s[:, 2C:]                                              [E, G]
//
// One kernel, two epilogues (an argument, not an environment switch):
//   general   de [E, G] is stored in the storage dtype (CSR edge order)
//   distance  the edge features are a Gaussian expansion e[e, g] = exp(coeff (d_e - mu_g)^2) of ONE scalar per edge, so
//             dL/dd_e = scale * sum_g de[e, g] * 2 coeff (d_e - mu_g) e[e, g]  is added into dd [E] fp32; de never leaves the
//             registers.  Every edge belongs to one wave and one lane does its read-modify-write: no atomics, the same bits on
//             every run, and the layers of a model add into one buffer launch after launch.
//
// Per wave: an edge-balanced node range (NodeRange, as the per-wave K3), walked in tiles of 32 consecutive CSR slots.  Per tile
// and 32-channel slice the pre-activations are recomputed by the K2 / K3 tile code (pre_tile: e tile in the wave's LDS, x rows
// gathered into A fragments, packed weights from LDS where they fit), grad_out is gathered per (edge, channel), the gate
// derivative (Gate<>, the backward's) turns the accumulators into dpre, and dpre goes through a 32 x 32 LDS tile — the
// accumulator layout has lane = channel, the second product needs lane = edge — into
//   de_tile (32 x G) += dpre_tile (32 x 32) * W_e (32 x G)            once for the f part, once for the s part
// whose B fragments are columns of the same packed weights (fp32: read in place; bf16: a [G][2Cp] transposed copy per workgroup,
// so that a fragment is one 16-byte LDS read).  fp32 storage: v_mfma_f32_32x32x2_f32 throughout (exact fp32 products); bf16
// storage: v_mfma_f32_32x32x16_bf16, dpre rounded to bf16 for the second product.  A layer in the split-bf16 mode
// (MDL_SPLIT_BF16) is served by the exact fp32 form on plainly packed weights.
// Shapes: every (C, G) mdl_cgconv_wpack_bytes accepts (run-time dimensions; weights that do not fit the LDS are read from global
// memory).  Allocated for one wave per SIMD like cgconv_bwd_kernel: 4 waves per workgroup, one workgroup per CU.
#include "cgconv_tiles.inc"

namespace mdl {
namespace {

constexpr int DE_LDS_CAP = 160 * 1024;
constexpr int DE_WAVES = 4;
constexpr int DE_RANGE_EDGES = 128;        // edges per node range below which the launch shrinks instead (BWD_RANGE_EDGES of K3)
constexpr int DE_HDR = 32 + 128 + 32 + 16; // the per-wave index area setup_wave lays out behind the e tile

struct DeParams {
    void* de;               // general: [E, G] storage dtype
    const float* dnorm;     // distance: [E] the expanded scalar per edge (CSR order)
    const float* offsets;   // distance: [G] centres
    float* dd;              // distance: [E] fp32, added into
    float coeff2;           // distance: 2 * coeff
    float scale;            // distance: factor of the sum (chain rule of the caller's normalisation)
    int dist;               // 0 general, 1 distance
    int x0;                 // byte offset of this kernel's per-wave area inside a wave's LDS region
    int we_off;             // bf16: byte offset of the transposed edge-weight copy in the workgroup's LDS
    int wes;                // bf16: its row stride in elements (2Cp + 8)
};

template <typename T, int VEC, int EW, int WM>
__global__ __launch_bounds__(256, 1) void cgconv_de_kernel(CgParams p, DeParams q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef Mma<T> M;
    typedef Gate<M::FAST> GT;
    typedef Dims<T, 0, 0, EW> D;
    constexpr bool BF = std::is_same<T, bf16_t>::value;
    constexpr int DS = 32 + (BF ? 8 : 1);                  // dpre tile row stride (bf16: odd number of 16-byte slots; fp32: odd dwords)
    const D dm(p);
    WaveCtx<T> w;
    setup_wave<T>(p, dm, smem, WM == 1, w);

    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * DE_WAVES + wave;
    const int total_waves = gridDim.x * DE_WAVES;
    char* const mine = smem + (WM == 1 ? ((p.w_elems * (int)sizeof(T) + 15) & ~15) : 0) + wave * p.wave_lds_bytes + q.x0;
    int* const tg = reinterpret_cast<int*>(mine);                  // target node of every edge slot
    float* const invd = reinterpret_cast<float*>(mine + 128);       // 1 / in-degree of that target (mean), 1 (add), 0 (empty slot)
    float* const dn = reinterpret_cast<float*>(mine + 256);         // distance epilogue: the slot's expanded scalar
    T* const dt = reinterpret_cast<T*>(mine + 384);                 // dpre tile [32 edge slots][DS]
    const bf16_t* const we = reinterpret_cast<const bf16_t*>(smem + q.we_off);
    if constexpr (BF) {
        // transposed copy of the edge-feature columns of the packed weights: we[g][k], k = part * Cp + channel
        bf16_t* const wew = reinterpret_cast<bf16_t*>(smem + q.we_off);
        const bf16_t* const wp = static_cast<const bf16_t*>(p.wpack);
        const int K2 = 2 * dm.Cp;
        for (int t = threadIdx.x; t < 64 * K2; t += blockDim.x) {
            const int g = t / K2, k = t - g * K2;
            wew[g * q.wes + k] = g < dm.KE ? wp[k * dm.WS + g] : (bf16_t)0;
        }
        __syncthreads();
    }

    const T* go = static_cast<const T*>(p.gout);
    const NodeRange R(p, __builtin_amdgcn_readfirstlane(gw), total_waves, lane);
    const int e0 = p.rowptr[R.na], e1 = p.rowptr[R.nb];
    const int gnt = (dm.G + 31) >> 5;                              // 32-column tiles of G (1 or 2: G <= 64)
    const float unscale = 1.0f / GT::W_SCALE;                      // the packed weights carry the gate's pre-scale
    XFrags<T, 0, VEC> xf;                                          // (run-time channel count: pre_tile gathers the x rows itself)
    xf.t[0] = M::zero();
    xf.s[0] = M::zero();

    for (int eb = e0; eb < e1; eb += 32) {
        const int nv = min(32, e1 - eb);
        TileIdx idx;
        idx.template load<false, false>(p, eb, e1, i, R.na);
        wave_lds_fence();                                          // the previous tile's LDS reads are done
        stage_e_tile<T, EW>(p, dm, w, lane, eb, nv, 0);
        if (h == 0) {
            const int dg = p.rowptr[idx.tgt + 1] - p.rowptr[idx.tgt];
            tg[i] = idx.tgt;
            invd[i] = i < nv ? (p.aggr == MDL_MEAN ? 1.0f / (float)max(dg, 1) : 1.0f) : 0.0f;
            dn[i] = q.dist ? q.dnorm[min(eb + i, e1 - 1)] : 0.0f;
        }
        wave_lds_fence();

        f32x16 dacc[2];
#pragma unroll
        for (int gt = 0; gt < 2; ++gt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dacc[gt][r] = 0.0f;

        for (int s = 0; s < p.NS; ++s) {
            const int ch = s * 32 + i, chc = min(ch, dm.C - 1);
            const float bf = p.bias_col ? 0.0f : p.bpack[ch], bs = p.bias_col ? 0.0f : p.bpack[dm.Cp + ch];
            f32x16 accf, accs;
#pragma unroll
            for (int r = 0; r < 16; ++r) { accf[r] = bf; accs[r] = bs; }
            pre_tile<T, 0, VEC, WM>(p, dm, w, lane, s, idx.tgt, idx.src, xf, accf, accs);
            // dm[edge slot][ch] = grad_out[tgt][ch] / deg (an exact 0 for empty slots and padded channels), then the gate
            // derivative -> dpre in place
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = d_row(r, h);
                const float gv = Elem<T>::ld(go + (int64_t)tg[row] * dm.C + chc);
                const float dmv = ch < dm.C ? gv * invd[row] : 0.0f;
                float sf, sp_u, ss;
                GT::deriv(accf[r], accs[r], sf, sp_u, ss);
                const float t = dmv * sf;
                accf[r] = (t * GT::M_SCALE) * (1.0f - sf) * sp_u;
                accs[r] = t * ss;
            }
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                wave_lds_fence();                                  // the previous part's fragment reads are done
#pragma unroll
                for (int r = 0; r < 16; ++r) Elem<T>::st(dt + d_row(r, h) * DS + i, part ? accs[r] : accf[r]);
                wave_lds_fence();
                const int krow = part * dm.Cp + s * 32;            // first weight row (= k of the transposed copy) of this block
#pragma unroll
                for (int gt = 0; gt < 2; ++gt) {
                    if (gt < gnt) {
                        const int gc = min(gt * 32 + i, dm.KE - 1);
#pragma unroll
                        for (int k0 = 0; k0 < 32; k0 += M::KSTEP) {
                            const typename M::frag_t a = ld_frag(dt, i, DS, k0, h);
                            typename M::frag_t b;
                            if constexpr (BF) b = *reinterpret_cast<const bf16x8*>(we + gc * q.wes + krow + k0 + 8 * h);
                            else b = w.wbase[(krow + k0 + h) * dm.WS + gc];
                            dacc[gt] = M::mma(a, b, dacc[gt]);
                        }
                    }
                }
            }
        }

        // epilogue: dacc[gt] = de[edge slot d_row(r, h)][g = 32 gt + i] * W_SCALE
        if (!q.dist) {
            T* de = static_cast<T*>(q.de);
#pragma unroll
            for (int gt = 0; gt < 2; ++gt) {
                const int g = gt * 32 + i;
                if (gt < gnt && g < dm.G) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = d_row(r, h);
                        if (row < nv) Elem<T>::st(de + (int64_t)(eb + row) * dm.G + g, dacc[gt][r] * unscale);
                    }
                }
            }
        } else {
            float part[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) part[r] = 0.0f;
#pragma unroll
            for (int gt = 0; gt < 2; ++gt) {
                const int g = gt * 32 + i;
                if (gt < gnt && g < dm.G) {
                    const float mu = q.offsets[g];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = d_row(r, h);
                        part[r] += dacc[gt][r] * ((dn[row] - mu) * Elem<T>::ld(w.et + row * dm.EKS + g));
                    }
                }
            }
            // sum over the 32 lanes (= features) of a half-wave; afterwards lane i < 16 of half h owns edge slot d_row(i, h)
            float own = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = part[r];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
                own = (i == r) ? v : own;
            }
            const int row = d_row(i & 15, h);
            if (i < 16 && row < nv) q.dd[eb + row] += (q.scale * q.coeff2 * unscale) * own;
        }
    }
}

template <typename T>
int de_launch(CgParams& p, DeParams& q, int dtype, hipStream_t st, const char* name) {
    const CgDims d = cg_dims(p.C, p.G, dtype);
    p.Cp = d.Cp; p.KE = d.KE; p.KT = d.KT; p.WS = d.WS; p.EKS = d.EKS; p.NS = d.NS; p.GP = d.GP;
    p.w_elems = 2 * d.Cp * d.WS;
    p.w_slice = 0;
    p.bias_col = (p.G % 16) != 0;
    const bool word4 = (p.G * sizeof(T)) % 4 == 0 && (reinterpret_cast<uintptr_t>(p.ea) % 4) == 0;
    const int EW = word4 ? (int)(4 / sizeof(T)) : 1;
    p.GW = p.G / EW;
    p.gw_inv = (unsigned)((0x100000000ull + p.GW - 1) / p.GW);
    int vec = 1;
    if (sizeof(T) == 2 && p.C % 8 == 0 && reinterpret_cast<uintptr_t>(p.x) % 16 == 0) vec = 8;

    constexpr bool BF = sizeof(T) == 2;
    const int et_bytes = (32 * d.EKS * (int)sizeof(T) + 15) & ~15;
    const int dt_bytes = (32 * (32 + (BF ? 8 : 1)) * (int)sizeof(T) + 15) & ~15;
    q.x0 = et_bytes + DE_HDR;
    p.wave_lds_bytes = q.x0 + 384 + dt_bytes;
    q.wes = 2 * d.Cp + 8;
    const int we_bytes = BF ? 64 * q.wes * 2 : 0;
    const int w_bytes = (p.w_elems * (int)sizeof(T) + 15) & ~15;
    const bool w_lds = w_bytes + DE_WAVES * p.wave_lds_bytes + we_bytes <= DE_LDS_CAP;
    q.we_off = (w_lds ? w_bytes : 0) + DE_WAVES * p.wave_lds_bytes;
    const int lds = q.we_off + we_bytes;
    if (lds > DE_LDS_CAP) { set_error("%s: C=%d G=%d needs %d bytes of LDS", name, p.C, p.G, lds); return MDL_E_UNSUPP; }

    const int64_t ranges = std::max<int64_t>(1, std::min<int64_t>(cdiv(p.E, DE_RANGE_EDGES), p.N));
    const int64_t grid = std::min<int64_t>(cdiv(ranges, DE_WAVES), 256);

#define MDL_DE_LAUNCH(VEC_, EW_, WM_)                                                                                      \
    do {                                                                                                                   \
        auto kf = cgconv_de_kernel<T, VEC_, EW_, WM_>;                                                                     \
        hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(kf), lds);                                        \
        if (e != hipSuccess) { set_error("%s: LDS attribute (%d B): %s", name, lds, hipGetErrorString(e)); return MDL_E_LAUNCH; } \
        hipLaunchKernelGGL(kf, dim3((unsigned)grid), dim3(DE_WAVES * 64), lds, st, p, q);                                  \
    } while (0)
#define MDL_DE_BY_WL(VEC_, EW_) do { if (w_lds) MDL_DE_LAUNCH(VEC_, EW_, 1); else MDL_DE_LAUNCH(VEC_, EW_, 0); } while (0)
    if constexpr (BF) {
        if (vec == 8 && EW == 2) MDL_DE_BY_WL(8, 2);
        else if (vec == 8) MDL_DE_BY_WL(8, 1);
        else if (EW == 2) MDL_DE_BY_WL(1, 2);
        else MDL_DE_BY_WL(1, 1);
    } else {
        MDL_DE_BY_WL(1, 1);
    }
#undef MDL_DE_BY_WL
#undef MDL_DE_LAUNCH
    return check_launch(name);
}

}  // namespace
}  // namespace mdl

extern "C" int mdl_cgconv_bwd_edge(const void* x, const void* edge_attr, const int32_t* rowptr, const int32_t* src, const int32_t* tgt,
                                   const void* wpack, const float* bpack, const void* grad_out, int64_t N, int64_t E, int C, int G,
                                   int aggr, int dtype, void* de, const float* d_norm, const float* offsets, float coeff, float scale,
                                   float* dd, mdlStream_t stream) {
    using namespace mdl;
    const char* name = "mdl_cgconv_bwd_edge";
    MDL_REQUIRE(N >= 0 && E >= 0 && N < (1ll << 31) - 64 && E < (1ll << 31) - 64, MDL_E_ARG, "%s: bad N=%lld E=%lld", name, (long long)N,
                (long long)E);
    MDL_REQUIRE(C >= 1 && C <= 256, MDL_E_UNSUPP, "%s: unsupported channels C=%d (1..256)", name, C);
    MDL_REQUIRE(G >= 1 && G <= 64, MDL_E_UNSUPP, "%s: unsupported edge feature count G=%d (1..64)", name, G);
    MDL_REQUIRE(dtype == MDL_F32 || dtype == MDL_BF16, MDL_E_UNSUPP, "%s: unsupported dtype %d (MDL_SPLIT_BF16 layers: pack the weights plainly)",
                name, dtype);
    MDL_REQUIRE(aggr == MDL_MEAN || aggr == MDL_SUM, MDL_E_UNSUPP, "%s: unsupported aggr %d", name, aggr);
    if (E == 0 || N == 0) return MDL_OK;                  // (no edges: nothing to write, and the per-edge pointers may be null)
    MDL_REQUIRE((de != nullptr) != (dd != nullptr), MDL_E_ARG, "%s: give de (general epilogue) or dd (distance epilogue)", name);
    MDL_REQUIRE(!dd || (d_norm && offsets), MDL_E_ARG, "%s: the distance epilogue needs d_norm and offsets", name);
    MDL_REQUIRE(x && edge_attr && rowptr && src && tgt && wpack && bpack && grad_out, MDL_E_ARG, "%s: null pointer", name);
    MDL_REQUIRE(reinterpret_cast<uintptr_t>(wpack) % 16 == 0, MDL_E_ARG, "%s: wpack must be 16-byte aligned", name);
    CgParams p = {};
    p.x = x; p.ea = edge_attr; p.rowptr = rowptr; p.src = src; p.tgt = tgt; p.wpack = wpack; p.bpack = bpack; p.gout = grad_out;
    p.N = N; p.E = E; p.C = C; p.G = G; p.aggr = aggr;
    DeParams q = {};
    q.de = de; q.dnorm = d_norm; q.offsets = offsets; q.dd = dd; q.coeff2 = 2.0f * coeff; q.scale = scale; q.dist = dd ? 1 : 0;
    if (dtype == MDL_BF16) return de_launch<bf16_t>(p, q, dtype, (hipStream_t)stream, name);
    return de_launch<float>(p, q, dtype, (hipStream_t)stream, name);
}
