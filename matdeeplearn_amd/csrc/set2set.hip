// set2set.hip — the Set2Set readout (torch_geometric.nn.Set2Set with a one-layer LSTM; the reference's pool = "set2set",
// matdeeplearn/models/cgcnn.py:112-119,152) as ONE launch per direction for all processing steps.
//
// Set2Set is independent per graph: for every segment s of rowptr (nodes rowptr[s] .. rowptr[s+1]-1 of x [N, C]), from
// q*_0 = 0, h_0 = c_0 = 0 and for t = 1..T
//     G_t  = W_ih q*_{t-1} + b_ih + W_hh h_{t-1} + b_hh                        (4C, torch's gate order i | f | g | o)
//     c_t  = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g);   q_t = h_t = sigmoid(o) tanh(c_t)
//     e_n  = <x_n, q_t>;  a_n = exp(e_n - max e) / (sum exp(e_n - max e) + 1e-16);  r_t = sum a_n x_n
//     q*_t = [q_t | r_t],      out[s] = q*_T.
//
// Work split.  A workgroup of four waves owns a tile of S2S_GT = 4 graphs for the whole recurrence; the per-graph state (q, r, c,
// the gate vector) lives in LDS.  Each step has two phases:
//   gates      thread j owns row j of [W_ih | W_hh] (4C rows of 3C floats) and forms the row's product with the tile's FOUR state
//              vectors (LDS broadcast reads), so a weight row fetched from L2 serves four graphs.  The weights (4C x 3C floats:
//              196 KB at C = 64, 480 KB at C = 100) do not fit the LDS and are the same for every tile: they stay in L2.
//   attention  wave w owns graph w.  Lanes are split into 64 / LPN node slots of LPN lanes; a slot's lanes hold one row of x as
//              VW-element vectors (16 bytes of fp32, 8 of bf16 when C % 4 == 0; single elements otherwise, two per lane above
//              C = 64).  ONE pass over the graph's rows per step with the running-maximum ("online") form of the softmax: every
//              slot keeps (max, sum, weighted row sum) of the rows it saw, rescaled when its maximum grows, and the slots are
//              merged at the end.  Nothing of a graph is held on chip but that state, so the segment length is unbounded; x is
//              read T times forward (it sits in L2 / MALL between the steps).  When the backward's state is wanted, e_n is parked
//              in a[t, n] during the pass and turned into a_n by a second pass over those N floats.
// The backward walks t = T..1 in the same tile shape:
//   attention  da_n = <dr, x_n> (parked in the caller's [T, N] workspace), s = sum a_n da_n, v = sum a_n da_n x_n in ONE pass;
//              sum_n de_n x_n = v - s r_t because de_n = a_n (da_n - s) and r_t = sum a_n x_n;
//   cell       the LSTM cell's backward per (graph, channel) from the stored activated gates and c; dG_t leaves for the
//              parameter gradients (dense products over the stacked T S rows, formed by the caller);
//   products   [dq*_{t-1} | dh_{t-1}] = [W_ih | W_hh]^T dG_t, thread k owning COLUMN k (coalesced rows of the weights);
//   dx         after the walk, one pass writes dx_n = sum_t a_tn dr_t + a_tn (da_tn - s_t) q_t ONCE in x's dtype (2T scalars per
//              node instead of T read-modify-write passes over a possibly bf16 row); rows outside every segment get exact zeros.
// Every sum has a fixed order and no floating-point atomic appears: the result is bitwise repeatable.
#include <math.h>

#include "mdl_common.h"

namespace mdl {

constexpr int S2S_GT = 4;          // graphs per workgroup = waves per workgroup
constexpr int S2S_THREADS = 256;
constexpr int S2S_MAX_C = 128, S2S_MAX_T = 8;

__device__ __forceinline__ float s2s_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

template <typename T, int VW> struct S2SRow;
template <typename T> struct S2SRow<T, 4> {
    __device__ static __forceinline__ void ld(const T* p, float* v) { VecW<T, 4>::ld(p, v); }
    __device__ static __forceinline__ void st(T* p, const float* v) { VecW<T, 4>::st(p, v); }
};
template <typename T> struct S2SRow<T, 1> {
    __device__ static __forceinline__ void ld(const T* p, float* v) { v[0] = Elem<T>::ld(p); }
    __device__ static __forceinline__ void st(T* p, const float* v) { Elem<T>::st(p, v[0]); }
};

// how a wave's lanes cover the rows of one graph
struct S2SLanes {
    int lc, slot, lpn, npw, nvec;
    __device__ __forceinline__ S2SLanes(int lane, int lpn_log2, int nvec_) {
        lpn = 1 << lpn_log2;
        lc = lane & (lpn - 1);
        slot = lane >> lpn_log2;
        npw = WAVE >> lpn_log2;
        nvec = nvec_;
    }
};

template <int M, int VW>
__device__ __forceinline__ void s2s_load_state(const S2SLanes& L, const float* s_vec, float (&v)[M][VW]) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int iv = L.lc + m * L.lpn;
#pragma unroll
        for (int i = 0; i < VW; ++i) v[m][i] = iv < L.nvec ? s_vec[iv * VW + i] : 0.0f;
    }
}

template <typename T, int VW, int M>
__device__ __forceinline__ void s2s_load_row(const S2SLanes& L, const T* __restrict__ x, int64_t n, int64_t end, int C, float (&v)[M][VW]) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int iv = L.lc + m * L.lpn;
        if (n < end && iv < L.nvec) {
            S2SRow<T, VW>::ld(x + n * C + iv * VW, v[m]);
        } else {
#pragma unroll
            for (int i = 0; i < VW; ++i) v[m][i] = 0.0f;
        }
    }
}

// sum over the lanes of one node slot (all lanes of the wave take part)
__device__ __forceinline__ float s2s_slot_sum(float v, int lpn) {
    for (int o = lpn >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sum over the node slots of the wave (lanes with the same position inside their slot)
__device__ __forceinline__ float s2s_wave_sum(float v, int lpn) {
    for (int o = lpn; o < WAVE; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T, int VW, int M>
__global__ __launch_bounds__(S2S_THREADS) void set2set_fwd_kernel(
    const T* __restrict__ x, const int32_t* __restrict__ rowptr, const float* __restrict__ w_ih, const float* __restrict__ w_hh,
    const float* __restrict__ b_ih, const float* __restrict__ b_hh, float* __restrict__ out, float* __restrict__ sv_gates,
    float* __restrict__ sv_c, float* __restrict__ sv_q, float* __restrict__ sv_r, float* __restrict__ sv_a, int64_t N, int64_t S, int C,
    int steps, int lpn_log2) {
    constexpr int GT = S2S_GT;
    constexpr int U = 8 / M;                 // rows in flight per slot
    extern __shared__ float s2s_lds[];
    float* s_q = s2s_lds;                    // [GT][C]
    float* s_r = s_q + GT * C;               // [GT][C]
    float* s_c = s_r + GT * C;               // [GT][C]
    float* s_g = s_c + GT * C;               // [GT][4C] pre-activation gates
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int64_t s0 = (int64_t)blockIdx.x * GT;
    const int C2 = 2 * C, C4 = 4 * C;
    const S2SLanes L(lane, lpn_log2, C / VW);

    for (int i = tid; i < 3 * GT * C; i += S2S_THREADS) s2s_lds[i] = 0.0f;
    __syncthreads();

    for (int t = 0; t < steps; ++t) {
        // ---- gates: G = b_ih + b_hh + W_ih [q | r] + W_hh q (h = q); q*_0 = h_0 = 0 leaves the biases at t = 0
        for (int j = tid; j < C4; j += S2S_THREADS) {
            float acc[GT];
            const float bias = b_ih[j] + b_hh[j];
#pragma unroll
            for (int g = 0; g < GT; ++g) acc[g] = bias;
            if (t > 0) {
                const float* wi = w_ih + (int64_t)j * C2;
                const float* wh = w_hh + (int64_t)j * C;
                if (VW == 4) {
#pragma unroll 2
                    for (int k = 0; k < C; k += 4) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(wi + k);
                        const f32x4 b = *reinterpret_cast<const f32x4*>(wh + k);
                        const f32x4 c = *reinterpret_cast<const f32x4*>(wi + C + k);
#pragma unroll
                        for (int g = 0; g < GT; ++g) {
                            const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + g * C + k);
                            const f32x4 rv = *reinterpret_cast<const f32x4*>(s_r + g * C + k);
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc[g] = fmaf(c[i], rv[i], fmaf(b[i], qv[i], fmaf(a[i], qv[i], acc[g])));
                        }
                    }
                } else {
#pragma unroll 8
                    for (int k = 0; k < C; ++k) {
                        const float a = wi[k], b = wh[k], c = wi[C + k];
#pragma unroll
                        for (int g = 0; g < GT; ++g)
                            acc[g] = fmaf(c, s_r[g * C + k], fmaf(b, s_q[g * C + k], fmaf(a, s_q[g * C + k], acc[g])));
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < GT; ++g) s_g[g * C4 + j] = acc[g];
        }
        __syncthreads();
        // ---- cell
        for (int idx = tid; idx < GT * C; idx += S2S_THREADS) {
            const int g = idx / C, c = idx - g * C;
            const int64_t s = s0 + g;
            if (s < S) {
                const float gi = s2s_sigmoid(s_g[g * C4 + c]), gf = s2s_sigmoid(s_g[g * C4 + C + c]);
                const float gg = tanhf(s_g[g * C4 + C2 + c]), go = s2s_sigmoid(s_g[g * C4 + 3 * C + c]);
                const float cc = gf * s_c[idx] + gi * gg;
                const float q = go * tanhf(cc);
                s_c[idx] = cc;
                s_q[idx] = q;
                if (sv_gates) {
                    const int64_t row = (int64_t)t * S + s;
                    float* gp = sv_gates + row * C4 + c;
                    gp[0] = gi; gp[C] = gf; gp[C2] = gg; gp[3 * C] = go;
                    sv_c[row * C + c] = cc;
                    sv_q[row * C + c] = q;
                }
            }
        }
        __syncthreads();
        // ---- attention: wave = graph
        for (int g = wave; g < GT; g += S2S_THREADS / WAVE) {
            const int64_t s = s0 + g;
            const int64_t end = s < S ? min((int64_t)rowptr[s + 1], N) : 0, beg = s < S ? max((int64_t)rowptr[s], (int64_t)0) : 0;
            float qv[M][VW], racc[M][VW];
            s2s_load_state<M, VW>(L, s_q + g * C, qv);
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int i = 0; i < VW; ++i) racc[m][i] = 0.0f;
            float mx = -INFINITY, l = 0.0f;
            float* at = sv_a ? sv_a + (int64_t)t * N : nullptr;
            for (int64_t n0 = beg; n0 < end; n0 += (int64_t)L.npw * U) {
                float xv[U][M][VW];
#pragma unroll
                for (int u = 0; u < U; ++u) s2s_load_row<T, VW, M>(L, x, n0 + u * L.npw + L.slot, end, C, xv[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t n = n0 + u * L.npw + L.slot;
                    float e = 0.0f;
#pragma unroll
                    for (int m = 0; m < M; ++m)
#pragma unroll
                        for (int i = 0; i < VW; ++i) e = fmaf(xv[u][m][i], qv[m][i], e);
                    e = s2s_slot_sum(e, L.lpn);
                    if (n < end) {
                        const float mn = fmaxf(mx, e);
                        const float sc = mx == mn ? 1.0f : expf(mx - mn);       // (mx = -inf before the slot's first row: 0)
                        const float p = expf(e - mn);
                        l = fmaf(l, sc, p);
#pragma unroll
                        for (int m = 0; m < M; ++m)
#pragma unroll
                            for (int i = 0; i < VW; ++i) racc[m][i] = fmaf(racc[m][i], sc, p * xv[u][m][i]);
                        mx = mn;
                        if (at && L.lc == 0) at[n] = e;
                    }
                }
            }
            // merge the slots
            float mall = mx;
            for (int o = L.lpn; o < WAVE; o <<= 1) mall = fmaxf(mall, __shfl_xor(mall, o));
            const float sc = mx == -INFINITY ? 0.0f : expf(mx - mall);
            l = s2s_wave_sum(l * sc, L.lpn);
            const float inv = 1.0f / (l + 1e-16f);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const int iv = L.lc + m * L.lpn;
#pragma unroll
                for (int i = 0; i < VW; ++i) {
                    const float r = s2s_wave_sum(racc[m][i] * sc, L.lpn) * inv;
                    if (L.slot == 0 && iv < L.nvec && s < S) {
                        s_r[g * C + iv * VW + i] = r;
                        if (sv_r) sv_r[((int64_t)t * S + s) * C + iv * VW + i] = r;
                    }
                }
            }
            if (at) {                 // e_n -> a_n by the whole wave (the scores were parked by the first lane of every slot)
                __threadfence_block();
                for (int64_t n = beg + lane; n < end; n += WAVE) at[n] = expf(at[n] - mall) * inv;
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < GT * C; idx += S2S_THREADS) {
        const int g = idx / C, c = idx - g * C;
        const int64_t s = s0 + g;
        if (s < S) {
            out[s * C2 + c] = s_q[idx];
            out[s * C2 + C + c] = s_r[idx];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T, int VW, int M>
__global__ __launch_bounds__(S2S_THREADS) void set2set_bwd_kernel(
    const T* __restrict__ x, const int32_t* __restrict__ rowptr, const float* __restrict__ w_ih, const float* __restrict__ w_hh,
    const float* __restrict__ gout, const float* __restrict__ sv_gates, const float* __restrict__ sv_c, const float* __restrict__ sv_q,
    const float* __restrict__ sv_r, const float* __restrict__ sv_a, float* __restrict__ da_ws, T* __restrict__ dx, float* __restrict__ dG,
    int64_t N, int64_t S, int C, int steps, int lpn_log2) {
    constexpr int GT = S2S_GT;
    constexpr int U = 8 / M;
    constexpr int UD = 4;                    // rows in flight per slot in the dx pass
    extern __shared__ float s2s_lds[];
    const int C2 = 2 * C, C3 = 3 * C, C4 = 4 * C;
    float* s_dq = s2s_lds;                   // [GT][C]      dL/dq_t (with the carried dh)
    float* s_dc = s_dq + GT * C;             // [GT][C]      carried dL/dc
    float* s_dr = s_dc + GT * C;             // [GT][T][C]   dL/dr_t of every step (the dx pass needs them all)
    float* s_qt = s_dr + GT * steps * C;     // [GT][T][C]   q_t
    float* s_dg = s_qt + GT * steps * C;     // [GT][4C]     dG_t
    float* s_tmp = s_dg + GT * C4;           // [GT][3C]     [W_ih | W_hh]^T dG_t
    float* s_ss = s_tmp + GT * C3;           // [GT][T]      s_t = sum a_n da_n
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int64_t s0 = (int64_t)blockIdx.x * GT;
    const S2SLanes L(lane, lpn_log2, C / VW);

    for (int idx = tid; idx < GT * C; idx += S2S_THREADS) {
        const int g = idx / C, c = idx - g * C;
        const int64_t s = s0 + g;
        s_dq[idx] = s < S ? gout[s * C2 + c] : 0.0f;
        s_dc[idx] = 0.0f;
        for (int t = 0; t < steps; ++t) {
            s_dr[(g * steps + t) * C + c] = (s < S && t == steps - 1) ? gout[s * C2 + C + c] : 0.0f;
            s_qt[(g * steps + t) * C + c] = s < S ? sv_q[((int64_t)t * S + s) * C + c] : 0.0f;
        }
    }
    for (int i = tid; i < GT * steps; i += S2S_THREADS) s_ss[i] = 0.0f;
    __syncthreads();

    for (int t = steps - 1; t >= 0; --t) {
        // ---- attention: s = sum a_n da_n, v = sum a_n da_n x_n; dq += v - s r_t
        for (int g = wave; g < GT; g += S2S_THREADS / WAVE) {
            const int64_t s = s0 + g;
            const int64_t end = s < S ? min((int64_t)rowptr[s + 1], N) : 0, beg = s < S ? max((int64_t)rowptr[s], (int64_t)0) : 0;
            float drv[M][VW], vacc[M][VW];
            s2s_load_state<M, VW>(L, s_dr + (g * steps + t) * C, drv);
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int i = 0; i < VW; ++i) vacc[m][i] = 0.0f;
            float ssum = 0.0f;
            const float* at = sv_a + (int64_t)t * N;
            float* dat = da_ws ? da_ws + (int64_t)t * N : nullptr;
            for (int64_t n0 = beg; n0 < end; n0 += (int64_t)L.npw * U) {
                float xv[U][M][VW];
#pragma unroll
                for (int u = 0; u < U; ++u) s2s_load_row<T, VW, M>(L, x, n0 + u * L.npw + L.slot, end, C, xv[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t n = n0 + u * L.npw + L.slot;
                    float da = 0.0f;
#pragma unroll
                    for (int m = 0; m < M; ++m)
#pragma unroll
                        for (int i = 0; i < VW; ++i) da = fmaf(xv[u][m][i], drv[m][i], da);
                    da = s2s_slot_sum(da, L.lpn);
                    if (n < end) {
                        const float w = at[n] * da;
                        ssum += w;
#pragma unroll
                        for (int m = 0; m < M; ++m)
#pragma unroll
                            for (int i = 0; i < VW; ++i) vacc[m][i] = fmaf(w, xv[u][m][i], vacc[m][i]);
                        if (dat && L.lc == 0) dat[n] = da;
                    }
                }
            }
            ssum = s2s_wave_sum(ssum, L.lpn);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const int iv = L.lc + m * L.lpn;
#pragma unroll
                for (int i = 0; i < VW; ++i) {
                    const float v = s2s_wave_sum(vacc[m][i], L.lpn);
                    if (L.slot == 0 && iv < L.nvec && s < S) {
                        const int c = iv * VW + i;
                        s_dq[g * C + c] += v - ssum * sv_r[((int64_t)t * S + s) * C + c];
                    }
                }
            }
            if (lane == 0) s_ss[g * steps + t] = ssum;
        }
        __syncthreads();
        // ---- LSTM cell
        for (int idx = tid; idx < GT * C; idx += S2S_THREADS) {
            const int g = idx / C, c = idx - g * C;
            const int64_t s = s0 + g;
            float d_i = 0.0f, d_f = 0.0f, d_g = 0.0f, d_o = 0.0f;
            if (s < S) {
                const int64_t row = (int64_t)t * S + s;
                const float* gp = sv_gates + row * C4 + c;
                const float gi = gp[0], gf = gp[C], gg = gp[C2], go = gp[3 * C];
                const float cprev = t > 0 ? sv_c[(row - S) * C + c] : 0.0f;
                const float th = tanhf(sv_c[row * C + c]);
                const float dq = s_dq[idx];
                const float dc = s_dc[idx] + dq * go * (1.0f - th * th);
                d_i = dc * gg * gi * (1.0f - gi);
                d_f = dc * cprev * gf * (1.0f - gf);
                d_g = dc * gi * (1.0f - gg * gg);
                d_o = dq * th * go * (1.0f - go);
                s_dc[idx] = dc * gf;
                float* dp = dG + row * C4 + c;
                dp[0] = d_i; dp[C] = d_f; dp[C2] = d_g; dp[3 * C] = d_o;
            }
            s_dg[g * C4 + c] = d_i; s_dg[g * C4 + C + c] = d_f; s_dg[g * C4 + C2 + c] = d_g; s_dg[g * C4 + 3 * C + c] = d_o;
        }
        __syncthreads();
        if (t == 0) break;                    // q*_0 = h_0 = 0: nothing upstream
        // ---- [dq*_{t-1} | dh_{t-1}] = [W_ih | W_hh]^T dG_t: thread = column
        for (int k = tid; k < C3; k += S2S_THREADS) {
            const float* p = k < C2 ? w_ih + k : w_hh + (k - C2);
            const int64_t ld = k < C2 ? C2 : C;
            float acc[GT];
#pragma unroll
            for (int g = 0; g < GT; ++g) acc[g] = 0.0f;
#pragma unroll 8      // (measured: 16 loads in flight per thread cost 15 % of the whole readout at 8192 graphs)
            for (int j = 0; j < C4; ++j) {
                const float w = p[j * ld];
#pragma unroll
                for (int g = 0; g < GT; ++g) acc[g] = fmaf(w, s_dg[g * C4 + j], acc[g]);
            }
#pragma unroll
            for (int g = 0; g < GT; ++g) s_tmp[g * C3 + k] = acc[g];
        }
        __syncthreads();
        for (int idx = tid; idx < GT * C; idx += S2S_THREADS) {
            const int g = idx / C, c = idx - g * C;
            s_dq[idx] = s_tmp[g * C3 + c] + s_tmp[g * C3 + C2 + c];
            s_dr[(g * steps + t - 1) * C + c] = s_tmp[g * C3 + C + c];
        }
        __syncthreads();
    }

    if (!dx) return;
    // ---- dx_n = sum_t a_tn dr_t + a_tn (da_tn - s_t) q_t, written once
    for (int g = wave; g < GT; g += S2S_THREADS / WAVE) {
        const int64_t s = s0 + g;
        const int64_t end = s < S ? min((int64_t)rowptr[s + 1], N) : 0, beg = s < S ? max((int64_t)rowptr[s], (int64_t)0) : 0;
        for (int64_t n0 = beg; n0 < end; n0 += (int64_t)L.npw * UD) {
            float acc[UD][M][VW];
#pragma unroll
            for (int u = 0; u < UD; ++u)
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int i = 0; i < VW; ++i) acc[u][m][i] = 0.0f;
            for (int t = 0; t < steps; ++t) {
                float an[UD], de[UD], drv[M][VW], qv[M][VW];
                const float st = s_ss[g * steps + t];
#pragma unroll
                for (int u = 0; u < UD; ++u) {
                    const int64_t n = n0 + u * L.npw + L.slot;
                    an[u] = n < end ? sv_a[(int64_t)t * N + n] : 0.0f;
                    de[u] = n < end ? da_ws[(int64_t)t * N + n] : 0.0f;
                }
                s2s_load_state<M, VW>(L, s_dr + (g * steps + t) * C, drv);
                s2s_load_state<M, VW>(L, s_qt + (g * steps + t) * C, qv);
#pragma unroll
                for (int u = 0; u < UD; ++u) {
                    de[u] = an[u] * (de[u] - st);
#pragma unroll
                    for (int m = 0; m < M; ++m)
#pragma unroll
                        for (int i = 0; i < VW; ++i) acc[u][m][i] = fmaf(de[u], qv[m][i], fmaf(an[u], drv[m][i], acc[u][m][i]));
                }
            }
#pragma unroll
            for (int u = 0; u < UD; ++u) {
                const int64_t n = n0 + u * L.npw + L.slot;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const int iv = L.lc + m * L.lpn;
                    if (n < end && iv < L.nvec) S2SRow<T, VW>::st(dx + n * C + iv * VW, acc[u][m]);
                }
            }
        }
    }
    // ---- rows outside every segment: exact zeros
    const int64_t lo = (int64_t)rowptr[0] * C, hi = (int64_t)rowptr[S] * C, total = N * C;
    const int64_t cnt = lo + (total - hi), stride = (int64_t)gridDim.x * S2S_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * S2S_THREADS + tid; i < cnt; i += stride) Elem<T>::st(dx + (i < lo ? i : i - lo + hi), 0.0f);
}

static int s2s_check(const char* name, int64_t N, int64_t S, int C, int T, int dtype) {
    MDL_REQUIRE(mdl_set2set_supported(C, T, dtype), MDL_E_UNSUPP, "%s: unsupported C = %d, T = %d, dtype = %d (1 <= C <= %d, 1 <= T <= %d)",
                name, C, T, dtype, S2S_MAX_C, S2S_MAX_T);
    MDL_REQUIRE(N >= 0 && S >= 0 && N < ((int64_t)1 << 31) && cdiv(S, S2S_GT) < ((int64_t)1 << 31), MDL_E_ARG, "%s: bad N = %lld, S = %lld", name,
                (long long)N, (long long)S);
    return MDL_OK;
}

static bool s2s_aligned(std::initializer_list<const void*> ptrs, size_t a) {
    for (const void* p : ptrs)
        if (p && reinterpret_cast<uintptr_t>(p) % a) return false;
    return true;
}

// lanes per node slot (log2): the smallest power of two that covers the row's vectors, at most 32 lanes of vectors / the wave
static int s2s_lpn_log2(int nvec, int cap_log2) {
    int l = 0;
    while ((1 << l) < nvec && l < cap_log2) ++l;
    return l;
}

}  // namespace mdl

extern "C" int mdl_set2set_supported(int C, int T, int dtype) {
    return (C >= 1 && C <= mdl::S2S_MAX_C && T >= 1 && T <= mdl::S2S_MAX_T && (dtype == MDL_F32 || dtype == MDL_BF16)) ? 1 : 0;
}

#define S2S_DISPATCH(KERNEL, TT, ...)                                                                                              \
    do {                                                                                                                           \
        if (vec)                                                                                                                   \
            hipLaunchKernelGGL((KERNEL<TT, 4, 1>), grid, dim3(S2S_THREADS), lds, st, __VA_ARGS__, s2s_lpn_log2(C / 4, 5));           \
        else if (C <= 64)                                                                                                          \
            hipLaunchKernelGGL((KERNEL<TT, 1, 1>), grid, dim3(S2S_THREADS), lds, st, __VA_ARGS__, s2s_lpn_log2(C, 6));               \
        else                                                                                                                       \
            hipLaunchKernelGGL((KERNEL<TT, 1, 2>), grid, dim3(S2S_THREADS), lds, st, __VA_ARGS__, 6);                                \
    } while (0)

extern "C" int mdl_set2set_fwd(const void* x, const int32_t* rowptr, const float* w_ih, const float* w_hh, const float* b_ih,
                               const float* b_hh, float* out, float* gates, float* c, float* q, float* r, float* a, int64_t N, int64_t S,
                               int C, int T, int dtype, mdlStream_t stream) {
    using namespace mdl;
    int rc = s2s_check("mdl_set2set_fwd", N, S, C, T, dtype);
    if (rc) return rc;
    if (S == 0) return MDL_OK;
    MDL_REQUIRE(rowptr && w_ih && w_hh && b_ih && b_hh && out && (x || N == 0), MDL_E_ARG, "mdl_set2set_fwd: null pointer");
    const bool save = gates || c || q || r || a;
    MDL_REQUIRE(!save || (gates && c && q && r && (a || N == 0)), MDL_E_ARG, "mdl_set2set_fwd: the saved state is all five buffers or none");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(S, S2S_GT));
    const size_t lds = (size_t)S2S_GT * 7 * C * sizeof(float);
    const bool vec = C % 4 == 0 && s2s_aligned({x, w_ih, w_hh}, 16);
    if (dtype == MDL_BF16)
        S2S_DISPATCH(set2set_fwd_kernel, bf16_t, (const bf16_t*)x, rowptr, w_ih, w_hh, b_ih, b_hh, out, gates, c, q, r, a, N, S, C, T);
    else
        S2S_DISPATCH(set2set_fwd_kernel, float, (const float*)x, rowptr, w_ih, w_hh, b_ih, b_hh, out, gates, c, q, r, a, N, S, C, T);
    return check_launch("mdl_set2set_fwd");
}

extern "C" int mdl_set2set_bwd(const void* x, const int32_t* rowptr, const float* w_ih, const float* w_hh, const float* g,
                               const float* gates, const float* c, const float* q, const float* r, const float* a, float* da_ws, void* dx,
                               float* dG, int64_t N, int64_t S, int C, int T, int dtype, mdlStream_t stream) {
    using namespace mdl;
    int rc = s2s_check("mdl_set2set_bwd", N, S, C, T, dtype);
    if (rc) return rc;
    MDL_REQUIRE(rowptr && w_ih && w_hh && (S == 0 || (g && gates && c && q && r && dG)) && ((x && a) || N == 0), MDL_E_ARG,
                "mdl_set2set_bwd: null pointer");
    MDL_REQUIRE(!dx || da_ws || N == 0, MDL_E_ARG, "mdl_set2set_bwd: dx needs the [T, N] workspace");
    if (S == 0 && (!dx || N == 0)) return MDL_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(S > 0 ? cdiv(S, S2S_GT) : 1));
    const size_t lds = (size_t)S2S_GT * ((9 + 2 * T) * C + T) * sizeof(float);      // <= 51.3 KB at C = 128, T = 8
    const bool vec = C % 4 == 0 && s2s_aligned({x, dx}, dtype == MDL_BF16 ? 8 : 16);
    if (dtype == MDL_BF16)
        S2S_DISPATCH(set2set_bwd_kernel, bf16_t, (const bf16_t*)x, rowptr, w_ih, w_hh, g, gates, c, q, r, a, da_ws, (bf16_t*)dx, dG, N, S, C, T);
    else
        S2S_DISPATCH(set2set_bwd_kernel, float, (const float*)x, rowptr, w_ih, w_hh, g, gates, c, q, r, a, da_ws, (float*)dx, dG, N, S, C, T);
    return check_launch("mdl_set2set_bwd");
}
