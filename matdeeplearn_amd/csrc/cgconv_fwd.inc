// cgconv_fwd.inc — K2: the fused CGConv forward kernel (cgconv_fwd_kernel; design in the header of cgconv.hip and DESIGN.md 4).
// Included by cgconv.hip behind cgconv_tiles.inc.
namespace mdl {

constexpr int FWD_THREADS = 256;   // workgroup size of the forward kernel (waves share one LDS copy of W)
constexpr int FWD_WAVES = 2;       // waves per SIMD it is register-allocated for
// (fp32: the packed weights alone are 99 KB of LDS, so one 4-wave workgroup fits a CU whatever the register count — the fp32
// STATIC instantiation is allocated for ONE wave per SIMD (512 registers) instead of spilling 102 registers at 256: round 6)
constexpr int FWD_WAVES_F32 = 1;
constexpr int FWD_PRE_DEPTH = 3;   // all-slices forward: pinned LDS-read / MFMA interleave in pre_tile, reads issued ahead (-6 %)
constexpr int FWD_AGE_SKEW = 60;   // all-slices forward at two workgroups per CU: per mille of extra work for the older half
template <typename T, int CP_, int G_, int VEC, int EW, int WM, bool AB_ = false, int WSP = 0, bool X3 = false>   // WM: 0 global, 1 LDS; X3: split-bf16 products on fp32 storage
__global__ __launch_bounds__(FWD_THREADS, ((sizeof(T) == 4 && CP_ != 0) ? FWD_WAVES_F32 : FWD_WAVES)) void cgconv_fwd_kernel(CgParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef Mma<T> M;
    typedef Gate<M::FAST || X3> GT;   // x3: hardware exp2 / log2 / rcp (1 ulp) on base-2 pre-activations, like the bf16 kernels
    typedef Dims<T, CP_, G_, EW, WSP, X3> D;
    constexpr bool ST = D::STATIC;
    const D dm(p);
    WaveCtx<T> w;
    setup_wave<T>(p, dm, smem, WM == 1, w);
    TDECL;

    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int gw = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int total_waves = gridDim.x * (blockDim.x >> 6);
    // channel slice of this wave and its index among the waves of that slice (w_slice: a workgroup's waves share the slice)
    const bool wsl = (CP_ == 0 || CP_ > 64) && p.w_slice;
    const int s = wsl ? (int)blockIdx.x % p.NS : gw % p.NS;
    const int gstride = total_waves / p.NS;
    const int gidx = wsl ? ((int)blockIdx.x / p.NS) * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6) : gw / p.NS;
    // with a bias column the bias rides in the GEMM (K column G); otherwise it seeds the accumulators
    constexpr bool BC = G_ != 0 && (G_ % 16) != 0;   // bias column known at compile time
    const float bf = (BC || p.bias_col) ? 0.0f : p.bpack[s * 32 + i];
    const float bs = (BC || p.bias_col) ? 0.0f : p.bpack[dm.Cp + s * 32 + i];
    const T* x = static_cast<const T*>(p.x);
    T* out = static_cast<T*>(p.out);
    const int ch = s * 32 + i;

    if constexpr (ST && WM == 1 && CP_ <= 64) {     // (wider static shapes: one slice per wave, the workgroup keeps that slice of W in LDS)
        // One wave handles ALL channel slices of its group.  Staging the tile (edge-feature stream, index
        // loads, x gathers, one-hot table) is slice independent: doing it once per tile instead of once per
        // (tile, slice) removes the duplicated per-tile overhead; the pre-GEMM / gate / aggregation then
        // run per 32-channel slice on the same staged operands.
        constexpr int NSL = CP_ / 32;
        const int nw_total = gridDim.x * (blockDim.x >> 6);
        // Two workgroups share a CU and its SIMDs arbitrate by age: the waves of the workgroup dispatched first (block index
        // below half the grid) run 14 % faster than their younger co-residents (measured wave lifetimes 161 vs 184 us), which
        // then finish alone at half occupancy.  The older half takes FWD_AGE_SKEW per mille more of the work.
        NodeRange R(0, 0);
        {
            const int half = nw_total >> 1, gwu = __builtin_amdgcn_readfirstlane(gw);
            if ((nw_total & 1) || gridDim.x < 512) {
                R = NodeRange(p, gwu, nw_total, lane);
            } else {
                const int64_t Et = (int64_t)p.rowptr[p.N] + p.N;
                const int64_t wa = 1000 + FWD_AGE_SKEW, wb = 1000 - FWD_AGE_SKEW;        // weights of the two halves
                auto cut = [&](int k) -> int64_t {                                               // work in front of wave k
                    const int64_t units = k <= half ? wa * k : wa * half + wb * (k - half);
                    return Et * units / (1000 * (int64_t)nw_total);
                };
                R.na = gwu == 0 ? 0 : wave_lower_bound(p.rowptr, (int)p.N, cut(gwu), lane);
                R.nb = gwu == nw_total - 1 ? (int)p.N : wave_lower_bound(p.rowptr, (int)p.N, cut(gwu + 1), lane);
            }
        }
        if (R.na >= R.nb) return;
        // The wave walks its groups as one continuous stream: the next group's row pointers are requested
        // at the top of the current group, and the indices / edge-feature words of the next group's first
        // tile during the current group's last tile, so a group boundary costs no dependent round trips.
        GroupInfo G, GN;
        G.load(p, R.na, R.nb);
        GN = G;
        TileIdx cur, nxt;
        EWords<T, G_, EW> ew;
        XFrags<T, WSP ? 0 : CP_, VEC, X3> xf;
        // W-split: projection rows instead of x rows, ONE slice's fragments at a time (32 registers, like the x rows): the
        // rows of slice sl + 1 — or of the next tile's slice 0 — are requested right after slice sl's MFMAs have consumed
        // the registers, and arrive under that slice's gate arithmetic and aggregation
        PFrags<CP_, 1> pf;
        bf16x8 idf[2];
        if constexpr (WSP != 0) identity_frags(i, h, idf);
        auto load_rows = [&](int tg, int sr) {
            if constexpr (WSP != 0) pf.load(p.pt, p.ps, tg, sr, h, 0); else xf.load(x, dm.C, tg, sr, h);
        };
        bool primed = false;                                  // cur / ew / xf already hold the group's first tile
        while (true) {
            const bool hasN = G.n1 < R.nb;
            if (hasN) GN.load(p, G.n1, R.nb);
            if (G.e0 == G.e1) {
                // Nodes without edges: out = x.  The whole RUN of edge-less nodes of this wave's range is copied at once
                // with 16-byte vectors (8 rows per trip) — the padding rows of a static batch come as thousands of such
                // nodes in a row, and walking them as 32-node groups (a scalar rowptr round trip + 32 two-byte copies
                // each) made the waves that own them 3x slower than the rest of the launch.
                int ne = G.n1;
                {
                    int lo = G.n1, hi = R.nb;                      // first node in [n1, nb] whose rowptr exceeds e0
                    while (lo < hi) {
                        const int step = (hi - lo + 63) >> 6;
                        const int n = min(lo + lane * step, hi);
                        const unsigned long long gt = __ballot(n < R.nb ? p.rowptr[n + 1] > G.e0 : true);
                        if (gt == 0ull) { lo = min(lo + 63 * step, hi) + 1; continue; }
                        const int fl = __builtin_ctzll(gt);
                        if (fl == 0) { hi = lo; break; }
                        hi = min(lo + fl * step, hi);
                        lo = lo + (fl - 1) * step + 1;
                    }
                    ne = min(__builtin_amdgcn_readfirstlane(lo), R.nb);
                }
                {
                    constexpr int VW = 16 / (int)sizeof(T);        // elements per 16-byte vector
                    constexpr int VPR = CP_ / VW;                    // vectors per row (CP_ == C for the static shapes)
                    typedef __attribute__((ext_vector_type(4))) unsigned u32x4c;
                    const int64_t v0 = (int64_t)G.n0 * VPR, v1 = (int64_t)ne * VPR;
                    const u32x4c* __restrict__ xs = reinterpret_cast<const u32x4c*>(x);
                    u32x4c* __restrict__ os = reinterpret_cast<u32x4c*>(out);
                    for (int64_t q = v0 + lane; q < v1; q += 4 * WAVE) {
                        u32x4c v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) v[u] = xs[min(q + u * WAVE, v1 - 1)];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (q + u * WAVE < v1) os[q + u * WAVE] = v[u];
                    }
                }
                if (ne >= R.nb) break;
                G.load(p, ne, R.nb);
                primed = false;
                continue;
            }
            f32x16 acc_out[NSL];
#pragma unroll
            for (int sl = 0; sl < NSL; ++sl)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc_out[sl][r] = 0.0f;
            if (!primed) {
                cur.template load<false>(p, G.e0, G.e1, i, G.n0);
                ew.prefetch(p, lane, G.e0, min(32, G.e1 - G.e0), cur.ep);
                load_rows(cur.tgt, cur.src);
            }
            nxt = cur;
            bool nextHasEdges = false;                        // evaluated at the last tile (GN arrives by then)
            // saved-gate forward: the packed factors of a tile's LAST slice wait in registers and are stored during the
            // next tile (see below); abq_eb < 0 = nothing pending
            constexpr int ROWB = 4 * CP_;
            unsigned abq[16];
            int abq_eb = -1, abq_nv = 0;
            auto ab_store = [&](const unsigned (&v)[16], int eb_, int nv_, int sl_) {
                // rows past the group's end are dropped by the range check of the store resource (they belong to the
                // next group's owner); row offsets = two per-lane bases + an immediate < 4096, all inside the range check
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                    static_cast<char*>(p.ab) + (int64_t)eb_ * ROWB, 0, nv_ * ROWB, 0x00020000);
                const int vo0 = 4 * h * ROWB + sl_ * 128 + i * 4, vo1 = vo0 + 16 * ROWB;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    __builtin_amdgcn_raw_buffer_store_b32(v[r], rs, (r < 8 ? vo0 : vo1) + ((r & 3) + 8 * ((r >> 2) & 1)) * ROWB, 0, 0);
            };
            TRESET();
            for (int eb = G.e0; eb < G.e1; eb += 32) {
                const int nv = min(32, G.e1 - eb);
                const bool last = eb + 32 >= G.e1;
                TMARK(0);
                wave_lds_fence();
                ew.commit(w.et, dm.EKS, lane);
                if (h == 0) reinterpret_cast<unsigned char*>(w.tsl)[i] = (i < nv) ? (unsigned char)(cur.tgt - G.n0) : 0xff;
                wave_lds_fence();
                TMARK(1);
                // The next tile's loads are issued on EVERY path, from uniform selects of the tile base (next tile of
                // this group / first tile of the next group / this tile again when the stream ends): a path that skips
                // them joins the loop with "the x fragments are the newest loads in flight", and the waits hipcc then
                // places in front of the x MFMAs also drain the prefetches issued a few instructions earlier.
                {
                    const bool nh = hasN && GN.e0 < GN.e1;
                    nextHasEdges = last && nh;
                    const int pe = last ? (nh ? GN.e0 : eb) : eb + 32;
                    const int pe1 = nextHasEdges ? GN.e1 : G.e1;
                    const int pn0 = nextHasEdges ? GN.n0 : G.n0;
                    nxt.template load<false, false>(p, pe, pe1, i, pn0);
                    ew.prefetch(p, lane, pe, 32, 0);
                }
                TMARK(2);
                unsigned t4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) t4[j] = w.tsl[2 * j + h];
#pragma unroll
                for (int sl = 0; sl < NSL; ++sl) {
                    f32x16 accf, accs;
                    const float b0 = (BC || p.bias_col) ? 0.0f : p.bpack[sl * 32 + i];
                    const float b1 = (BC || p.bias_col) ? 0.0f : p.bpack[dm.Cp + sl * 32 + i];
#pragma unroll
                    for (int r = 0; r < 16; ++r) { accf[r] = b0; accs[r] = b1; }
                    if constexpr (WSP != 0) {
                        pre_tile_wsp<CP_, 1, FWD_PRE_DEPTH>(dm, w, lane, sl, 0, pf, idf, accf, accs);
                        pf.load(p.pt, p.ps, sl == NSL - 1 ? nxt.tgt : cur.tgt, sl == NSL - 1 ? nxt.src : cur.src, h, (sl + 1) % NSL);
                    } else {
                        pre_tile<T, CP_, VEC, WM, FWD_PRE_DEPTH, X3>(p, dm, w, lane, sl, cur.tgt, cur.src, xf, accf, accs);
                    }
                    TPIN16(accf); TPIN16(accs);
                    TMARK(3 + 3 * sl);
                    if constexpr (AB_) {
                        // Stores poison the wait counters: loads and stores complete out of order with respect to each
                        // other, so the next wait for ANY load (top of the next tile) also waits for every store in
                        // flight.  A slice's factors stored right after its gate leave the last slice ~10 % of a tile
                        // to complete before that wait (measured: +1500 cycles per tile in the first MFMA chain).  So the
                        // last slice's dwords stay in registers and go out HERE, behind the first slice's MFMA chain of
                        // the NEXT tile: more than half a tile ahead of the next wait.
                        if (sl == 0 && abq_eb >= 0) { ab_store(abq, abq_eb, abq_nv, NSL - 1); abq_eb = -1; }
                    }
                    // the x rows of the NEXT tile: requested as soon as the last slice's MFMAs have consumed this
                    // tile's fragments (same registers), so their latency hides under the gate / aggregation
                    if constexpr (WSP == 0) { if (sl == NSL - 1) load_rows(nxt.tgt, nxt.src); }   // unconditional, like the loads above
                    f32x16 m;
                    if constexpr (AB_) {
                        // m and, for the backward, A = dm/dpre_f = sigmoid'(f) softplus(s), B = dm/dpre_s = sigmoid(f) sigmoid(s)
                        // (same four transcendentals as the plain gate: the two reciprocals share one v_rcp), packed
                        // as one dword per (edge, channel): a row of a slice is 128 contiguous bytes
                        unsigned abv[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float sf, sp_u, ss;
                            GT::deriv(accf[r], accs[r], sf, sp_u, ss);
                            const float mm = sf * sp_u;
                            m[r] = mm;
                            abv[r] = pk_bf16((mm * GT::M_SCALE) * (1.0f - sf), sf * ss);
                        }
                        if (sl == NSL - 1) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) abq[r] = abv[r];
                            abq_eb = eb;
                            abq_nv = nv;
                        } else {
                            ab_store(abv, eb, nv, sl);
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) m[r] = GT::sigmoid(accf[r]) * GT::softplus_u(accs[r]);
                    }
                    TPIN16(m);
                    TMARK(4 + 3 * sl);
                    if constexpr (X3) seg_reduce_mma_x3(m, t4, i, acc_out[sl]); else seg_reduce_mma<T>(m, t4, i, acc_out[sl]);
                    TPIN16(acc_out[sl]);
                    TMARK(5 + 3 * sl);
                    __builtin_amdgcn_sched_barrier(0);      // keep the slices' register footprints apart
                }
                cur = nxt;
                TTILE();
            }
            if constexpr (AB_) {
                if (abq_eb >= 0) ab_store(abq, abq_eb, abq_nv, NSL - 1);        // the group's last tile
            }
            // epilogue: out = x + acc / deg.  All residual rows are requested first (clamped row index, no
            // guards), so the group pays one memory round trip instead of one per row.
            {
                // in-degrees straight from rowptr (lane i keeps the degree of node slot i; no count accumulator and
                // no count MFMAs in the tile loop), fetched together with the residual rows
                const int ndg = min(G.n0 + i, G.n1 - 1);
                const int dg0 = p.rowptr[ndg], dg1 = p.rowptr[ndg + 1];
                float xr[NSL][16];
#pragma unroll
                for (int sl = 0; sl < NSL; ++sl)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int n = min(G.n0 + d_row(r, h), G.n1 - 1);
                        xr[sl][r] = Elem<T>::ld(x + (int64_t)n * dm.C + sl * 32 + i);
                    }
                const float invd = (M::FAST && !X3) ? __builtin_amdgcn_rcpf((float)max(dg1 - dg0, 1)) : 1.0f / (float)max(dg1 - dg0, 1);
                float invr[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) invr[r] = __shfl(invd, d_row(r, h));
#pragma unroll
                for (int sl = 0; sl < NSL; ++sl) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int n = G.n0 + d_row(r, h);
                        float a = acc_out[sl][r] * GT::M_SCALE;
                        if (p.aggr == MDL_MEAN) a *= invr[r];
                        if (n < G.n1) Elem<T>::st(out + (int64_t)n * dm.C + sl * 32 + i, xr[sl][r] + a);
                    }
                }
            }
            TMARK(11);
            if (!hasN) break;
            G = GN;
            primed = nextHasEdges;
        }
        TFLUSH(0);
        return;
    }
    // The wave walks its groups as ONE continuous stream of edge tiles: while tile t computes, the
    // indices and edge-feature words of tile t+1 are in flight — across group boundaries too — so
    // the load pipeline never drains.  A group's epilogue (residual add, mean, store) needs no
    // dependent loads: the in-degree comes out of the one-hot MFMA (cnt) and the residual rows are
    // requested at the top of the group's last tile.
    const NodeRange R(p, __builtin_amdgcn_readfirstlane(gidx), gstride, lane);
    if (R.na >= R.nb) return;
    GroupInfo G, GN;
    G.load(p, R.na, R.nb);
    bool hasN = G.n1 < R.nb;
    if (hasN) GN.load(p, G.n1, R.nb);

    f32x16 acc_out, cnt;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc_out[r] = 0.0f; cnt[r] = 0.0f; }
    TileIdx cur, nxt;
    EWords<T, G_, EW> ew;
    XFrags<T, CP_, VEC, X3> xf;
    float xr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) xr[r] = 0.0f;

    int eb = G.e0;
    bool primed = false;          // cur / ew already hold the tile at eb (prefetched by the previous tile)
            TRESET();
    while (true) {
        if (G.e0 == G.e1) {
            // group without edges: out = x for its nodes (mean over nothing = 0)
            if (ch < dm.C) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = G.n0 + d_row(r, h);
                    if (n < G.n1) out[(int64_t)n * dm.C + ch] = x[(int64_t)n * dm.C + ch];
                }
            }
            if (!hasN) break;
            G = GN;
            hasN = G.n1 < R.nb;
            if (hasN) GN.load(p, G.n1, R.nb);
            eb = G.e0;
            primed = false;
            continue;
        }
        if (!primed) {
            cur.template load<!ST>(p, eb, G.e1, i, G.n0);
            if constexpr (ST) ew.prefetch(p, lane, eb, min(32, G.e1 - eb), cur.ep);
        }
        const int nv = min(32, G.e1 - eb);
        const bool valid_i = i < nv;
        const bool last = eb + 32 >= G.e1;
        TMARK(0);
        wave_lds_fence();
        if constexpr (ST) ew.commit(w.et, dm.EKS, lane); else stage_e_tile<T, EW>(p, dm, w, lane, eb, nv, cur.ep);
        if (h == 0) reinterpret_cast<unsigned char*>(w.tsl)[i] = valid_i ? (unsigned char)(cur.tgt - G.n0) : 0xff;
        wave_lds_fence();
        TMARK(1);

        if constexpr (CP_ != 0) xf.load(x, dm.C, cur.tgt, cur.src, h);
        // prefetch the next tile of the stream (same group, or the first tile of the next group)
        primed = false;
        if (!last) {
            nxt.template load<!ST>(p, eb + 32, G.e1, i, G.n0);
            if constexpr (ST) ew.prefetch(p, lane, eb + 32, min(32, G.e1 - eb - 32), nxt.ep);
            primed = true;
        } else {
            if (hasN && GN.e0 < GN.e1) {
                nxt.template load<!ST>(p, GN.e0, GN.e1, i, GN.n0);
                if constexpr (ST) ew.prefetch(p, lane, GN.e0, min(32, GN.e1 - GN.e0), nxt.ep);
                primed = true;
            }
            // residual rows of this group, needed by the epilogue right after this tile
            if (ch < dm.C) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = min(G.n0 + d_row(r, h), G.n1 - 1);
                    xr[r] = Elem<T>::ld(x + (int64_t)n * dm.C + ch);
                }
            }
        }

        TMARK(2);
        f32x16 accf, accs;
#pragma unroll
        for (int r = 0; r < 16; ++r) { accf[r] = bf; accs[r] = bs; }
        pre_tile<T, CP_, VEC, WM, 0, X3>(p, dm, w, lane, s, cur.tgt, cur.src, xf, accf, accs);

        TMARK(3);
        unsigned t4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t4[j] = w.tsl[2 * j + h];
        // gate.  Edge slots >= nv hold finite garbage; their one-hot column is all zero, so they
        // contribute exact zeros to the aggregation — no per-element masking needed.
        f32x16 m;
#pragma unroll
        for (int r = 0; r < 16; ++r) m[r] = GT::sigmoid(accf[r]) * GT::softplus_u(accs[r]);
        TMARK(4);
        seg_reduce_cnt<T>(m, t4, i, acc_out, cnt);
        TMARK(5);

        if (last) {
            // epilogue: out = x + acc / deg   (rows = node slots in D layout, col = channel)
            if (ch < dm.C) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = G.n0 + d_row(r, h);
                    if (n < G.n1) {
                        float a = acc_out[r] * GT::M_SCALE;
                        if (p.aggr == MDL_MEAN) {
                            const float deg = fmaxf(cnt[r], 1.0f);
                            a = M::FAST ? a * __builtin_amdgcn_rcpf(deg) : a / deg;
                        }
                        Elem<T>::st(out + (int64_t)n * dm.C + ch, xr[r] + a);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc_out[r] = 0.0f; cnt[r] = 0.0f; }
            if (!hasN) break;
            G = GN;
            hasN = G.n1 < R.nb;
            if (hasN) GN.load(p, G.n1, R.nb);
            eb = G.e0;
        } else {
            eb += 32;
        }
        cur = nxt;
        TMARK(6);
            TTILE();
    }
}

}  // namespace mdl
