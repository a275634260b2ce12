// cgconv_bwd.inc — K3, per-wave form: the recomputing CGConv backward edge pass (cgconv_bwd_kernel) — small batches, fp32 / bf16x3
// storage, widths other than 64; the edge-per-lane form of the bench batch is cgconv_ep2.inc.  Included by cgconv.hip behind cgconv_tiles.inc.
namespace mdl {

// ------------------------------------------------------------------------------------------
// Backward edge pass
// ------------------------------------------------------------------------------------------
constexpr int BWD_WAVES = 1;   // waves per SIMD the backward kernel is register-allocated for
template <typename T, int CP_, int G_, int VEC, int EW, int WM, int WSP = 0, bool X3 = false>
__global__ __launch_bounds__(256, BWD_WAVES) void cgconv_bwd_kernel(CgParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef Mma<T> M;
    typedef Gate<M::FAST || X3> GT;   // x3: hardware exp2 / log2 / rcp (1 ulp) on base-2 pre-activations, like the bf16 kernels
    typedef Dims<T, CP_, G_, EW, WSP, X3> D;
    constexpr bool ST = D::STATIC;
    constexpr bool BF = std::is_same<T, bf16_t>::value;
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
    const int ch = s * 32 + i;
    constexpr bool BC = G_ != 0 && (G_ % 16) != 0;
    const float bf = (BC || p.bias_col) ? 0.0f : p.bpack[ch], bs = (BC || p.bias_col) ? 0.0f : p.bpack[dm.Cp + ch];
    const T* x = static_cast<const T*>(p.x);
    const T* go = static_cast<const T*>(p.gout);
    const int C2 = 2 * dm.Cp;

    // dwe accumulators: [part f|s][n-tile of G]  (rows = channel slot, cols = edge feature)
    constexpr int GNT = G_ ? (G_ + 31) / 32 : 2;
    f32x16 dwe_acc[2][GNT];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < GNT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) dwe_acc[a][b][r] = 0.0f;

    float dbf_acc = 0.0f, dbs_acc = 0.0f;
    int oh_a = -1;                   // where this lane currently has its 1.0 in the one-hot tables it keeps (bf16 path):
                                     // lanes h = 0 keep the TARGET tables (oh_t, oh_e), lanes h = 1 the WINDOW table (oh_w)
    // Work distribution.  Static: one edge-balanced node range per wave (NodeRange).  Dynamic (p.ctr, large
    // problems): the waves of a slice take 32-node groups from a shared counter — equal tile counts do not mean equal
    // time (graphs wider than the source window fall back to atomics, CUs differ in memory latency), and the
    // kernel ends with its slowest wave.  The next group id is requested at the top of the current group.
    const bool dyn = p.ctr != nullptr;
    NodeRange R{0, 0};
    if (!dyn) R = NodeRange(p, __builtin_amdgcn_readfirstlane(gidx), gstride, lane);
    const int nend = dyn ? (int)p.N : R.nb;
    int gpend = 0;                                   // lane 0: group id returned by the counter (in flight)
    if (dyn && lane == 0) gpend = (int)atomicAdd(p.ctr + s, 1u);
    // The last groups the counter hands out are HALF groups (16 nodes): a 32-node group is ~13 tiles = 45 us of a wave's
    // ~550, and the kernel ends with the wave that drew the last one (measured spread of the waves' end times: 10 %).
    auto group_start = [&](int g) { return g < p.g_full ? 32 * g : 32 * p.g_full + 16 * (g - p.g_full); };
    int n0 = dyn ? group_start(__builtin_amdgcn_readfirstlane(gpend)) : R.na;
    while (n0 < nend) {
        const int n1 = min(n0 + ((dyn && n0 >= 32 * p.g_full) ? 16 : 32), nend);
        if (dyn && lane == 0) gpend = (int)atomicAdd(p.ctr + s, 1u);   // next group: issued now, read at the end of this one
        const int e0 = p.rowptr[n0];          // n0 is wave-uniform: scalar loads
        const int e1 = p.rowptr[n1];

        // ---- group prologue.  Every load below is unconditional on a clamped index and all of them are
        // issued before the first use, so the group pays ~one memory round trip (a guarded load costs one each).
        // (1) in-degrees of the group's nodes: lane i keeps 1/deg of node slot i
        const int nd = min(n0 + i, n1 - 1);
        const int dg0 = p.rowptr[nd], dg1 = p.rowptr[nd + 1];
        // (2) grad_out columns of this lane's channel for the B fragments of the one-hot expansion to edges
        constexpr bool PK = BF || X3;                // k-slots of a fragment: eight node slots per lane half (bf16 MFMA shapes)
        constexpr int NFg = PK ? 2 : 16, PERg = PK ? 8 : 1;
        float graw[NFg][PERg];
        {
            const int chc = min(ch, dm.C - 1);
#pragma unroll
            for (int f = 0; f < NFg; ++f)
#pragma unroll
                for (int q = 0; q < PERg; ++q) {
                    const int ns = PK ? (16 * f + 8 * h + q) : (2 * f + h);
                    graw[f][q] = Elem<T>::ld(go + (int64_t)min(n0 + ns, n1 - 1) * dm.C + chc);
                }
        }
        // (3) source window base.  The sources of a group's edges are its in-graph neighbours, i.e. a short
        // node range: sums by SOURCE for the 64 nodes [wb, wb+64) are kept in registers (one-hot MFMA, like the
        // target reduction) and flushed once per group; only sources outside the window (very large graphs)
        // fall back to per-edge atomics.  wb = smallest source of the group.
        int wb = 0x7fffffff;
        for (int eb = e0; eb < e1; eb += 8 * WAVE) {
            int sv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) sv[u] = p.src[min(eb + u * WAVE + lane, e1 - 1)];     // clamp, never guard
#pragma unroll
            for (int u = 0; u < 8; ++u) wb = min(wb, sv[u]);                                    // (clamped slots repeat a real edge)
        }
        // (4) first tiles of the edge stream
        TileIdx cur, nxt, nn;
        EWords<T, G_, EW> ew;
        XFrags<T, WSP ? 0 : CP_, VEC, X3> xf, xn;
        PFrags<CP_, 1> pf, pn;                      // W-split: the projection rows of this wave's slice instead of x rows
        bf16x8 idf[2];
        if constexpr (WSP != 0) identity_frags(i, h, idf);
        cur.template load<!ST>(p, e0, e1, i, n0);
        nxt = cur;
        if (e0 + 32 < e1) nxt.template load<!ST>(p, e0 + 32, e1, i, n0);
        nn = nxt;
        constexpr bool XDB = !(X3 && CP_ > 64);   // (x3 at 128 channels: two sets of fp32 x chunks are 256 registers)
        if constexpr (ST) ew.prefetch(p, lane, e0, min(32, e1 - e0), cur.ep);
        if constexpr (WSP != 0) pf.load(p.pt, p.ps, cur.tgt, cur.src, h, s);
        else if constexpr (CP_ != 0 && XDB) xf.load(x, dm.C, cur.tgt, cur.src, h);

        const float invd = (p.aggr == MDL_MEAN) ? 1.0f / (float)max(dg1 - dg0, 1) : 1.0f;
        typename M::frag_t gB[NFg];
        SplitFrag gBx[2];                            // x3: grad_out / deg as (hi, lo) fragments
#pragma unroll
        for (int f = 0; f < NFg; ++f) {
            float v[PERg];
#pragma unroll
            for (int q = 0; q < PERg; ++q) {
                const int ns = PK ? (16 * f + 8 * h + q) : (2 * f + h);
                const float sc = __shfl(invd, ns);
                v[q] = (n0 + ns < n1 && ch < dm.C) ? graw[f][q] * sc : 0.0f;
            }
            if constexpr (BF) gB[f] = pack_bf16x8(v);
            else if constexpr (X3) gBx[f] = split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]});
            else gB[f] = v[0];
        }

        TMARK(12);           // (timing builds: prologue up to here = loads + their wait + the gB shuffles)
        f32x16 Rf, Rs;
#pragma unroll
        for (int r = 0; r < 16; ++r) { Rf[r] = 0.0f; Rs[r] = 0.0f; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wb = min(wb, __shfl_xor(wb, o));
        wb = __builtin_amdgcn_readfirstlane(wb);
        f32x16 Wf[2], Ws[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { Wf[mt][r] = 0.0f; Ws[mt][r] = 0.0f; }
        if constexpr (BF) w.touched_b[lane] = 0; else if (lane == 0) *w.touched = 0ull;

            TRESET();
        for (int eb = e0; eb < e1; eb += 32) {
            TMARK(0);
            const int nv = min(32, e1 - eb);
            const bool valid_i = i < nv;
            const int my_ts = valid_i ? (cur.tgt - n0) : 0xff;
            const unsigned my_ss = (unsigned)(cur.src - wb);
            const bool in_win = valid_i && my_ss < 64u;
            const bool oob = valid_i && !in_win;
            wave_lds_fence();
            if constexpr (ST) ew.commit(w.et, dm.EKS, lane); else stage_e_tile<T, EW>(p, dm, w, lane, eb, nv, cur.ep);
            if constexpr (BF) {
                // Branch-free, and split over the two half-waves (both hold the indices of edge slot i): lanes h = 0 keep the
                // target-side tables, lanes h = 1 the source-window side.  Every store is unconditional; a lane with nothing to
                // write aims at its own dummy dword.  (As `if (h == 0) { if (changed) { if (old >= 0) ... } }` this was a chain
                // of ~20 divergent skip branches per tile, each a v_cmp -> saveexec -> branch round trip, and one basic block
                // boundary each for the scheduler.)
                unsigned char* const dmb = reinterpret_cast<unsigned char*>(w.dummy + lane);
                bf16_t* const dmh = reinterpret_cast<bf16_t*>(w.dummy + lane);
                reinterpret_cast<unsigned char*>(h ? w.ssl : w.tsl)[i] =
                    h ? (in_win ? (unsigned char)my_ss : (unsigned char)0xff) : (unsigned char)my_ts;
                *(h ? (w.srcl + i) : (w.dummy + lane)) = oob ? cur.src : -1;
                *((h && in_win) ? (w.touched_b + my_ss) : dmb) = 1;
                const int nA = h ? (in_win ? (int)my_ss : -1) : (valid_i ? my_ts : -1);
                bf16_t* const tabA = (h ? w.oh_w : w.oh_t) + oh_pos(i);
                const bool chg = oh_a != nA, clr = chg && oh_a >= 0, set = chg && nA >= 0;
                *(clr ? tabA + oh_a * OHS : dmh) = 0;
                *(set ? tabA + nA * OHS : dmh) = 0x3F80;
                *((clr && h == 0) ? w.oh_e + i * OHS + oh_a : dmh) = 0;
                *((set && h == 0) ? w.oh_e + i * OHS + nA : dmh) = 0x3F80;
                oh_a = nA;
            } else if (h == 0) {
                reinterpret_cast<unsigned char*>(w.tsl)[i] = (unsigned char)my_ts;
                reinterpret_cast<unsigned char*>(w.ssl)[i] = in_win ? (unsigned char)my_ss : (unsigned char)0xff;
                w.srcl[i] = oob ? cur.src : -1;
                if (in_win) atomicOr(w.touched, 1ull << my_ss);
            }
            wave_lds_fence();
            TMARK(1);

            if constexpr (CP_ != 0 && !XDB && WSP == 0) xf.load(x, dm.C, cur.tgt, cur.src, h);
            // Unconditional on purpose (indices are clamped, so the last tile of a group re-reads valid rows): a path
            // that skips these loads merges into the loop with "the x fragments are the newest loads in flight", and
            // the waits hipcc then puts in front of the MFMAs drain this tile's prefetches as well.
            if constexpr (WSP != 0) pn.load(p.pt, p.ps, nxt.tgt, nxt.src, h, s);
            else if constexpr (CP_ != 0 && XDB) xn.load(x, dm.C, nxt.tgt, nxt.src, h);
            nn.template load<!ST, false>(p, eb + 64, e1, i, n0);
            if constexpr (ST) ew.prefetch(p, lane, eb + 32, 32, nxt.ep);

            TMARK(2);
            f32x16 accf, accs;
#pragma unroll
            for (int r = 0; r < 16; ++r) { accf[r] = bf; accs[r] = bs; }
            if constexpr (WSP != 0) pre_tile_wsp<CP_, 1, 0>(dm, w, lane, s, 0, pf, idf, accf, accs);
            else pre_tile<T, CP_, VEC, WM, 0, X3>(p, dm, w, lane, s, cur.tgt, cur.src, xf, accf, accs);
            TPIN16(accf); TPIN16(accs);
            TMARK(3);

            // dmv[edge slot][ch] = grad_out[tgt(edge)][ch] / deg : one-hot(edge -> node slot) x gB
            f32x16 dmv;
#pragma unroll
            for (int r = 0; r < 16; ++r) dmv[r] = 0.0f;
            if constexpr (BF) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    dmv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oh_frag(w.oh_e, i, ks, h), gB[ks], dmv, 0, 0, 0);
            } else if constexpr (X3) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 a;                        // one-hot(edge slot i -> node slot 16 ks + 8 h + q), exact in bf16
#pragma unroll
                    for (int q = 0; q < 8; ++q) a[q] = (my_ts == 16 * ks + 8 * h + q) ? (short)0x3F80 : (short)0;
                    dmv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, gBx[ks].lo, dmv, 0, 0, 0);
                    dmv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, gBx[ks].hi, dmv, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int f = 0; f < 16; ++f)
                    dmv = __builtin_amdgcn_mfma_f32_32x32x2f32((my_ts == 2 * f + h) ? 1.0f : 0.0f, gB[f], dmv, 0, 0, 0);
            }

            TPIN16(dmv);
            TMARK(4);
            // gate derivative -> dpre (in place in accf/accs)
            // (dmv is an exact 0 for edge slots >= nv — their one-hot row is empty — so dpre is 0 there)
            {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float sf, sp_u, ss;
                    GT::deriv(accf[r], accs[r], sf, sp_u, ss);
                    const float t = dmv[r] * sf;
                    accf[r] = (t * GT::M_SCALE) * (1.0f - sf) * sp_u;
                    accs[r] = t * ss;
                }
            }

            // sources outside the window: per-edge fp32 atomics (graphs wider than the window).  Issued as early as the
            // values exist: a pending atomic turns every later wait for a load into vmcnt(0) (loads and stores complete out of
            // order with respect to each other), so the more of this tile's MFMA work lies behind them the better
            if (__any(oob) && ch < dm.C) {
                // the 16 source ids of this lane's rows (d_row(4q+k, h) = 8q + 4h + k) in four 16-byte LDS reads up front:
                // read one by one between the atomics, each costs an LDS round trip the compiler will not hoist
                typedef __attribute__((ext_vector_type(4))) int i32x4;
                int sj[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const i32x4 v = *reinterpret_cast<const i32x4*>(w.srcl + 8 * q + 4 * h);
#pragma unroll
                    for (int k = 0; k < 4; ++k) sj[4 * q + k] = v[k];
                }
                if (BF && p.rs16) {
                    bf16_t* const b16 = reinterpret_cast<bf16_t*>(p.r_src) + (ch & ~1);
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const int64_t ra = (int64_t)max(sj[r], 0) * C2, rb = (int64_t)max(sj[r + 1], 0) * C2;
                        rsrc16_add2(b16, ra, rb, accf[r], accf[r + 1], sj[r] >= 0, sj[r + 1] >= 0, i & 1);
                        rsrc16_add2(b16 + dm.Cp, ra, rb, accs[r], accs[r + 1], sj[r] >= 0, sj[r + 1] >= 0, i & 1);
                    }
                } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (sj[r] >= 0) {
                        float* dst = p.r_src + (int64_t)sj[r] * C2 + ch;
                        unsafeAtomicAdd(dst, accf[r]);
                        unsafeAtomicAdd(dst + dm.Cp, accs[r]);
                    }
                }
                }
            }

            TPIN16(accf); TPIN16(accs);
            TMARK(5);
            DFrags<T> dp;
            DFragsX3 dpx;
            if constexpr (X3) dpx.pack(accf, accs); else dp.pack(accf, accs);
            TMARK(6);
            if constexpr (BF) {
                seg_reduce2_tab(dp, w.oh_t, i, h, Rf, Rs);                  // by target  -> r_tgt
                TPIN16(Rf); TPIN16(Rs);
                TMARK(7);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) seg_reduce2_tab(dp, w.oh_w, i + 32 * mt, h, Wf[mt], Ws[mt]);   // by source window
            } else {
                unsigned t4[4], s4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { t4[j] = w.tsl[2 * j + h]; s4[j] = w.ssl[2 * j + h]; }
                if constexpr (X3) {
                    seg_reduce2_x3(dpx, t4, (unsigned)i, Rf, Rs);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) seg_reduce2_x3(dpx, s4, (unsigned)(i + 32 * mt), Wf[mt], Ws[mt]);
                } else {
                    seg_reduce2<T>(dp, t4, (unsigned)i, Rf, Rs);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) seg_reduce2<T>(dp, s4, (unsigned)(i + 32 * mt), Wf[mt], Ws[mt]);
                }
            }

            TMARK(8);
            // dwe[ch][gcol] += sum_slot dpre[slot][ch] * e[slot][gcol]
            //   A = dpre^T (lane = channel, k = edge slots: own registers), B = e tile column (LDS)
#pragma unroll
            for (int nt = 0; nt < GNT; ++nt) {
                const int gcol = nt * 32 + i;
                if (nt * 32 < dm.KE) {
                    if constexpr (BF) {
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            bf16x8 b;
                            if constexpr (ST) {
                                // column fragment of the row-major e tile with the LDS transpose read: each 16-lane group
                                // reads a [4 rows][16 cols] block (lane t supplies row t>>2, cols 4*(t&3)..) and lane t gets
                                // column t of the 4 rows.  K slots 8ks+q = rows 16ks+4h+q (q<4) and 16ks+8+4h+(q-4).
                                typedef __attribute__((ext_vector_type(4))) short s16x4;
                                typedef __attribute__((address_space(3))) s16x4* lds4_t;
                                const int t = i & 15;
                                const bf16_t* base = w.et + (16 * ks + 4 * h + (t >> 2)) * dm.EKS + nt * 32 + (i & 16) + 4 * (t & 3);
                                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(base));
                                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(base + 8 * dm.EKS));
                                b = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                            } else {
#pragma unroll
                                for (int q = 0; q < 8; ++q)
                                    b[q] = (gcol < dm.KE) ? (short)w.et[d_row(8 * ks + q, h) * dm.EKS + gcol] : (short)0;
                            }
                            dwe_acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dp.f[ks], b, dwe_acc[0][nt], 0, 0, 0);
                            dwe_acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dp.s[ks], b, dwe_acc[1][nt], 0, 0, 0);
                        }
                    } else if constexpr (X3) {
                        // both operands split: dpre_hi e_hi + dpre_lo e_hi + dpre_hi e_lo (k = the tile's 32 edge slots)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            float ev[8];
#pragma unroll
                            for (int q = 0; q < 8; ++q) ev[q] = w.et[d_row(8 * ks + q, h) * dm.EKS + gcol];
                            const SplitFrag b = split8(f32x4{ev[0], ev[1], ev[2], ev[3]}, f32x4{ev[4], ev[5], ev[6], ev[7]});
                            dwe_acc[0][nt] = mma_x3(dpx.f[ks], b, dwe_acc[0][nt]);
                            dwe_acc[1][nt] = mma_x3(dpx.s[ks], b, dwe_acc[1][nt]);
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float b = (gcol < dm.KE) ? w.et[d_row(r, h) * dm.EKS + gcol] : 0.0f;
                            dwe_acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(accf[r], b, dwe_acc[0][nt], 0, 0, 0);
                            dwe_acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(accs[r], b, dwe_acc[1][nt], 0, 0, 0);
                        }
                    }
                }
            }
            cur = nxt;
            nxt = nn;
            if constexpr (WSP != 0) pf = pn; else if constexpr (XDB) xf = xn;
            TMARK(9);
            TTILE();
        }

        // the id of the next group (requested at the top of this one) is read BEFORE the flush: behind ~100 atomics and
        // stores, waiting for any returning operation means waiting for all of them
        const int n0_dyn = dyn ? group_start(__builtin_amdgcn_readfirstlane(gpend)) : 0;
        // flush the source window: one atomic row update per touched window node (instead of per edge)
        wave_lds_fence();
        {
            // (the mask is the same in every lane: SGPRs; d_row(r, h) = d_row(r, 0) + 4h: one per-lane shift, then constant
            // bit tests — per-row masks 1 << sl hoisted out of the group loop are the first thing hipcc spills)
            unsigned long long tm;
            if constexpr (BF) {
                tm = __ballot(w.touched_b[lane] != 0);
            } else {
                const unsigned long long tmv = *w.touched;
                tm = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(tmv >> 32)) << 32) |
                     (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)tmv);
            }
            const unsigned long long tmh = tm >> (4 * h);
            if (BF && p.rs16) {
                // (static bf16 shapes only: C == Cp, every lane owns a real column)
                bf16_t* const b16 = reinterpret_cast<bf16_t*>(p.r_src) + (int64_t)(wb + 4 * h) * C2 + (ch & ~1);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const int ra = 32 * mt + d_row(r, 0), rb = ra + 1;
                        const bool ca = (tmh >> ra) & 1ull, cb = (tmh >> rb) & 1ull;
                        rsrc16_add2(b16, (int64_t)ra * C2, (int64_t)rb * C2, Wf[mt][r], Wf[mt][r + 1], ca, cb, i & 1);
                        rsrc16_add2(b16 + dm.Cp, (int64_t)ra * C2, (int64_t)rb * C2, Ws[mt][r], Ws[mt][r + 1], ca, cb, i & 1);
                    }
            } else if (ch < dm.C) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int sl = 32 * mt + d_row(r, h);
                        if ((tmh >> (32 * mt + d_row(r, 0))) & 1ull) {          // bit sl of tm
                            float* dst = p.r_src + (int64_t)(wb + sl) * C2 + ch;
                            unsafeAtomicAdd(dst, Wf[mt][r]);
                            unsafeAtomicAdd(dst + dm.Cp, Ws[mt][r]);
                        }
                    }
            }
        }
        // r_tgt rows of this group (each written exactly once); bias gradient = their column sums
#pragma unroll
        for (int r = 0; r < 16; ++r) { dbf_acc += Rf[r]; dbs_acc += Rs[r]; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + d_row(r, h);
            if (n < n1) {
                T* dst = static_cast<T*>(p.r_tgt) + (int64_t)n * C2 + ch;
                Elem<T>::st(dst, Rf[r]);
                Elem<T>::st(dst + dm.Cp, Rs[r]);
            }
        }
        TMARK(11);
        n0 = dyn ? n0_dyn : n1;
    }

    TFLUSH(16);
    if (p.db) {
        dbf_acc += __shfl_xor(dbf_acc, 32);
        dbs_acc += __shfl_xor(dbs_acc, 32);
        if (h == 0) {
            unsafeAtomicAdd(p.db + ch, dbf_acc);
            unsafeAtomicAdd(p.db + dm.Cp + ch, dbs_acc);
        }
    }
    // flush the wave's dwe partial sums: D rows = channel slot d_row(r,h) of slice s, cols = feature
    if (p.dwe_combine) {
        // Two slices, four waves: waves w and w + 2 of a workgroup hold partial sums of the SAME slice.  The flush is 64 atomic
        // instructions per wave on addresses every wave of the slice hits (12.5 of 45 us at the reference's batch size, where a
        // wave has one or two tiles of work in front of it): wave w + 2 hands its sums over through the LDS area of the weights —
        // free once every wave is out of its loop — and only wave w flushes.
        const int wv4 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        float* const cb = reinterpret_cast<float*>(smem) + (wv4 & 1) * (2 * GNT * 16 * WAVE) + lane;
        __syncthreads();
        if (wv4 >= 2) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int nt = 0; nt < GNT; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) cb[((a * GNT + nt) * 16 + r) * WAVE] = dwe_acc[a][nt][r];
        }
        __syncthreads();
        if (wv4 >= 2) return;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int nt = 0; nt < GNT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) dwe_acc[a][nt][r] += cb[((a * GNT + nt) * 16 + r) * WAVE];
    }
#pragma unroll
    for (int nt = 0; nt < GNT; ++nt) {
        const int gcol = nt * 32 + i;
        if (gcol < dm.G) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = s * 32 + d_row(r, h);
                unsafeAtomicAdd(p.dwe + (int64_t)c * p.GP + gcol, dwe_acc[0][nt][r]);
                unsafeAtomicAdd(p.dwe + (int64_t)(dm.Cp + c) * p.GP + gcol, dwe_acc[1][nt][r]);
            }
        }
    }
}

}  // namespace mdl
