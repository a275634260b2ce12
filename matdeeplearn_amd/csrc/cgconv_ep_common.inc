// cgconv_ep_common.inc — tile walk, per-edge gathers and the LDS-only barrier shared by the edge-per-lane CGConv backward
// kernels (cgconv_ep2.inc here; the first, phases-one-after-the-other version lives in experiments/csrc/cgconv_ep.inc).
// Included by cgconv.hip in the cgconv_ep.hip translation unit.

namespace ep {

typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((address_space(3))) s16x4* lds4_t;

// LDS-only workgroup barrier: the fences name the local address space, so no vmcnt wait is attached to it and the global
// loads prefetched for the next round stay in flight across it.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// wave-uniform cursor over the edge tiles of a node range (groups of <= 32 nodes, 32-edge tiles inside a group, one empty
// tile for a group without edges), like cb::TileWalk, but a group change reads no memory: the ends of the next 64 groups
// (rowptr[n + 32 k], lane k) sit in ONE vector register, fetched by one load that is waited for on the spot, and a group
// change takes its lane with v_readlane.  What this replaces: a scalar load per group change — it shares its wait counter with
// every LDS access, so the next LDS wait of the wave also waited for it (a memory round trip per group: 2-5 % of the kernel on
// the bench batch, and the whole kernel time again on the run of edge-less padding nodes at the end of a static batch, where
// every tile is a group change).
struct Walk {
    int n0, n1, e0, e1, eb, nb, used;
    int ends;            // lane 0: rowptr[nbase]; lane k: rowptr[min(nbase + 32 k, nb)] = end of the (k-1)-th group from node nbase
    bool done;           // no tile left
    __device__ __forceinline__ void fetch(const CgParams& p, int nbase) {
        const int lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int32_t* a = p.rowptr + min(nbase + 32 * lane, nb);
        asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(ends) : "v"(a) : "memory");
    }
    __device__ __forceinline__ void start(const CgParams& p, int na, int nb_) {
        nb = nb_; n0 = na;
        n1 = min(n0 + 32, nb); e0 = 0; e1 = 0; used = 0;
        if (na < nb_) {
            fetch(p, n0);
            e0 = __builtin_amdgcn_readlane(ends, 0);
            e1 = __builtin_amdgcn_readlane(ends, 1);
            used = 2;
        }
        eb = e0;
    }
    __device__ __forceinline__ void init(const CgParams& p, int na, int nb_) {
        ends = 0;
        start(p, na, nb_);
        done = na >= nb_;
    }
    __device__ __forceinline__ bool last() const { return eb + 32 >= e1; }
    __device__ __forceinline__ void next(const CgParams& p) {
        if (!last()) { eb += 32; return; }
        n0 = n1;
        if (n0 >= nb) {
            done = true;
            return;
        }
        if (used == 64) { fetch(p, n0); used = 1; }       // (once per 63 groups)
        n1 = min(n0 + 32, nb);
        e0 = e1;
        e1 = __builtin_amdgcn_readlane(ends, used);
        ++used;
        eb = e0;
    }
};

struct Tile {          // wave-uniform snapshot of the walker
    int n0, n1, e1, eb;
    bool valid;
    __device__ __forceinline__ int nv() const { return max(0, min(32, e1 - eb)); }
};

// the tile of wave `wv` in the next round; every wave walks all NW tiles so that all agree on the sequence
template <int NW>
__device__ __forceinline__ Tile take(const CgParams& p, Walk& wk, int wv, bool& round_has) {
    Tile m = {wk.n0, wk.n1, wk.e1, wk.eb, false};
    round_has = !wk.done;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const bool live = !wk.done;
        if (j == wv) m = Tile{wk.n0, wk.n1, wk.e1, wk.eb, live};
        if (live) wk.next(p);
    }
    return m;
}

struct Idx {
    int src, tgt;
    __device__ __forceinline__ void load(const CgParams& p, const Tile& t, int i) {
        const int ec = max(min(t.eb + i, t.e1 - 1), 0);     // clamp, never guard (slots past the group repeat its last edge)
        src = p.src[ec];
        tgt = p.tgt[ec];
    }
};

// B fragments gathered per edge: x rows of target / source, grad_out row of the target, and the target's row pointers
template <int C_>
struct Gathers {
    bf16x8 t[C_ / 16], s[C_ / 16], g[C_ / 32][2];
    int rp0, rp1;
    __device__ __forceinline__ void load(const CgParams& p, const Idx& id, int h) {
        const bf16_t* xt = static_cast<const bf16_t*>(p.x) + (int64_t)id.tgt * C_ + 8 * h;
        const bf16_t* xs = static_cast<const bf16_t*>(p.x) + (int64_t)id.src * C_ + 8 * h;
        const bf16_t* gt = static_cast<const bf16_t*>(p.gout) + (int64_t)id.tgt * C_ + 8 * h;
#pragma unroll
        for (int f = 0; f < C_ / 16; ++f) t[f] = *reinterpret_cast<const bf16x8*>(xt + 16 * f);
#pragma unroll
        for (int f = 0; f < C_ / 16; ++f) s[f] = *reinterpret_cast<const bf16x8*>(xs + 16 * f);
#pragma unroll
        for (int bc = 0; bc < C_ / 32; ++bc)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) g[bc][ks] = *reinterpret_cast<const bf16x8*>(gt + 32 * bc + 16 * ks);
        rp0 = p.rowptr[id.tgt];
        rp1 = p.rowptr[id.tgt + 1];
    }
};


}  // namespace ep
