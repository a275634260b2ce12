// neb.hip — the band force of a nudged elastic band (improved tangent: Henkelman & Jonsson, J. Chem. Phys. 113, 9978 (2000);
// climbing image: Henkelman, Uberuaga & Jonsson, 113, 9901) for every image of every band of a batch in ONE launch.
// No reference counterpart.  It is the first of the two launches of mdl_fire_step's band mode (include/mdl_hip.h states the
// definition; csrc/relax.hip makes the second, fire_kernel<false> over the bands).
//
//   neb_force_kernel   one workgroup of 256 lanes per image, looping over the image's atoms; all arithmetic fp64.
//                   Every lane finds the band of its image (a bisection of band_ptr), the climber of that band (a scan of the
//                   band's energies) and the tangent's weights (a, b) itself, from numbers every lane reads alike.
//                   pass 1: t+ = R(i+1) - R(i) and t- = R(i) - R(i-1) per atom, each wrapped to its minimum image in the cell of
//                           image i, and the five sums |t+|^2, |t-|^2, t+.t-, F.t+, F.t- in ONE block_reduce (struct_reduce.h);
//                   pass 2: t+ and t- again (the positions come from L2), F_band = F + g (a t+ + b t-) written as fp32.
//                   End images, images whose neighbours have another atom count, and fixed atoms get zero rows.
//                   Workgroup x < B also writes climber[x] (lane 0), so a band without images gets its -1.
// The bits: contraction is off and every fused multiply-add is written out, as in relax.hip; no atomics.
#include "struct_reduce.h"

namespace mdl {
namespace {

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the climber of the band of images [i0, i1): the interior image of largest energy, the lowest index on ties; -1 where the band
// has no interior image or does not climb
__device__ __forceinline__ int64_t band_climber(const float* energy, int64_t i0, int64_t i1, bool climb) {
    if (!climb || i1 - i0 < 3) return -1;
    int64_t best = i0 + 1;
    float e = energy[best];
    for (int64_t k = i0 + 2; k < i1 - 1; ++k)
        if (energy[k] > e) {
            e = energy[k];
            best = k;
        }
    return best;
}

// d wrapped to its minimum image: f = d C^-1, f_k -= rint(f_k) on the periodic axes, d = f C (rows of C are lattice vectors)
__device__ __forceinline__ void min_image(double& x, double& y, double& z, const double* C, const double* inv, int pb) {
#pragma clang fp contract(off)
    double f0 = x * inv[0] + y * inv[3] + z * inv[6];
    double f1 = x * inv[1] + y * inv[4] + z * inv[7];
    double f2 = x * inv[2] + y * inv[5] + z * inv[8];
    if (pb & 1) f0 -= rint(f0);
    if (pb & 2) f1 -= rint(f1);
    if (pb & 4) f2 -= rint(f2);
    x = f0 * C[0] + f1 * C[3] + f2 * C[6];
    y = f0 * C[1] + f1 * C[4] + f2 * C[7];
    z = f0 * C[2] + f1 * C[5] + f2 * C[8];
}

__global__ __launch_bounds__(STRUCT_THREADS) void neb_force_kernel(NebArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[STRUCT_WAVES][5];
    const int64_t s = blockIdx.x;
    if (s < a.B && threadIdx.x == 0) {
        const int64_t i0 = clamp_to(a.band_ptr[s], a.I), i1 = clamp_to(a.band_ptr[s + 1], a.I);
        a.climber[s] = (int32_t)band_climber(a.energy, i0, i1, a.climb[s] != 0);
    }
    if (s >= a.I) return;                                          // (every return is uniform over the workgroup)
    // the band of image s: the last b with band_ptr[b] <= s
    int64_t b = 0, top = a.B;
    while (top - b > 1) {
        const int64_t mid = b + (top - b) / 2;
        if (clamp_to(a.band_ptr[mid], a.I) <= s)
            b = mid;
        else
            top = mid;
    }
    const int64_t i0 = clamp_to(a.band_ptr[b], a.I), i1 = clamp_to(a.band_ptr[b + 1], a.I);
    if (s < i0 || s >= i1) return;                                 // an image of no band: nothing of it is written
    const int64_t a0 = clamp_to(a.image_ptr[s], a.N);
    int64_t a1 = clamp_to(a.image_ptr[s + 1], a.N);
    a1 = a1 < a0 ? a0 : a1;
    const int64_t n = a1 - a0;
    // a neighbour counts only with the atom count of this image: p0 + n == a0 <= N and a1 + n <= N, so every row read exists
    bool has_prev = s > i0, has_next = s + 1 < i1;
    int64_t p0 = 0;
    if (has_prev) {
        p0 = clamp_to(a.image_ptr[s - 1], a.N);
        has_prev = a0 - p0 == n;
    }
    if (has_next) has_next = clamp_to(a.image_ptr[s + 2], a.N) - a1 == n;
    const bool interior = has_prev && has_next;

    // the tangent's weights and the climber, from the band's energies
    double ca = 0.0, cb = 0.0;
    bool climbs = false;
    if (interior) {
        const double Ep = (double)a.energy[s - 1], E0 = (double)a.energy[s], En = (double)a.energy[s + 1];
        if (En > E0 && E0 > Ep) {
            ca = 1.0;
        } else if (En < E0 && E0 < Ep) {
            cb = 1.0;
        } else {
            const double dn = fabs(En - E0), dp = fabs(Ep - E0);
            const double hi = dn > dp ? dn : dp, lo = dn > dp ? dp : dn;
            ca = En > Ep ? hi : lo;
            cb = En > Ep ? lo : hi;
        }
        climbs = band_climber(a.energy, i0, i1, a.climb[b] != 0) == s;
    }
    double C[9], inv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) C[k] = a.cell[s * 9 + k];
    const double det = adjugate3(C, inv);
    const int pb = det != 0.0 ? (int)(a.pbc[s] & 7) : 0;           // no wrap where the cell has no volume
    if (pb)
#pragma unroll
        for (int k = 0; k < 9; ++k) inv[k] = inv[k] / det;
    const double* pos = a.pos;
    const float* force = a.force;
    const uint8_t* fixed = a.fixed;

    // pass 1: acc = (|t+|^2, |t-|^2, t+.t-, F.t+, F.t-); a fixed atom has F = 0
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t j = threadIdx.x; j < n; j += STRUCT_THREADS) {
        const int64_t i = a0 + j;
        const double rx = pos[i * 3 + 0], ry = pos[i * 3 + 1], rz = pos[i * 3 + 2];
        double px = 0.0, py = 0.0, pz = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
        if (has_next) {
            px = pos[(a1 + j) * 3 + 0] - rx;
            py = pos[(a1 + j) * 3 + 1] - ry;
            pz = pos[(a1 + j) * 3 + 2] - rz;
            if (pb) min_image(px, py, pz, C, inv, pb);
        }
        if (has_prev) {
            mx = rx - pos[(p0 + j) * 3 + 0];
            my = ry - pos[(p0 + j) * 3 + 1];
            mz = rz - pos[(p0 + j) * 3 + 2];
            if (pb) min_image(mx, my, mz, C, inv, pb);
        }
        double fx = 0.0, fy = 0.0, fz = 0.0;
        if (!(fixed && fixed[i])) {
            fx = (double)force[i * 3 + 0];
            fy = (double)force[i * 3 + 1];
            fz = (double)force[i * 3 + 2];
        }
        acc[0] += __builtin_fma(pz, pz, __builtin_fma(px, px, py * py));
        acc[1] += __builtin_fma(mz, mz, __builtin_fma(mx, mx, my * my));
        acc[2] += __builtin_fma(pz, mz, __builtin_fma(px, mx, py * my));
        acc[3] += __builtin_fma(fz, pz, __builtin_fma(fx, px, fy * py));
        acc[4] += __builtin_fma(fz, mz, __builtin_fma(fx, mx, fy * my));
    }
    block_reduce<5, 5>(acc, red);
    const double len_p = sqrt(acc[0]), len_m = sqrt(acc[1]);
    const double t2 = (ca * ca) * acc[0] + ((2.0 * ca) * cb) * acc[2] + (cb * cb) * acc[1];
    // F_band = F + g t: g = (-(F.t^) + k (|t+| - |t-|)) / |t|, for the climber -2 (F.t^) / |t|; no tangent (t2 is not > 0): g = 0
    double ft = 0.0, g = 0.0;
    if (interior && t2 > 0.0) {
        const double len_t = sqrt(t2);
        ft = (ca * acc[3] + cb * acc[4]) / len_t;
        g = (climbs ? -2.0 * ft : a.spring[b] * (len_p - len_m) - ft) / len_t;
    }
    if (threadIdx.x == 0) {
        a.tangent_force[s] = ft;
        a.seg_len[s] = len_m;                                      // 0 for the first image of a band: it has no t-
    }

    // pass 2: the rows of the image
    float* out = a.band_force;
    for (int64_t j = threadIdx.x; j < n; j += STRUCT_THREADS) {
        const int64_t i = a0 + j;
        double ox = 0.0, oy = 0.0, oz = 0.0;
        if (interior && !(fixed && fixed[i])) {
            const double rx = pos[i * 3 + 0], ry = pos[i * 3 + 1], rz = pos[i * 3 + 2];
            double px = pos[(a1 + j) * 3 + 0] - rx, py = pos[(a1 + j) * 3 + 1] - ry, pz = pos[(a1 + j) * 3 + 2] - rz;
            double mx = rx - pos[(p0 + j) * 3 + 0], my = ry - pos[(p0 + j) * 3 + 1], mz = rz - pos[(p0 + j) * 3 + 2];
            if (pb) {
                min_image(px, py, pz, C, inv, pb);
                min_image(mx, my, mz, C, inv, pb);
            }
            ox = (double)force[i * 3 + 0] + g * (ca * px + cb * mx);
            oy = (double)force[i * 3 + 1] + g * (ca * py + cb * my);
            oz = (double)force[i * 3 + 2] + g * (ca * pz + cb * mz);
        }
        out[i * 3 + 0] = (float)ox;
        out[i * 3 + 1] = (float)oy;
        out[i * 3 + 2] = (float)oz;
    }
}

}  // namespace

int neb_band_force(const char* fn, const NebArgs& a, hipStream_t stream) {
    MDL_REQUIRE(a.I >= 0, MDL_E_ARG, "%s: bad I=%lld", fn, (long long)a.I);
    MDL_REQUIRE(a.band_ptr && a.energy && a.cell && a.pbc && a.spring && a.climb && a.band_force && a.tangent_force && a.seg_len && a.climber,
                MDL_E_ARG, "%s: band mode (image_ptr given): null pointer", fn);
    MDL_REQUIRE((const void*)a.band_force != (const void*)a.force, MDL_E_ARG, "%s: band_force must not be force", fn);
    const int64_t grid = a.I > a.B ? a.I : a.B;                    // workgroup x: image x, and climber[x] of band x
    MDL_REQUIRE(grid < (1ll << 31), MDL_E_UNSUPP, "%s: I=%lld images overflow the grid", fn, (long long)a.I);
    hipLaunchKernelGGL(neb_force_kernel, dim3((unsigned)grid), dim3(STRUCT_THREADS), 0, stream, a);
    return check_launch(fn);
}

}  // namespace mdl
