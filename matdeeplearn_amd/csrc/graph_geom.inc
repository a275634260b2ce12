// graph_geom.inc — the minimum-image geometry of a batch of structures, shared by graph_build.hip (the graph builder) and
// edge_geom.hip (distances and unit vectors of given edges, and their backward): per structure the reduced cell, the completed
// basis, its inverse and the image shifts (graph_geom_kernel), and per atom pair the minimum-image r^2 (min_image_r2), in the
// operation order of graph.distance_matrix.  Both translation units switch FMA contraction off (pragma + -ffp-contract=off), so a pair's distance is
// bitwise the same in both.  Included inside namespace mdl { namespace { ... } }.
struct GraphGeom {
    double inv[9];                             // inverse of the completed basis, row-major
    double full[9];                            // completed basis (rows: reduced periodic vectors + unit complements)
    double img[27 * 3];                        // image shifts (a c0 + b c1) + c c2 of the reduced cell
    int32_t nimg;                              // 3^(periodic axes); 0: non-periodic
    int32_t pbc;
};

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// graph.reduce_cell + the basis completion and inverse of graph.distance_matrix, one lane per structure
__global__ __launch_bounds__(64) void graph_geom_kernel(const double* __restrict__ cell, const int32_t* __restrict__ pbc,
                                                        int64_t G, GraphGeom* __restrict__ geom) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int mask = pbc[g] & 7;
    GraphGeom* out = geom + g;
    out->pbc = mask;
    if (mask == 0) {
        out->nimg = 0;
        return;
    }
    double c[3][3];
    for (int r = 0; r < 3; ++r)
        for (int m = 0; m < 3; ++m) c[r][m] = cell[g * 9 + r * 3 + m];
    int per[3], np_ = 0, free_[3], nf = 0;
    for (int k = 0; k < 3; ++k) {
        if (mask >> k & 1) per[np_++] = k;
        else free_[nf++] = k;
    }
    // reduce_cell
    for (int it = 0; it < 64; ++it) {
        bool changed = false;
        for (int ia = 0; ia < np_; ++ia)
            for (int ib = 0; ib < np_; ++ib) {
                const int a = per[ia], b = per[ib];
                if (a == b) continue;
                const double nb = dot3(c[b], c[b]);
                if (nb < 1e-24) continue;
                const double k = rint(dot3(c[a], c[b]) / nb);
                if (k != 0.0) {
                    double nw[3];
                    for (int m = 0; m < 3; ++m) nw[m] = c[a][m] - k * c[b][m];
                    if (dot3(nw, nw) < dot3(c[a], c[a]) - 1e-12) {
                        for (int m = 0; m < 3; ++m) c[a][m] = nw[m];
                        changed = true;
                    }
                }
            }
        if (!changed) break;
    }
    // complete the basis: non-periodic directions orthogonal to the periodic ones
    double f[3][3];
    for (int r = 0; r < 3; ++r)
        for (int m = 0; m < 3; ++m) f[r][m] = c[r][m];
    if (np_ == 2) {
        double v[3];
        cross3(c[per[0]], c[per[1]], v);
        const double s = sqrt(dot3(v, v));
        for (int m = 0; m < 3; ++m) f[free_[0]][m] = v[m] / s;
    } else if (np_ == 1) {
        const double* p = c[per[0]];
        const double s = sqrt(dot3(p, p));
        double u[3], e[3] = {0.0, 0.0, 0.0}, v1[3], v2[3];
        for (int m = 0; m < 3; ++m) u[m] = p[m] / s;
        int am = 0;                                            // np.argmin(np.abs(u)): first minimum
        for (int m = 1; m < 3; ++m)
            if (fabs(u[m]) < fabs(u[am])) am = m;
        e[am] = 1.0;
        cross3(u, e, v1);
        const double s1 = sqrt(dot3(v1, v1));
        for (int m = 0; m < 3; ++m) v1[m] /= s1;
        cross3(u, v1, v2);
        for (int m = 0; m < 3; ++m) {
            f[free_[0]][m] = v1[m];
            f[free_[1]][m] = v2[m];
        }
    }
    // inverse: exact reciprocals for one non-zero per row and column (what LAPACK returns there), else the adjugate
    double inv[3][3];
    int col_of[3], ncol[3] = {0, 0, 0};
    bool monomial = true;
    for (int r = 0; r < 3; ++r) {
        int nz = 0;
        for (int m = 0; m < 3; ++m)
            if (f[r][m] != 0.0) {
                ++nz;
                col_of[r] = m;
                ++ncol[m];
            }
        monomial = monomial && nz == 1;
    }
    monomial = monomial && ncol[0] == 1 && ncol[1] == 1 && ncol[2] == 1;
    if (monomial) {
        for (int r = 0; r < 3; ++r)
            for (int m = 0; m < 3; ++m) inv[r][m] = 0.0;
        for (int r = 0; r < 3; ++r) inv[col_of[r]][r] = 1.0 / f[r][col_of[r]];
    } else {
        double adj[3][3];
        for (int r = 0; r < 3; ++r)
            for (int m = 0; m < 3; ++m) {
                const int r1 = (m + 1) % 3, r2 = (m + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
                adj[r][m] = f[r1][c1] * f[r2][c2] - f[r1][c2] * f[r2][c1];     // cofactor (m, r)
            }
        const double det = (f[0][0] * adj[0][0] + f[0][1] * adj[1][0]) + f[0][2] * adj[2][0];
        for (int r = 0; r < 3; ++r)
            for (int m = 0; m < 3; ++m) inv[r][m] = adj[r][m] / det;
    }
    for (int r = 0; r < 3; ++r)
        for (int m = 0; m < 3; ++m) {
            out->inv[r * 3 + m] = inv[r][m];
            out->full[r * 3 + m] = f[r][m];
        }
    // image shifts over the periodic axes, (a c0 + b c1) + c c2 as the host forms them
    int n = 0;
    for (int a = -1; a <= 1; ++a) {
        if (a != 0 && !(mask & 1)) continue;
        for (int b = -1; b <= 1; ++b) {
            if (b != 0 && !(mask & 2)) continue;
            for (int cc = -1; cc <= 1; ++cc) {
                if (cc != 0 && !(mask & 4)) continue;
                for (int m = 0; m < 3; ++m)
                    out->img[n * 3 + m] = ((double)a * c[0][m] + (double)b * c[1][m]) + (double)cc * c[2][m];
                ++n;
            }
        }
    }
    out->nimg = n;
}

// r^2 of the minimum image of the difference (dx, dy, dz) = p_j - p_i in structure `gm` (nimg == 0: the plain difference).
// WITH_VEC: v receives the displacement of that image (the first of the images that reach the minimum, as the running `<` keeps it).
template <bool WITH_VEC>
__device__ __forceinline__ double min_image_r2(const GraphGeom* __restrict__ gm, int nimg, int mask, double dx, double dy, double dz,
                                               double* v) {
    if (nimg == 0) {
        if (WITH_VEC) { v[0] = dx; v[1] = dy; v[2] = dz; }
        return (dx * dx + dy * dy) + dz * dz;
    }
    double fr[3];
    for (int m = 0; m < 3; ++m) {
        fr[m] = (dx * gm->inv[0 * 3 + m] + dy * gm->inv[1 * 3 + m]) + dz * gm->inv[2 * 3 + m];
        if (mask >> m & 1) fr[m] = fr[m] - rint(fr[m]);
    }
    double e[3];
    for (int m = 0; m < 3; ++m) e[m] = (fr[0] * gm->full[0 * 3 + m] + fr[1] * gm->full[1 * 3 + m]) + fr[2] * gm->full[2 * 3 + m];
    double r2 = __builtin_inf();
    for (int im = 0; im < nimg; ++im) {
        const double vx = e[0] + gm->img[im * 3 + 0], vy = e[1] + gm->img[im * 3 + 1], vz = e[2] + gm->img[im * 3 + 2];
        const double q = (vx * vx + vy * vy) + vz * vz;
        if (WITH_VEC && q < r2) { v[0] = vx; v[1] = vy; v[2] = vz; }
        r2 = q < r2 ? q : r2;
    }
    return r2;
}
