// lpa_qed.hpp -- device helpers shared by the two LCFA sources: lpa_qed.hip (nonlinear Compton emission) and lpa_bw.hip
// (Breit-Wheeler pair production).  The counter-based generator, the global-memory field gather at a position, chi, the
// row lookup of the tables and the ballistic photon step.  All of it is charge-blind.
#pragma once
#include "lpa_common.hpp"

constexpr int QED_THREADS = 256;
constexpr int QED_MAX_CHI_N = 256;     // the 1-D rate table staged in LDS: 2 KB

// ---- Philox-4x32-10: the generator and the key / counter convention of lpa_collide.hip (pairing contract of the header)
struct U4 { uint32_t w[4]; };

__device__ inline U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{{c0, c1, c2, c3}};
}

__device__ inline double u01(uint32_t lo, uint32_t hi) {
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}

// ---- global-memory gather at a position in cells from node 0: the operations, in the order, of gather_global_2d / _3d
// (lpa_particles.hip, lpa_particles3d.hip; unified_pusher_2d.c:112-135, unified_pusher_3d.c:111-143,190-195)
template <bool D3>
struct GIdx { long r[3]; int c[3]; int d[3]; };

template <bool D3>
__device__ __forceinline__ void gidx(GIdx<D3> &o, int ix, int iy, int iz, const GridV &g) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        o.r[a] = (long)torus(ix - 1 + a + g.ng, g.NX) * g.NY * g.NZ;
        o.c[a] = torus(iy - 1 + a + g.ng, g.NY) * g.NZ;
        o.d[a] = D3 ? torus(iz - 1 + a + g.ng, g.NZ) : 0;
    }
}

__device__ __forceinline__ double gather9(const double *__restrict__ f, const GIdx<false> &o, const double fx[3],
                                          const double fy[3]) {
    return fy[0] * (fx[0] * f[o.r[0] + o.c[0]] + fx[1] * f[o.r[1] + o.c[0]] + fx[2] * f[o.r[2] + o.c[0]]) +
           fy[1] * (fx[0] * f[o.r[0] + o.c[1]] + fx[1] * f[o.r[1] + o.c[1]] + fx[2] * f[o.r[2] + o.c[1]]) +
           fy[2] * (fx[0] * f[o.r[0] + o.c[2]] + fx[1] * f[o.r[1] + o.c[2]] + fx[2] * f[o.r[2] + o.c[2]]);
}

__device__ __forceinline__ double gather27(const double *__restrict__ f, const GIdx<true> &o, const double fx[3],
                                           const double fy[3], const double fz[3]) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double pl = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const long b = o.c[j] + o.d[k];
            pl += fy[j] * (fx[0] * f[o.r[0] + b] + fx[1] * f[o.r[1] + b] + fx[2] * f[o.r[2] + b]);
        }
        acc += fz[k] * pl;
    }
    return acc;
}

template <bool D3>
__device__ __forceinline__ void gather_eb(const GridV &g, double xo, double yo, double zo, double eb[6]) {
    const int ix1 = ifloor(xo + 0.5), ix2 = ifloor(xo), iy1 = ifloor(yo + 0.5), iy2 = ifloor(yo);
    double gx[3], hx[3], gy[3], hy[3];
    tsc3(ix1 - xo, gx); tsc3(ix2 - xo + 0.5, hx);
    tsc3(iy1 - yo, gy); tsc3(iy2 - yo + 0.5, hy);
    GIdx<D3> a;
    if constexpr (!D3) {
        gidx<false>(a, ix2, iy1, 0, g); eb[0] = gather9(g.ex, a, hx, gy); eb[4] = gather9(g.by, a, hx, gy);
        gidx<false>(a, ix1, iy2, 0, g); eb[1] = gather9(g.ey, a, gx, hy); eb[3] = gather9(g.bx, a, gx, hy);
        gidx<false>(a, ix1, iy1, 0, g); eb[2] = gather9(g.ez, a, gx, gy);
        gidx<false>(a, ix2, iy2, 0, g); eb[5] = gather9(g.bz, a, hx, hy);
    } else {
        const int iz1 = ifloor(zo + 0.5), iz2 = ifloor(zo);
        double gz[3], hz[3];
        tsc3(iz1 - zo, gz); tsc3(iz2 - zo + 0.5, hz);
        gidx<true>(a, ix2, iy1, iz1, g); eb[0] = gather27(g.ex, a, hx, gy, gz);
        gidx<true>(a, ix1, iy2, iz1, g); eb[1] = gather27(g.ey, a, gx, hy, gz);
        gidx<true>(a, ix1, iy1, iz2, g); eb[2] = gather27(g.ez, a, gx, gy, hz);
        gidx<true>(a, ix1, iy2, iz2, g); eb[3] = gather27(g.bx, a, gx, hy, hz);
        gidx<true>(a, ix2, iy1, iz2, g); eb[4] = gather27(g.by, a, hx, gy, hz);
        gidx<true>(a, ix2, iy2, iz1, g); eb[5] = gather27(g.bz, a, hx, hy, gz);
    }
}

// ---- the tables and the step as the event kernels see them -----------------------------------------------------------
struct QedK {
    double dt, cdt_half, chi_factor, chi_min;
    const double *rate, *cum;
    int chi_n, delta_n;
    double lc_min, lc_max, dlc, ld_min, dld;
    uint32_t k0, k1, itime;
    int stored_eb;
    double *chi_out;
};

static inline QedK make_qedk(const lpa_qed_params *qp) {
    QedK k;
    k.dt = qp->dt; k.cdt_half = LPA_C * 0.5 * qp->dt; k.chi_factor = qp->chi_factor; k.chi_min = qp->chi_min;
    k.rate = qp->rate; k.cum = qp->cum; k.chi_n = qp->chi_n; k.delta_n = qp->delta_n;
    k.lc_min = qp->log_chi_min; k.lc_max = qp->log_chi_max;
    k.dlc = (qp->log_chi_max - qp->log_chi_min) / (qp->chi_n - 1);
    k.ld_min = qp->log_delta_min; k.dld = (qp->log_delta_max - qp->log_delta_min) / (qp->delta_n - 1);
    k.k0 = (uint32_t)qp->seed; k.k1 = (uint32_t)(qp->seed >> 32); k.itime = qp->itime;
    k.stored_eb = (qp->flags & LPA_QED_STORED_EB) != 0; k.chi_out = qp->chi_out;
    return k;
}

static inline bool qed_tables_ok(const lpa_qed_params *qp) {
    return qp->rate && qp->cum && qp->chi_n >= 2 && qp->chi_n <= QED_MAX_CHI_N && qp->delta_n >= 2 &&
           qp->log_chi_max > qp->log_chi_min && qp->log_delta_max > qp->log_delta_min && qp->dt > 0;
}

// calculate_chi_inline (core/qed/inline.py:5-13)
__device__ __forceinline__ double chi_of(const double eb[6], double ux, double uy, double uz, double ig, double factor) {
    const double c = LPA_C, gamma = 1.0 / ig;
    const double fx = gamma * eb[0] + (uy * eb[5] - uz * eb[4]) * c;
    const double fy = gamma * eb[1] + (uz * eb[3] - ux * eb[5]) * c;
    const double fz = gamma * eb[2] + (ux * eb[4] - uy * eb[3]) * c;
    const double ue = ux * eb[0] + uy * eb[1] + uz * eb[2];
    return factor * sqrt(fx * fx + fy * fy + fz * fz - ue * ue);
}

// row index and blend weight of log10(chi) in the table: _get_chi_idx (optical_depth_tables.py:32-42), clamped above
// the last node (there the reference reads one row past its table)
__device__ __forceinline__ int chi_row(const QedK &k, double chi, double &lc, double &left) {
    lc = log10(chi);
    lc = lc > k.lc_max ? k.lc_max : lc;
    int idx = ifloor((lc - k.lc_min) / k.dlc);
    idx = idx < 0 ? 0 : (idx > k.chi_n - 2 ? k.chi_n - 2 : idx);
    left = k.lc_min + idx * k.dlc;
    return idx;
}

// ---- photons move ballistically (the reference's PhotonPusher is a stub: momenta never change) -----------------------
struct PhotonK {
    double cdt;
    int wrap;
    double lo[3], hi[3], alo[3], ahi[3];
};

static inline PhotonK make_photonk(const lpa_push_params *pp, double dt) {
    PhotonK k;
    k.cdt = LPA_C * dt; k.wrap = pp->wrap;
    for (int a = 0; a < 3; a++) { k.lo[a] = pp->lo[a]; k.hi[a] = pp->hi[a]; k.alo[a] = pp->alo[a]; k.ahi[a] = pp->ahi[a]; }
    return k;
}

__device__ __forceinline__ double fold(double v, double lo, double hi) {     // sync_particles_2d.c:168-182, self neighbour
    const double L = hi - lo;
    if (v > hi) v -= L;
    if (v < lo) v += L;
    return v;
}

// r += c dt u / |u| on the store's axes, the periodic fold, the open-face rule; true: beyond an open face
// (mark_out_of_bound_as_dead).  The one statement of the photon step: k_push_photons and k_bw_push_event both call it
template <bool D3>
__device__ __forceinline__ bool photon_advance(const PhotonK &k, double r[3], const double u[3], double ig) {
    const double s = k.cdt * ig;
    bool dead = false;
#pragma unroll
    for (int a = 0; a < (D3 ? 3 : 2); a++) {
        r[a] += s * u[a];
        if (k.wrap & (1 << a)) r[a] = fold(r[a], k.lo[a], k.hi[a]);
        dead = dead || ((k.wrap & (LPA_ABSORB_X << a)) && (r[a] < k.alo[a] || r[a] > k.ahi[a]));
    }
    return dead;
}
