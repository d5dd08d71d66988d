// lpa_collide.hip -- relativistic binary Coulomb collisions on a tile-binned store (gfx950, wave64, FP64).
//
// Replaces core/collision/cpu.py (intra_ / inter_collision_patches, debye_length_patches,
// constrain_debye_length_patches) and the pairing iterators of core/collision/utils.py:233-419.  The reference
// shuffles every cell with a serial Fisher-Yates walk of a stateful generator; here the pairing is a pure function
// of the particle ids and a counter-based generator (the pairing contract of include/lambdapic_amd.h), so the result
// does not depend on the order of the store and a restart needs no generator state.
//
// Decomposition: a workgroup per 256-cell tile, a wave per cell, a lane per pair.
//   1. bin     the tile's slots of each species are counted per cell (LDS atomics), the counts scanned, and
//              (key, id, slot) of every live particle written to the cell's list in the workspace -- the only
//              assumption about the store is lpa_tiling.tile_off;
//   2. order   a wave takes a cell: a list of up to 64 entries is sorted in registers (bitonic network on
//              ds_bpermute lane exchanges), a longer one by a same-direction bitonic network on the staged copy;
//   3. collide ux uy uz w of the cell's particles are staged in the wave's LDS slice once, the disjoint pairs of a
//              round run one per lane, and the momenta go back once.  Intra-species: all pairs but the closing
//              one of an odd cell, then that one.  Inter-species: lane j owns the canonical particle j (mod 64)
//              through all its rounds, so no round waits for another.
// A cell whose two lists exceed the wave's LDS slice (CL_WAVE_ENTRIES) runs the same code on the workspace lists and
// the particle arrays (global path).
#include "lpa_common.hpp"
#include "lpa_cellsort.hpp"

namespace {

constexpr int CL_THREADS = 256, CL_WAVES = CL_THREADS / 64;
constexpr int CL_WAVE_ENTRIES = 256;   // entries (both species) of a cell that fit the wave's LDS slice: 52 bytes each

// ---- Philox-4x32-10 (Salmon et al., SC'11) ---------------------------------------------------------------------------
struct U4 { uint32_t w[4]; };

__host__ __device__ inline U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{{c0, c1, c2, c3}};
}

__host__ __device__ inline double u01(uint32_t lo, uint32_t hi) {
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}

// ---- kernel arguments ------------------------------------------------------------------------------------------------
struct CollK {
    Geom g;
    PartV p[2];
    const int32_t *toff[2];
    long nsort[2], base[2];            // tile-ordered slots of each side; start of its region in the workspace lists
    double m[2], q[2];
    int inter;
    double dt, lnl, cell_vol, eps0;
    const double *inv_d2;
    uint32_t k0, k1, itime, pidx;
    uint32_t *skipped;
    unsigned long long *ws_key, *ws_id;
    uint32_t *ws_slot;
};

// global cell index of cell `c` of tile `t`, -1 beyond the grid
template <bool D3>
__device__ __forceinline__ int global_cell(const Geom &g, int t, int c) {
    if (!D3) {
        const int ix = (t / g.tiles_y) * LPA_TILE_X + c / LPA_TILE_Y, iy = (t % g.tiles_y) * LPA_TILE_Y + c % LPA_TILE_Y;
        return ix < g.nx && iy < g.ny ? ix * g.ny + iy : -1;
    }
    const int tz = t % g.tiles_z, ty = (t / g.tiles_z) % g.tiles_y, tx = t / (g.tiles_z * g.tiles_y);
    const int ix = tx * LPA_TILE3_X + c / (LPA_TILE3_Y * LPA_TILE3_Z), iy = ty * LPA_TILE3_Y + (c / LPA_TILE3_Z) % LPA_TILE3_Y,
              iz = tz * LPA_TILE3_Z + c % LPA_TILE3_Z;
    return ix < g.nx && iy < g.ny && iz < g.nz ? (ix * g.ny + iy) * g.nz + iz : -1;
}

// ---- the pair: collision_data, varying_lnLambda, coulomb_scattering, rotate_momentum, boost_to_lab and the accept rule
// of collision_kernel (core/collision/utils.py:26-205, cpu.py:252-278,374-428), operation for operation; gamma comes
// from the momenta.  Returns bit 0 / bit 1 = particle 1 / 2 was updated.
struct PairK { double m1, q1, m2, q2, cell_vol, eps0, lnl, inv_d2; };

__device__ __forceinline__ void boost_to_lab(double pxc, double pyc, double pzc, double gcp, double m, double vxc, double vyc,
                                             double vzc, double vc2, double gc, double inv_mc, double u[3]) {
    const double vdotp = vxc * pxc + vyc * pyc + vzc * pzc;
    const double fac = vc2 > 0 ? (gc - 1) / vc2 : 0.0;
    const double f = fac * vdotp + m * gcp * gc;
    u[0] = (pxc + vxc * f) * inv_mc; u[1] = (pyc + vyc * f) * inv_mc; u[2] = (pzc + vzc * f) * inv_mc;
}

__device__ int collide_pair(const PairK &k, double u1[3], double w1, double u2[3], double w2, double w_corr, double dt,
                            double u_theta, double phi, double u_acc) {
    const double c = LPA_C, c2 = c * c, pi = 3.141592653589793, planck = 6.62607015e-34;
    const double m1 = k.m1, m2 = k.m2;
    w1 *= w_corr; w2 *= w_corr;
    const double w_max = fmax(w1, w2);
    const double g1 = sqrt(1 + u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]), ig1 = 1 / g1;
    const double g2 = sqrt(1 + u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]), ig2 = 1 / g2;
    const double px1 = u1[0] * m1 * c, py1 = u1[1] * m1 * c, pz1 = u1[2] * m1 * c;
    const double px2 = u2[0] * m2 * c, py2 = u2[1] * m2 * c, pz2 = u2[2] * m2 * c;
    const double vx1 = u1[0] * ig1 * c, vy1 = u1[1] * ig1 * c, vz1 = u1[2] * ig1 * c;
    const double vx2 = u2[0] * ig2 * c, vy2 = u2[1] * ig2 * c, vz2 = u2[2] * ig2 * c;
    const double msum = g1 * m1 + g2 * m2;
    const double vxc = (px1 + px2) / msum, vyc = (py1 + py2) / msum, vzc = (pz1 + pz2) / msum;
    const double vc2 = vxc * vxc + vyc * vyc + vzc * vzc;
    const double gc = 1.0 / sqrt(1 - vc2 / c2);
    const double fac = vc2 > 0 ? (gc - 1) / vc2 : 0.0;
    const double v1dot = vx1 * vxc + vy1 * vyc + vz1 * vzc, v2dot = vxc * vx2 + vyc * vy2 + vzc * vz2;
    const double f1 = (fac * v1dot - gc) * m1 * g1;
    const double pxc = px1 + f1 * vxc, pyc = py1 + f1 * vyc, pzc = pz1 + f1 * vzc;
    const double pc = sqrt(pxc * pxc + pyc * pyc + pzc * pzc);
    if (pc == 0) return 0;                                        // a pair at rest
    const double g1c = (1 - v1dot / c2) * gc * g1, g2c = (1 - v2dot / c2) * gc * g2;
    const double pperp = sqrt(pxc * pxc + pyc * pyc);
    const double q1q2 = k.q1 * k.q2;
    const double shape = m1 * g1c * m2 * g2c / (pc * pc) * c2 + 1;
    double lnl = k.lnl;
    if (!(lnl > 0)) {                                             // varying_lnLambda
        const double b0 = fabs(q1q2) / (4 * pi * k.eps0 * c2) * gc / (m1 * g1c + m2 * g2c) * shape;
        const double bmin = fmax(planck / 2 / pc, b0);
        lnl = k.inv_d2 > 0 ? fmax(2.0, 0.5 * log(1 + (1 / k.inv_d2) / (bmin * bmin))) : 2.0;
    }
    const double s = w_max / k.cell_vol * dt * (lnl * (q1q2 * q1q2)) / (4 * pi * k.eps0 * k.eps0 * c2 * c2 * m1 * g1 * m2 * g2) *
                     (gc * pc) / msum * (shape * shape);
    double cosx, sinx;
    if (s < 4) {                                                  // Nanbu's fit
        const double alpha = 0.37 * s - 0.005 * s * s - 0.0064 * s * s * s;
        const double sin2 = alpha * u_theta / sqrt((1 - u_theta) + alpha * alpha * u_theta);
        cosx = 1. - 2. * sin2;
        sinx = 2. * sqrt(sin2 * (1. - sin2));
    } else {                                                      // isotropic
        cosx = 2. * u_theta - 1.;
        sinx = sqrt(1. - cosx * cosx);
    }
    const double scp = sinx * cos(phi), ssp = sinx * sin(phi);
    double nx, ny, nz;
    if (pperp > 1.e-10 * pc) {
        nx = (pxc * pzc * scp - pyc * pc * ssp) / pperp + pxc * cosx;
        ny = (pyc * pzc * scp + pxc * pc * ssp) / pperp + pyc * cosx;
        nz = -pperp * scp + pzc * cosx;
    } else {
        nx = pc * scp; ny = pc * ssp; nz = pc * cosx;
    }
    int upd = 0;
    if (w2 / w_max > u_acc) {
        boost_to_lab(nx, ny, nz, g1c, m1, vxc, vyc, vzc, vc2, gc, 1 / m1 / c, u1);
        upd |= 1;
    }
    if (w1 / w_max > u_acc) {
        boost_to_lab(-nx, -ny, -nz, g2c, m2, vxc, vyc, vzc, vc2, gc, 1 / m2 / c, u2);
        upd |= 2;
    }
    return upd;
}

// one species' particles of a cell as the pairs see them: LDS staging (index = position in the sorted list) or the
// particle arrays through the list's slots
template <bool LDS>
struct Side {
    double *ux, *uy, *uz, *w, *ig;      // ig: always the store's array (or NULL)
    const uint32_t *slot;               // sorted list of the cell
    __device__ __forceinline__ long at(int i) const { return LDS ? (long)i : (long)slot[i]; }
};

template <bool LDS>
__device__ __forceinline__ void run_pair(const CollK &k, const PairK &pk, const Side<LDS> &A, int ia, const Side<LDS> &B,
                                         int ib, uint32_t i, uint32_t gc, double w_corr, double dt) {
    const long a = A.at(ia), b = B.at(ib);
    double u1[3] = {A.ux[a], A.uy[a], A.uz[a]}, u2[3] = {B.ux[b], B.uy[b], B.uz[b]};
    const U4 r2 = philox(i, gc, k.itime, (k.pidx << 8) | 2u, k.k0, k.k1);
    const U4 r3 = philox(i, gc, k.itime, (k.pidx << 8) | 3u, k.k0, k.k1);
    const int upd = collide_pair(pk, u1, A.w[a], u2, B.w[b], w_corr, dt, u01(r2.w[0], r2.w[1]),
                                 2 * 3.141592653589793 * u01(r2.w[2], r2.w[3]), u01(r3.w[0], r3.w[1]));
    if (upd & 1) {
        A.ux[a] = u1[0]; A.uy[a] = u1[1]; A.uz[a] = u1[2];
        if (A.ig) A.ig[A.slot[ia]] = 1 / sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2] + 1);
    }
    if (upd & 2) {
        B.ux[b] = u2[0]; B.uy[b] = u2[1]; B.uz[b] = u2[2];
        if (B.ig) B.ig[B.slot[ib]] = 1 / sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2] + 1);
    }
}

// all pairs of one cell, by one wave; the lists are sorted
template <bool LDS>
__device__ __forceinline__ void run_cell(const CollK &k, const PairK &pk, const Side<LDS> &A, int na, const Side<LDS> &B,
                                         int nb, uint32_t gc, int lane) {
    if (!k.inter) {
        // utils.py:233-293: pairs (s[2i], s[2i+1]); an odd cell closes with (s[n-1], s[0]), first and last pair at half weight
        const int npairs = (na + 1) / 2, full = na / 2;
        const double dt = k.dt * (2 * npairs - 1);
        for (int i = lane; i < full; i += 64)
            run_pair<LDS>(k, pk, A, 2 * i, A, 2 * i + 1, (uint32_t)i, gc, (na & 1) && i == 0 ? 0.5 : 1.0, dt);
        if (na & 1) {
            wave_sync();
            if (lane == 0) run_pair<LDS>(k, pk, A, na - 1, A, 0, (uint32_t)(npairs - 1), gc, 0.5, dt);
        }
        return;
    }
    // utils.py:327-419: pair i = (shuffled[i], canonical[i mod nmin]); a lane keeps canonical particle j through its rounds
    const bool a_shuffled = na >= nb;
    const int nmax = a_shuffled ? na : nb, nmin = a_shuffled ? nb : na;
    const int rep = nmax / nmin, rem = nmax % nmin;
    const double dt = k.dt * nmax;
    for (int j = lane; j < nmin; j += 64) {
        const double w_corr = j < rem ? 1.0 / (rep + 1) : 1.0 / rep;
        for (int i = j; i < nmax; i += nmin)
            run_pair<LDS>(k, pk, A, a_shuffled ? i : j, B, a_shuffled ? j : i, (uint32_t)i, gc, w_corr, dt);
    }
}

template <bool D3>
__global__ void __launch_bounds__(CL_THREADS) k_collide(CollK k) {
    __shared__ int s_cnt[2][CL_CELLS], s_off[2][CL_CELLS];
    __shared__ unsigned long long s_key[CL_WAVES][CL_WAVE_ENTRIES], s_id[CL_WAVES][CL_WAVE_ENTRIES];
    __shared__ uint32_t s_slot[CL_WAVES][CL_WAVE_ENTRIES];
    __shared__ double s_u[CL_WAVES][4][CL_WAVE_ENTRIES];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nside = k.inter ? 2 : 1;
    s_cnt[0][tid] = 0; s_cnt[1][tid] = 0;
    __syncthreads();
    // ---- 1. bin: count
    uint32_t skipped = 0;
    long lo[2], hi[2];
    for (int s = 0; s < nside; s++) {
        lo[s] = k.toff[s][t]; hi[s] = k.toff[s][t + 1];
        hi[s] = hi[s] < k.nsort[s] ? hi[s] : k.nsort[s];
        for (long ip = lo[s] + tid; ip < hi[s]; ip += CL_THREADS) {
            const int ck = cell_of<D3>(k.p[s], ip, k.g);
            if (ck < 0) continue;
            if ((ck >> 8) != t) { skipped++; continue; }
            atomicAdd(&s_cnt[s][ck & 255], 1);
        }
    }
    if (skipped && k.skipped) atomicAdd(k.skipped, skipped);
    __syncthreads();
    // scan (inclusive, both sides at once), then shifted to the exclusive offsets
    const int c0 = s_cnt[0][tid], c1 = s_cnt[1][tid];
    s_off[0][tid] = c0; s_off[1][tid] = c1;
    __syncthreads();
    for (int d = 1; d < CL_CELLS; d <<= 1) {
        const int a0 = tid >= d ? s_off[0][tid - d] : 0, a1 = tid >= d ? s_off[1][tid - d] : 0;
        __syncthreads();
        s_off[0][tid] += a0; s_off[1][tid] += a1;
        __syncthreads();
    }
    s_off[0][tid] -= c0; s_off[1][tid] -= c1;
    __syncthreads();
    // ---- fill: (key, id, slot) into the cell's list; the fill cursor is the offset itself (it ends one past the cell)
    for (int s = 0; s < nside; s++) {
        const long base = k.base[s] + lo[s];
        for (long ip = lo[s] + tid; ip < hi[s]; ip += CL_THREADS) {
            const int ck = cell_of<D3>(k.p[s], ip, k.g);
            if (ck < 0 || (ck >> 8) != t) continue;
            const int c = ck & 255;
            const long o = base + atomicAdd(&s_off[s][c], 1);
            const unsigned long long id = k.p[s].id[ip];
            // shuffle key of the side that is shuffled in this cell (ties: species a), 0 = canonical order
            const bool shuffled = !k.inter || (s == 0 ? s_cnt[0][c] >= s_cnt[1][c] : s_cnt[1][c] > s_cnt[0][c]);
            unsigned long long key = 0;
            if (shuffled) {
                const U4 r = philox((uint32_t)id, (uint32_t)(id >> 32), k.itime, (k.pidx << 8) | (uint32_t)s, k.k0, k.k1);
                key = ((unsigned long long)r.w[1] << 32) | r.w[0];
            }
            k.ws_key[o] = key; k.ws_id[o] = id; k.ws_slot[o] = (uint32_t)ip;
        }
    }
    __syncthreads();
    // ---- 2 + 3. a wave per cell
    PairK pk;
    pk.m1 = k.m[0]; pk.q1 = k.q[0]; pk.m2 = k.m[k.inter]; pk.q2 = k.q[k.inter];
    pk.cell_vol = k.cell_vol; pk.eps0 = k.eps0; pk.lnl = k.lnl; pk.inv_d2 = 0.0;
    for (int c = wv; c < CL_CELLS; c += CL_WAVES) {
        const int na = s_cnt[0][c], nb = k.inter ? s_cnt[1][c] : 0;
        if (k.inter ? (na == 0 || nb == 0) : na < 2) continue;
        const int gcell = global_cell<D3>(k.g, t, c);
        if (gcell < 0) continue;
        if (!(k.lnl > 0)) pk.inv_d2 = k.inv_d2[gcell];
        const long ga = k.base[0] + lo[0] + s_off[0][c] - na, gb = k.inter ? k.base[1] + lo[1] + s_off[1][c] - nb : 0;
        const PartV &pa = k.p[0], &pb = k.p[k.inter];
        if (na + nb <= CL_WAVE_ENTRIES) {
            for (int i = lane; i < na + nb; i += 64) {
                const long o = i < na ? ga + i : gb + (i - na);
                s_key[wv][i] = k.ws_key[o]; s_id[wv][i] = k.ws_id[o]; s_slot[wv][i] = k.ws_slot[o];
            }
            wave_sync();
            sort_list(s_key[wv], s_id[wv], s_slot[wv], na, lane);
            sort_list(s_key[wv] + na, s_id[wv] + na, s_slot[wv] + na, nb, lane);
            wave_sync();
            for (int i = lane; i < na + nb; i += 64) {
                const PartV &p = i < na ? pa : pb;
                const long ip = s_slot[wv][i];
                s_u[wv][0][i] = p.ux[ip]; s_u[wv][1][i] = p.uy[ip]; s_u[wv][2][i] = p.uz[ip]; s_u[wv][3][i] = p.w[ip];
            }
            wave_sync();
            const Side<true> A{s_u[wv][0], s_u[wv][1], s_u[wv][2], s_u[wv][3], pa.ig, s_slot[wv]};
            const Side<true> B{s_u[wv][0] + na, s_u[wv][1] + na, s_u[wv][2] + na, s_u[wv][3] + na, pb.ig, s_slot[wv] + na};
            run_cell<true>(k, pk, A, na, k.inter ? B : A, nb, (uint32_t)gcell, lane);
            wave_sync();
            for (int i = lane; i < na + nb; i += 64) {
                const PartV &p = i < na ? pa : pb;
                const long ip = s_slot[wv][i];
                p.ux[ip] = s_u[wv][0][i]; p.uy[ip] = s_u[wv][1][i]; p.uz[ip] = s_u[wv][2][i];
            }
            wave_sync();
        } else {
            sort_list(k.ws_key + ga, k.ws_id + ga, k.ws_slot + ga, na, lane);
            if (k.inter) sort_list(k.ws_key + gb, k.ws_id + gb, k.ws_slot + gb, nb, lane);
            wave_sync();
            const Side<false> A{pa.ux, pa.uy, pa.uz, pa.w, pa.ig, k.ws_slot + ga};
            const Side<false> B{pb.ux, pb.uy, pb.uz, pb.w, pb.ig, k.ws_slot + gb};
            run_cell<false>(k, pk, A, na, k.inter ? B : A, nb, (uint32_t)gcell, lane);
            wave_sync();
        }
    }
}

// ---- Debye length (debye_length_patches + constrain_debye_length_patches, core/collision/cpu.py:136-250): a workgroup
// per tile sums w, w u and w u'^2 / sqrt(1 + u'^2) per cell with LDS atomics; thread c finishes cell c
struct DebyeK {
    Geom g;
    PartV p;
    const int32_t *toff;
    long nsort;
    double q, m, cell_vol, eps0;
    double *inv_d2, *ntot;
    uint32_t *skipped;
    int first, last;
};

template <bool D3>
__global__ void __launch_bounds__(CL_THREADS) k_debye(DebyeK k) {
    __shared__ double s_w[CL_CELLS], s_ux[CL_CELLS], s_uy[CL_CELLS], s_uz[CL_CELLS], s_kt[CL_CELLS];
    const int t = blockIdx.x, tid = threadIdx.x;
    s_w[tid] = 0; s_ux[tid] = 0; s_uy[tid] = 0; s_uz[tid] = 0; s_kt[tid] = 0;
    __syncthreads();
    const long lo = k.toff[t], hi = k.toff[t + 1] < k.nsort ? k.toff[t + 1] : k.nsort;
    uint32_t skipped = 0;
    for (long ip = lo + tid; ip < hi; ip += CL_THREADS) {
        const int ck = cell_of<D3>(k.p, ip, k.g);
        if (ck < 0) continue;
        if ((ck >> 8) != t) { skipped++; continue; }     // a store that was not sorted by its current positions
        const int c = ck & 255;
        const double w = k.p.w[ip];
        atomicAdd(&s_w[c], w); atomicAdd(&s_ux[c], w * k.p.ux[ip]); atomicAdd(&s_uy[c], w * k.p.uy[ip]);
        atomicAdd(&s_uz[c], w * k.p.uz[ip]);
    }
    if (skipped && k.skipped) atomicAdd(k.skipped, skipped);
    __syncthreads();
    if (s_w[tid] > 0) { s_ux[tid] /= s_w[tid]; s_uy[tid] /= s_w[tid]; s_uz[tid] /= s_w[tid]; }
    __syncthreads();
    for (long ip = lo + tid; ip < hi; ip += CL_THREADS) {
        const int ck = cell_of<D3>(k.p, ip, k.g);
        if (ck < 0 || (ck >> 8) != t) continue;
        const int c = ck & 255;
        const double dx = k.p.ux[ip] - s_ux[c], dy = k.p.uy[ip] - s_uy[c], dz = k.p.uz[ip] - s_uz[c];
        const double u2 = dx * dx + dy * dy + dz * dz;
        atomicAdd(&s_kt[c], k.p.w[ip] * u2 / sqrt(1 + u2) / 3);
    }
    __syncthreads();
    const int gc = global_cell<D3>(k.g, t, tid);
    if (gc < 0) return;
    double inv = k.first ? 0.0 : k.inv_d2[gc], n = k.first ? 0.0 : k.ntot[gc];
    if (s_w[tid] > 0) {
        const double density = s_w[tid] / k.cell_vol;
        const double kt = s_kt[tid] / s_w[tid] * k.m * LPA_C * LPA_C;
        inv += kt > 0 ? density * k.q * k.q / (k.eps0 * kt) : (double)INFINITY;
        n += density;
    }
    if (k.last && inv > 0) {      // the floor: no Debye length below the mean distance of the summed density
        const double rmin2 = pow(4 * 3.141592653589793 * n / 3, -2.0 / 3.0);
        if (1 / inv < rmin2) inv = 1 / rmin2;
    }
    k.inv_d2[gc] = inv; k.ntot[gc] = n;
}

int part_ok(const lpa_particles *p, const lpa_tiling *t, bool d3, const char *who) {
    LPA_REQUIRE(p && p->n >= 0 && t->n_sorted <= p->n, "%s: bad particle store", who);
    LPA_REQUIRE(p->n == 0 || (p->x && p->y && p->ux && p->uy && p->uz && p->w && (!d3 || p->z)), "%s: null particle array", who);
    LPA_REQUIRE(p->id, "%s: the pairing is defined on ids: lpa_particles.id must be set", who);
    return LPA_OK;
}

inline long align_up(long v) { return (v + 255) & ~255L; }

}  // namespace

extern "C" int64_t lpa_collide_workspace_bytes(const lpa_grid *g, int64_t capacity_a, int64_t capacity_b) {
    if (!g || capacity_a < 0 || capacity_b < 0) return LPA_ERR_ARG;
    const long n = capacity_a + capacity_b;
    return align_up(8 * n) * 2 + align_up(4 * n);
}

extern "C" int lpa_collide(const lpa_grid *g, const lpa_particles *pa, const lpa_tiling *ta, double qa, double ma,
                           const lpa_particles *pb, const lpa_tiling *tb, double qb, double mb,
                           const lpa_collide_params *cp, void *workspace, int64_t workspace_bytes, void *stream) {
    CollK k;
    int rc = fill_geom(&k.g, g, ta, "lpa_collide");
    if (rc) return rc;
    LPA_REQUIRE(cp && cp->dt > 0 && cp->eps0 > 0 && ma > 0 && mb > 0, "lpa_collide: bad parameters");
    LPA_REQUIRE(cp->lnLambda > 0 || cp->inv_d2, "lpa_collide: a varying Coulomb logarithm needs the Debye array");
    const bool d3 = ta->tiles_z > 0;
    k.inter = pa != pb;
    if (k.inter) {
        Geom gb;
        if ((rc = fill_geom(&gb, g, tb, "lpa_collide"))) return rc;
        LPA_REQUIRE((tb->tiles_z > 0) == d3, "lpa_collide: tilings of different dimension");
    } else {
        LPA_REQUIRE(ta == tb && qa == qb && ma == mb, "lpa_collide: pa == pb selects the intra-species form");
    }
    if ((rc = part_ok(pa, ta, d3, "lpa_collide")) || (rc = part_ok(pb, tb, d3, "lpa_collide"))) return rc;
    LPA_REQUIRE(workspace && workspace_bytes >= lpa_collide_workspace_bytes(g, ta->n_sorted, k.inter ? tb->n_sorted : 0),
                "lpa_collide: workspace too small");
    const long n = (long)ta->n_sorted + (k.inter ? (long)tb->n_sorted : 0);
    char *w = (char *)workspace;
    k.ws_key = (unsigned long long *)w; w += align_up(8 * n);
    k.ws_id = (unsigned long long *)w; w += align_up(8 * n);
    k.ws_slot = (uint32_t *)w;
    k.p[0] = make_partv(pa); k.p[1] = make_partv(pb);
    k.toff[0] = ta->tile_off; k.toff[1] = tb->tile_off;
    k.nsort[0] = ta->n_sorted; k.nsort[1] = tb->n_sorted;
    k.base[0] = 0; k.base[1] = ta->n_sorted;
    k.m[0] = ma; k.m[1] = mb; k.q[0] = qa; k.q[1] = qb;
    k.dt = cp->dt; k.lnl = cp->lnLambda; k.eps0 = cp->eps0; k.inv_d2 = cp->inv_d2;
    k.cell_vol = g->dx * g->dy * (d3 ? g->dz : 1.0);
    k.k0 = (uint32_t)cp->seed; k.k1 = (uint32_t)(cp->seed >> 32); k.itime = cp->itime; k.pidx = cp->pair_index;
    k.skipped = cp->skipped;
    const int ntiles = ta->tiles_x * ta->tiles_y * (d3 ? ta->tiles_z : 1);
    if (n == 0) return LPA_OK;
    if (d3) hipLaunchKernelGGL(k_collide<true>, dim3(ntiles), dim3(CL_THREADS), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(k_collide<false>, dim3(ntiles), dim3(CL_THREADS), 0, (hipStream_t)stream, k);
    LPA_CHECK_LAUNCH("lpa_collide");
    return LPA_OK;
}

extern "C" int lpa_collide_debye(const lpa_grid *g, int32_t nspecies, const lpa_particles *const *p,
                                 const lpa_tiling *const *t, const double *q, const double *m, double eps0,
                                 double *inv_d2, double *ntot, uint32_t *skipped, void *stream) {
    LPA_REQUIRE(nspecies > 0 && p && t && q && m && inv_d2 && ntot && eps0 > 0, "lpa_collide_debye: bad arguments");
    for (int s = 0; s < nspecies; s++) {
        DebyeK k;
        int rc = fill_geom(&k.g, g, t[s], "lpa_collide_debye");
        if (rc) return rc;
        const bool d3 = t[s]->tiles_z > 0;
        LPA_REQUIRE(d3 == (t[0]->tiles_z > 0), "lpa_collide_debye: tilings of different dimension");
        LPA_REQUIRE(p[s] && p[s]->n == t[s]->n_sorted && (p[s]->n == 0 || (p[s]->x && p[s]->y && p[s]->ux && p[s]->uy &&
                    p[s]->uz && p[s]->w && (!d3 || p[s]->z))) && m[s] > 0, "lpa_collide_debye: bad particle store");
        k.p = make_partv(p[s]); k.toff = t[s]->tile_off; k.nsort = t[s]->n_sorted;
        k.q = q[s]; k.m = m[s]; k.eps0 = eps0; k.cell_vol = g->dx * g->dy * (d3 ? g->dz : 1.0);
        k.inv_d2 = inv_d2; k.ntot = ntot; k.skipped = skipped; k.first = s == 0; k.last = s == nspecies - 1;
        const int ntiles = t[s]->tiles_x * t[s]->tiles_y * (d3 ? t[s]->tiles_z : 1);
        if (d3) hipLaunchKernelGGL(k_debye<true>, dim3(ntiles), dim3(CL_THREADS), 0, (hipStream_t)stream, k);
        else hipLaunchKernelGGL(k_debye<false>, dim3(ntiles), dim3(CL_THREADS), 0, (hipStream_t)stream, k);
        LPA_CHECK_LAUNCH("lpa_collide_debye");
    }
    return LPA_OK;
}
