// lpa_qed.hip -- nonlinear Compton photon emission in the locally-constant-field approximation (gfx950, wave64, FP64).
//
// Replaces the radiation stages of the reference (core/qed/inline.py:5-13,50-117, core/qed/optical_depth.py:38-81,
// core/qed/optical_depth_tables.py:32-90, core/qed/cpu.py:306-330) with two kernels around the fused push and a
// ballistic push for the photons:
//
//   lpa_qed_event   BEFORE the species' push.  A lane per slot of the store (tile ordered or loose: the same path).  The
//                   lane forms the mid-step position of the fused kernel's first half push in registers, gathers E / B
//                   there (the arithmetic of lpa_interpolate_2d / _3d) -- or reads the stored ex_part .. bz_part rows --,
//                   computes chi, looks the total rate up in a copy of the 1-D table staged in LDS once per workgroup,
//                   and tests for an event with a counter-based draw on the particle id (no optical-depth row exists).
//                   On an event the photon's energy fraction delta is sampled by the reference's row-blended bisection
//                   of the 2-D cumulative table (2 MB: read through L2; a lane's ten probes halve their stride).
//                   Events are counted with one ballot and one vector atomic per wave.
//   lpa_qed_emit    AFTER the species' push and deposit.  Lanes with delta > 0 that are still alive are compacted with a
//                   wave ballot and prefix count, one atomic per wave reserves the wave's slots at the loose tail of the
//                   photon store, each lane writes its photon and its electron recoils in place.
//   lpa_push_photons  x += c dt u / |u| with the periodic fold / open-face rule of the fused kernels; no field is read.
//
// Every store to memory is a plain vector store or a vector atomic.  The generator, the gather, chi and the photon step
// are shared with the pair-production kernels (lpa_bw.hip): lpa_qed.hpp.
#include "lpa_qed.hpp"

namespace {

// ---- the event kernel ----------------------------------------------------------------------------------------------
// _bisect_interp (optical_depth_tables.py:57-90) with the uniform draw `u` in place of np.random.rand(); equality with a
// node ends the search at that node (the reference loops forever there), and the node index is kept inside the table
__device__ __forceinline__ double sample_delta(const QedK &k, int row, double t, double u) {
    const double *__restrict__ a = k.cum + (long)row * k.delta_n, *__restrict__ b = a + k.delta_n;
    const double s = 1 - t;
    auto val = [&](int j) { return a[j] * s + b[j] * t; };
    const double ymin = val(0), ymax = val(k.delta_n - 1);
    const double r = u * (ymax - ymin) + ymin;
    int low = 0, high = k.delta_n - 1;
    while (low <= high) {
        const int mid = (low + high) >> 1;
        const double v = val(mid);
        if (v < r) low = mid + 1;
        else if (v > r) high = mid - 1;
        else { high = mid; break; }
    }
    const int j = high < 0 ? 0 : (high > k.delta_n - 2 ? k.delta_n - 2 : high);
    const double y1 = val(j), y2 = val(j + 1);
    const double slope = y2 > y1 ? k.dld / (y2 - y1) : 0.0;      // (a flat stretch -- the spectrum underflowed: its left node)
    return pow(10.0, k.ld_min + j * k.dld + slope * (r - y1));
}

template <bool D3>
__global__ void __launch_bounds__(QED_THREADS) k_qed_event(GridV g, PartV p, QedK k, double *__restrict__ delta_out,
                                                           uint32_t *__restrict__ counters) {
    __shared__ double s_rate[QED_MAX_CHI_N];
    for (int i = threadIdx.x; i < k.chi_n; i += QED_THREADS) s_rate[i] = k.rate[i];
    __syncthreads();
    const long ip = (long)blockIdx.x * QED_THREADS + threadIdx.x;
    double delta = 0.0;
    bool live = ip < p.n;
    double x = 0, y = 0, z = 0;
    if (live) {
        x = p.x[ip]; y = p.y[ip];
        if (D3) z = p.z[ip];
        live = !((p.dead && p.dead[ip]) || isnan(x) || isnan(y) || (D3 && isnan(z)));
    }
    if (live) {
        const double ux = p.ux[ip], uy = p.uy[ip], uz = p.uz[ip];
        const double ig = p.ig ? p.ig[ip] : inv_gamma_of(ux, uy, uz);     // (LPA_PUSH_NO_IG stores carry no inv_gamma)
        double eb[6];
        if (k.stored_eb) {
#pragma unroll
            for (int c = 0; c < 6; c++) eb[c] = p.eb[c][ip];
        } else {
            // the fused kernel's first half push (update_global_2d / _3d), in registers only
            x += k.cdt_half * ig * ux;
            y += k.cdt_half * ig * uy;
            if (D3) z += k.cdt_half * ig * uz;
            gather_eb<D3>(g, (x - g.x0) * (1.0 / g.dx), (y - g.y0) * (1.0 / g.dy), D3 ? (z - g.z0) * (1.0 / g.dz) : 0.0, eb);
        }
        const double chi = chi_of(eb, ux, uy, uz, ig, k.chi_factor);
        if (k.chi_out) k.chi_out[ip] = chi;
        if (chi >= k.chi_min) {                                            // (false for NaN: no table index from garbage)
            double lc, left;
            const int row = chi_row(k, chi, lc, left);
            // _linear_interp1d (optical_depth_tables.py:44-54)
            const double rate = s_rate[row] + (s_rate[row + 1] - s_rate[row]) / k.dlc * (lc - left);
            const double dtau = k.dt * ig;
            const unsigned long long id = p.id[ip];
            const U4 r = philox((uint32_t)id, (uint32_t)(id >> 32), k.itime, LPA_QED_PHILOX_TAG, k.k0, k.k1);
            // stateless event test: a fresh exponential optical depth is crossed within this step
            if (-log1p(-u01(r.w[0], r.w[1])) < rate * dtau)
                delta = sample_delta(k, row, (lc - left) / k.dlc, u01(r.w[2], r.w[3]));
        }
    }
    if (ip < p.n) delta_out[ip] = delta;
    const unsigned long long events = __ballot(delta > 0.0);
    if ((threadIdx.x & 63) == 0 && events) atomicAdd(&counters[0], (uint32_t)__popcll(events));
}

// ---- the emit kernel -----------------------------------------------------------------------------------------------
template <bool D3>
__global__ void __launch_bounds__(QED_THREADS) k_qed_emit(PartV e, PartV ph, long ph_capacity,
                                                          const double *__restrict__ delta, unsigned long long id_base,
                                                          unsigned long long *__restrict__ parent_out,
                                                          uint32_t *__restrict__ counters) {
    const long ip = (long)blockIdx.x * QED_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    double d = 0.0, x = 0, y = 0, z = 0;
    bool emit = false;
    if (ip < e.n) {
        d = delta[ip];
        x = e.x[ip]; y = e.y[ip];
        if (D3) z = e.z[ip];
        // a particle the push absorbed at an open face (x = NaN) emits nothing
        emit = d > 0.0 && !((e.dead && e.dead[ip]) || isnan(x) || isnan(y) || (D3 && isnan(z)));
    }
    const unsigned long long mask = __ballot(emit);
    if (!mask) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&counters[1], (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (!emit) return;
    const long k = (long)base + __popcll(mask & ((1ull << lane) - 1));
    const long slot = ph.n + k;
    const double ux = e.ux[ip], uy = e.uy[ip], uz = e.uz[ip];
    if (slot >= ph_capacity) {          // cannot happen when the host sized the store from the event count
        atomicAdd(&counters[2], 1u);
        return;
    }
    // create_photon_inline_2d / _3d (core/qed/inline.py:50-117)
    const double px = d * ux, py = d * uy, pz = d * uz;
    ph.x[slot] = x; ph.y[slot] = y;
    if (D3) ph.z[slot] = z;
    ph.ux[slot] = px; ph.uy[slot] = py; ph.uz[slot] = pz;
    ph.ig[slot] = 1.0 / sqrt(px * px + py * py + pz * pz);
    ph.w[slot] = e.w[ip];
    if (ph.id) ph.id[slot] = id_base + (unsigned long long)k;
    if (ph.dead) ph.dead[slot] = 0;
    if (parent_out) parent_out[k] = e.id ? e.id[ip] : 0ull;
    // photon_recoil_patches (core/qed/cpu.py:306-330)
    const double f = 1 - d;
    const double rx = ux * f, ry = uy * f, rz = uz * f;
    e.ux[ip] = rx; e.uy[ip] = ry; e.uz[ip] = rz;
    if (e.ig) e.ig[ip] = 1.0 / sqrt(1 + rx * rx + ry * ry + rz * rz);
}

template <bool D3>
__global__ void __launch_bounds__(QED_THREADS) k_push_photons(PartV p, PhotonK k) {
    const long ip = (long)blockIdx.x * QED_THREADS + threadIdx.x;
    if (ip >= p.n) return;
    if (p.dead && p.dead[ip]) return;
    double r[3] = {p.x[ip], p.y[ip], D3 ? p.z[ip] : 0.0};
    if (isnan(r[0]) || isnan(r[1]) || isnan(r[2])) return;
    const double u[3] = {p.ux[ip], p.uy[ip], p.uz[ip]};
    if (photon_advance<D3>(k, r, u, p.ig[ip])) {      // mark_out_of_bound_as_dead: beyond an open face
        r[0] = r[1] = r[2] = __longlong_as_double(0x7ff8000000000000ll);
        if (p.dead) p.dead[ip] = 1;
    }
    p.x[ip] = r[0]; p.y[ip] = r[1];
    if (D3) p.z[ip] = r[2];
}

}  // namespace

extern "C" int lpa_qed_event(const lpa_grid *g, const lpa_particles *p, const lpa_qed_params *qp, double *delta_out,
                             uint32_t *counters, void *stream) {
    LPA_REQUIRE(g && p && qp && counters, "lpa_qed_event: null argument");
    const bool d3 = p->z != nullptr;
    const bool stored = (qp->flags & LPA_QED_STORED_EB) != 0;
    LPA_REQUIRE(lpa_part_ok(p, d3 ? 3 : 2) || (p->n > 0 && !p->inv_gamma), "lpa_qed_event: bad particle store");
    LPA_REQUIRE(stored || lpa_grid_ok(g, d3 ? 3 : 2, 0), "lpa_qed_event: bad grid");
    if (p->n == 0) return LPA_OK;
    LPA_REQUIRE(p->x && p->y && p->ux && p->uy && p->uz && delta_out, "lpa_qed_event: null particle array");
    LPA_REQUIRE(p->id, "lpa_qed_event: the draws are defined on ids: lpa_particles.id must be set");
    LPA_REQUIRE(!stored || p->part_eb[0], "lpa_qed_event: LPA_QED_STORED_EB needs the ex_part .. bz_part rows");
    LPA_REQUIRE(qed_tables_ok(qp), "lpa_qed_event: bad tables (2 <= chi_n <= %d, delta_n >= 2, ascending ranges)",
                QED_MAX_CHI_N);
    const QedK k = make_qedk(qp);
    GridV gv;
    memset(&gv, 0, sizeof gv);
    if (!stored) gv = make_gridv(g, d3 ? 3 : 2);
    const dim3 grid((unsigned)((p->n + QED_THREADS - 1) / QED_THREADS));
    if (d3) hipLaunchKernelGGL(k_qed_event<true>, grid, dim3(QED_THREADS), 0, (hipStream_t)stream, gv, make_partv(p), k, delta_out, counters);
    else hipLaunchKernelGGL(k_qed_event<false>, grid, dim3(QED_THREADS), 0, (hipStream_t)stream, gv, make_partv(p), k, delta_out, counters);
    LPA_CHECK_LAUNCH("lpa_qed_event");
    return LPA_OK;
}

extern "C" int lpa_qed_emit(const lpa_particles *p_ele, const lpa_particles *p_pho, int64_t photon_capacity,
                            const double *delta, uint64_t id_base, uint64_t *parent_out, uint32_t *counters, void *stream) {
    LPA_REQUIRE(p_ele && p_pho && counters, "lpa_qed_emit: null argument");
    if (p_ele->n == 0) return LPA_OK;
    const bool d3 = p_ele->z != nullptr;
    LPA_REQUIRE(delta && p_ele->n > 0 && p_ele->x && p_ele->y && p_ele->ux && p_ele->uy && p_ele->uz && p_ele->w,
                "lpa_qed_emit: null electron array");
    LPA_REQUIRE(p_pho->n >= 0 && photon_capacity >= p_pho->n, "lpa_qed_emit: bad photon store");
    LPA_REQUIRE(photon_capacity == 0 || (p_pho->x && p_pho->y && p_pho->ux && p_pho->uy && p_pho->uz && p_pho->inv_gamma &&
                                         p_pho->w && (!d3 || p_pho->z)),
                "lpa_qed_emit: null photon array (a 3-D electron store needs a 3-D photon store)");
    const dim3 grid((unsigned)((p_ele->n + QED_THREADS - 1) / QED_THREADS));
    const unsigned long long base = id_base;
    if (d3) hipLaunchKernelGGL(k_qed_emit<true>, grid, dim3(QED_THREADS), 0, (hipStream_t)stream, make_partv(p_ele), make_partv(p_pho),
                               (long)photon_capacity, delta, base, (unsigned long long *)parent_out, counters);
    else hipLaunchKernelGGL(k_qed_emit<false>, grid, dim3(QED_THREADS), 0, (hipStream_t)stream, make_partv(p_ele), make_partv(p_pho),
                            (long)photon_capacity, delta, base, (unsigned long long *)parent_out, counters);
    LPA_CHECK_LAUNCH("lpa_qed_emit");
    return LPA_OK;
}

extern "C" int lpa_push_photons(const lpa_particles *p, const lpa_push_params *pp, double dt, void *stream) {
    LPA_REQUIRE(p && pp && p->n >= 0, "lpa_push_photons: bad args");
    if (p->n == 0) return LPA_OK;
    LPA_REQUIRE(p->x && p->y && p->ux && p->uy && p->uz && p->inv_gamma, "lpa_push_photons: null particle array");
    const bool d3 = p->z != nullptr;
    const PhotonK k = make_photonk(pp, dt);
    const dim3 grid((unsigned)((p->n + QED_THREADS - 1) / QED_THREADS));
    if (d3) hipLaunchKernelGGL(k_push_photons<true>, grid, dim3(QED_THREADS), 0, (hipStream_t)stream, make_partv(p), k);
    else hipLaunchKernelGGL(k_push_photons<false>, grid, dim3(QED_THREADS), 0, (hipStream_t)stream, make_partv(p), k);
    LPA_CHECK_LAUNCH("lpa_push_photons");
    return LPA_OK;
}
