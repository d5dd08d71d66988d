// lpa_merge.hip -- particle merging on a tile-binned store (gfx950, wave64, FP64): within a cell, particles that share
// a momentum bin are replaced by two that carry the same weight, momentum and energy (Vranic et al., CPC 191 (2015)
// 65-73).  The reference has no merging; the behaviour is the merge contract of include/lambdapic_amd.h: a pure function
// of the set of (id, x, u, w) of a cell -- no generator, no dependence on the storage order, restart exact.
//
// Decomposition: a workgroup per 256-cell tile, a wave per cell, a lane per particle.
//   1. bin     the tile's slots are counted per cell (LDS atomics), the counts scanned, and (key, id, slot) of every
//              live particle written to the cell's list in the workspace (key = momentum bin, all ones = no
//              candidate) -- the only assumption about the store is lpa_tiling.tile_off;
//   2. order   a wave takes a cell with enough particles: a list of up to MG_WAVE_ENTRIES entries is copied to the
//              wave's LDS slice and sorted there by (key, id) -- in registers up to 64 entries, by the bitonic network
//              on the staged copy beyond --, a longer one in the workspace (global path: the same code on other
//              pointers);
//   3. runs    every entry learns the start of its run of equal keys: a head is an entry whose left neighbour (lane
//              exchange; the last lane's entry is carried to the next 64) has another key, and a wave max-scan spreads
//              the heads' positions;
//   4. merge   the list is walked in batches of whole chunks (a run is cut from its start into chunks of max_packet
//              <= 64 entries, so a batch that starts at a chunk start holds at least that chunk): one entry per lane,
//              ux uy uz w read once into registers -- each entry is read by exactly one lane, so unlike the pairs of
//              lpa_collide.hip there is nothing a staging of the momenta in LDS could save; LDS holds the lists --,
//              the five sums reduced by a segmented tree on lane exchanges whose shape is a function of the entry's
//              offset in its chunk and of the chunk's length alone (bit-identical from run to run and for every storage
//              order), the head's sums broadcast; the two lowest lanes of a chunk write the survivors, the others NaN.
// Counters: one atomic per wave and counter.  No matrix instruction applies: there is no contraction here, only five
// short sums per packet and integer work.
#include "lpa_common.hpp"
#include "lpa_cellsort.hpp"

namespace {

constexpr int MG_THREADS = 256, MG_WAVES = MG_THREADS / 64;
constexpr int MG_WAVE_ENTRIES = 256;   // entries of a cell that fit the wave's LDS slice: 24 bytes each
constexpr unsigned long long MG_NO_KEY = ~0ull;

struct MergeK {
    Geom g;
    PartV p;
    const int32_t *toff;
    long nsort;
    int min_packet, max_packet, min_per_cell, radial_bits, angular_bins, massless;
    uint32_t *counters;
    unsigned long long *ws_key, *ws_id;
    uint32_t *ws_slot;
    int32_t *ws_run;
};

// |u|^2 as the bin key sees it: individually rounded products and sums, so that a host restatement gives the same bits
__device__ __forceinline__ double u_squared(double ux, double uy, double uz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)), __dmul_rn(uz, uz));
}

// the bin key of the merge contract; MG_NO_KEY = not a candidate
__device__ __forceinline__ unsigned long long bin_key(double ux, double uy, double uz, int radial_bits, int angular_bins) {
    const double s = u_squared(ux, uy, uz);
    if (!(s > 0.0) || isinf(s)) return MG_NO_KEY;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
    const unsigned long long r = (((bits >> 52) & 0x7ffull) << radial_bits) | ((bits >> (52 - radial_bits)) & ((1ull << radial_bits) - 1));
    const double ax = fabs(ux), ay = fabs(uy), az = fabs(uz);
    const int axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const double u[3] = {ux, uy, uz};
    const double um = u[axis], major = fabs(um);
    const unsigned long long face = 2 * axis + (um < 0.0 ? 1 : 0);
    const double nb = (double)angular_bins;
    const double qa = __ddiv_rn(u[(axis + 1) % 3], major), qb = __ddiv_rn(u[(axis + 2) % 3], major);
    int ia = (int)floor(__dmul_rn(__dmul_rn(__dadd_rn(qa, 1.0), 0.5), nb));
    int ib = (int)floor(__dmul_rn(__dmul_rn(__dadd_rn(qb, 1.0), 0.5), nb));
    ia = ia < angular_bins - 1 ? ia : angular_bins - 1;
    ib = ib < angular_bins - 1 ? ib : angular_bins - 1;
    return (r << 13) | (face << 10) | ((unsigned long long)ia << 5) | (unsigned long long)ib;
}

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src, 64), hi = __shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

__device__ __forceinline__ double shfl_f64(double v, int src) {
    return __longlong_as_double((long long)shfl_u64((unsigned long long)__double_as_longlong(v), src));
}

// run[i] = position of the first entry of the run of equal keys that holds entry i of the sorted list, -1 for an entry
// that is no candidate.  64 entries per round; the last entry's key and the scan's carry travel to the next round
__device__ __forceinline__ void mark_runs(const unsigned long long *key, int32_t *run, int n, int lane) {
    int carry = -1;
    unsigned long long kprev = MG_NO_KEY;
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        const unsigned long long k = i < n ? key[i] : MG_NO_KEY;
        unsigned long long kl = shfl_u64(k, lane > 0 ? lane - 1 : 0);
        if (lane == 0) kl = kprev;
        int v = (i == 0 || k != kl) ? i : -1;              // a run head carries its position
        for (int d = 1; d < 64; d <<= 1) {                 // inclusive max-scan: the nearest head at or left of the lane
            const int o = __shfl_up(v, d, 64);
            if (lane >= d && o > v) v = o;
        }
        if (carry > v) v = carry;
        if (i < n) run[i] = k == MG_NO_KEY ? -1 : v;
        carry = __shfl(v, 63, 64);
        kprev = shfl_u64(k, 63);
    }
    wave_sync();
}

// the packets of one cell's sorted list, by one wave; `merged` / `removed`: this lane's share of the counters
template <bool D3>
__device__ __forceinline__ void merge_cell(const MergeK &k, const unsigned long long *key, const uint32_t *slot,
                                           const int32_t *run, int n, int lane, uint32_t &merged, uint32_t &removed) {
    const PartV &p = k.p;
    const int maxp = k.max_packet;
    for (int b = 0; b < n;) {
        // ---- the batch: entries b .. b + 63, cut behind the last chunk that ends inside
        const int i = b + lane;
        const bool in = i < n;
        const int r = in ? run[i] : -2, rn = i + 1 < n ? run[i + 1] : -2;
        const int o = r >= 0 ? (i - r) % maxp : 0;                          // offset in the chunk
        const bool last = in && (r < 0 || rn != r || o + 1 == maxp);        // the chunk ends here
        const unsigned long long ends = __ballot(last);                     // (never 0: b is a chunk start, a chunk <= 64)
        if (ends == 0) break;
        const int end = 63 - __clzll((long long)ends);
        const bool act = lane <= end;
        const int ll = lane + __ffsll((long long)(ends >> lane)) - 1;       // lane of my chunk's last entry
        const int len = ll - (lane - o) + 1;                                // my chunk's length
        const bool member = act && r >= 0 && len >= k.min_packet;
        // ---- sums: wt, P = sum w u, K = sum w k
        double v[5] = {0, 0, 0, 0, 0}, ux = 0, uy = 0, uz = 0;
        long ip = 0;
        if (member) {
            ip = slot[i];
            ux = p.ux[ip]; uy = p.uy[ip]; uz = p.uz[ip];
            const double w = p.w[ip], s = u_squared(ux, uy, uz);
            const double kin = k.massless ? __dsqrt_rn(s) : s / (1.0 + __dsqrt_rn(1.0 + s));
            v[0] = w; v[1] = w * ux; v[2] = w * uy; v[3] = w * uz; v[4] = w * kin;
        }
        // segmented tree: at distance d the entries at offsets that are multiples of 2 d take in their neighbour at + d
        for (int d = 1; d < maxp; d <<= 1) {
            const bool take = member && (o & (2 * d - 1)) == 0 && o + d < len;
#pragma unroll
            for (int c = 0; c < 5; c++) {
                const double t = shfl_f64(v[c], lane + d < 64 ? lane + d : lane);
                if (take) v[c] += t;
            }
        }
        const int head = member ? lane - o : lane;
#pragma unroll
        for (int c = 0; c < 5; c++) v[c] = shfl_f64(v[c], head);
        const double wt = v[0];
        if (member && wt > 0.0) {                          // (a packet without weight is left untouched)
            if (o >= 2) {                                  // dies as a photon dies in lpa_bw_create
                const double nan = __longlong_as_double(0x7ff8000000000000ll);
                p.x[ip] = nan; p.y[ip] = nan;
                if (D3) p.z[ip] = nan;
                if (p.dead) p.dead[ip] = 1;
            } else {
                const double ka = v[4] / wt, pa2 = k.massless ? ka * ka : ka * (ka + 2.0);
                const double pn = __dsqrt_rn(v[1] * v[1] + v[2] * v[2] + v[3] * v[3]), pl = pn / wt;
                const double diff = pa2 - pl * pl, pperp = __dsqrt_rn(diff > 0.0 ? diff : 0.0);
                const int face = (int)((key[i] >> 10) & 7), axis = face >> 1;
                double dv[3] = {0, 0, 0}, e1[3], e3[3];
                dv[axis] = (face & 1) ? -1.0 : 1.0;
                for (int c = 0; c < 3; c++) e1[c] = pn > 0.0 ? v[1 + c] / pn : dv[c];
                double dd = dv[axis] * e1[axis], n2 = 0;
                for (int c = 0; c < 3; c++) { e3[c] = dv[c] - dd * e1[c]; n2 += e3[c] * e3[c]; }
                if (n2 < 1e-20) {                          // P along the face axis: the next axis in cyclic order
                    const int a2 = (axis + 1) % 3;
                    dv[axis] = 0.0; dv[a2] = 1.0;
                    dd = e1[a2]; n2 = 0;
                    for (int c = 0; c < 3; c++) { e3[c] = dv[c] - dd * e1[c]; n2 += e3[c] * e3[c]; }
                }
                const double f = (o == 0 ? pperp : -pperp) / __dsqrt_rn(n2);
                const double nx = pl * e1[0] + f * e3[0], ny = pl * e1[1] + f * e3[1], nz = pl * e1[2] + f * e3[2];
                p.ux[ip] = nx; p.uy[ip] = ny; p.uz[ip] = nz; p.w[ip] = 0.5 * wt;
                if (p.ig) {
                    const double u2 = nx * nx + ny * ny + nz * nz;
                    p.ig[ip] = 1.0 / __dsqrt_rn(k.massless ? u2 : 1.0 + u2);
                }
                if (o == 0) { merged += 1; removed += (uint32_t)(len - 2); }
            }
        }
        b += end + 1;
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

template <bool D3>
__global__ void __launch_bounds__(MG_THREADS) k_merge(MergeK k) {
    __shared__ int s_cnt[CL_CELLS], s_off[CL_CELLS];
    __shared__ unsigned long long s_key[MG_WAVES][MG_WAVE_ENTRIES], s_id[MG_WAVES][MG_WAVE_ENTRIES];
    __shared__ uint32_t s_slot[MG_WAVES][MG_WAVE_ENTRIES];
    __shared__ int32_t s_run[MG_WAVES][MG_WAVE_ENTRIES];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    s_cnt[tid] = 0;
    __syncthreads();
    // ---- 1. bin: count
    const long lo = k.toff[t], hi = k.toff[t + 1] < k.nsort ? k.toff[t + 1] : k.nsort;
    uint32_t skipped = 0;
    for (long ip = lo + tid; ip < hi; ip += MG_THREADS) {
        const int ck = cell_of<D3>(k.p, ip, k.g);
        if (ck < 0) continue;
        if ((ck >> 8) != t) { skipped++; continue; }
        atomicAdd(&s_cnt[ck & 255], 1);
    }
    __syncthreads();
    // scan (inclusive), then shifted to the exclusive offsets
    const int c0 = s_cnt[tid];
    s_off[tid] = c0;
    __syncthreads();
    for (int d = 1; d < CL_CELLS; d <<= 1) {
        const int a0 = tid >= d ? s_off[tid - d] : 0;
        __syncthreads();
        s_off[tid] += a0;
        __syncthreads();
    }
    s_off[tid] -= c0;
    __syncthreads();
    // ---- fill: (key, id, slot) into the cell's list; the fill cursor is the offset itself (it ends one past the cell)
    for (long ip = lo + tid; ip < hi; ip += MG_THREADS) {
        const int ck = cell_of<D3>(k.p, ip, k.g);
        if (ck < 0 || (ck >> 8) != t) continue;
        const int c = ck & 255;
        if (s_cnt[c] < k.min_per_cell || s_cnt[c] < k.min_packet) continue;      // (no wave will take this cell)
        const long o = lo + atomicAdd(&s_off[c], 1);
        k.ws_key[o] = bin_key(k.p.ux[ip], k.p.uy[ip], k.p.uz[ip], k.radial_bits, k.angular_bins);
        k.ws_id[o] = k.p.id[ip]; k.ws_slot[o] = (uint32_t)ip;
    }
    __syncthreads();
    // ---- 2 - 4. a wave per cell
    uint32_t merged = 0, removed = 0;
    for (int c = wv; c < CL_CELLS; c += MG_WAVES) {
        const int n = s_cnt[c];
        if (n < k.min_per_cell || n < k.min_packet) continue;
        const long ga = lo + s_off[c] - n;
        if (n <= MG_WAVE_ENTRIES) {
            for (int i = lane; i < n; i += 64) {
                s_key[wv][i] = k.ws_key[ga + i]; s_id[wv][i] = k.ws_id[ga + i]; s_slot[wv][i] = k.ws_slot[ga + i];
            }
            wave_sync();
            sort_list(s_key[wv], s_id[wv], s_slot[wv], n, lane);
            wave_sync();
            mark_runs(s_key[wv], s_run[wv], n, lane);
            merge_cell<D3>(k, s_key[wv], s_slot[wv], s_run[wv], n, lane, merged, removed);
            wave_sync();
        } else {
            sort_list(k.ws_key + ga, k.ws_id + ga, k.ws_slot + ga, n, lane);
            wave_sync();
            mark_runs(k.ws_key + ga, k.ws_run + ga, n, lane);
            merge_cell<D3>(k, k.ws_key + ga, k.ws_slot + ga, k.ws_run + ga, n, lane, merged, removed);
            wave_sync();
        }
    }
    if (k.counters) {
        merged = wave_sum(merged); removed = wave_sum(removed); skipped = wave_sum(skipped);
        if (lane == 0) {
            if (merged) atomicAdd(&k.counters[0], merged);
            if (removed) atomicAdd(&k.counters[1], removed);
            if (skipped) atomicAdd(&k.counters[2], skipped);
        }
    }
}

inline long align_up(long v) { return (v + 255) & ~255L; }

}  // namespace

extern "C" int64_t lpa_merge_workspace_bytes(const lpa_grid *g, int64_t capacity) {
    if (!g || capacity < 0) return LPA_ERR_ARG;
    return align_up(8 * capacity) * 2 + align_up(4 * capacity) * 2;
}

extern "C" int lpa_merge(const lpa_grid *g, const lpa_particles *p, const lpa_tiling *t, const lpa_merge_params *mp,
                         void *workspace, int64_t workspace_bytes, void *stream) {
    MergeK k;
    int rc = fill_geom(&k.g, g, t, "lpa_merge");
    if (rc) return rc;
    const bool d3 = t->tiles_z > 0;
    LPA_REQUIRE(p && p->n >= 0 && t->n_sorted <= p->n, "lpa_merge: bad particle store");
    LPA_REQUIRE(p->n == 0 || (p->x && p->y && p->ux && p->uy && p->uz && p->w && (!d3 || p->z)), "lpa_merge: null particle array");
    LPA_REQUIRE(p->id, "lpa_merge: the merge is defined on ids: lpa_particles.id must be set");
    LPA_REQUIRE(mp && mp->min_packet >= 3 && mp->max_packet >= mp->min_packet && mp->max_packet <= 64,
                "lpa_merge: need 3 <= min_packet <= max_packet <= 64");
    LPA_REQUIRE(mp->min_per_cell >= 0 && mp->radial_bits >= 0 && mp->radial_bits <= 8 && mp->angular_bins >= 1 &&
                    mp->angular_bins <= 32 && (mp->massless == 0 || mp->massless == 1),
                "lpa_merge: need min_per_cell >= 0, radial_bits in 0..8, angular_bins in 1..32, massless 0 or 1");
    const long n = t->n_sorted;
    LPA_REQUIRE(n < (1L << 31), "lpa_merge: more than 2^31 tile-ordered slots");
    LPA_REQUIRE(workspace && workspace_bytes >= lpa_merge_workspace_bytes(g, n), "lpa_merge: workspace too small");
    char *w = (char *)workspace;
    k.ws_key = (unsigned long long *)w; w += align_up(8 * n);
    k.ws_id = (unsigned long long *)w; w += align_up(8 * n);
    k.ws_slot = (uint32_t *)w; w += align_up(4 * n);
    k.ws_run = (int32_t *)w;
    k.p = make_partv(p); k.toff = t->tile_off; k.nsort = n;
    k.min_packet = mp->min_packet; k.max_packet = mp->max_packet; k.min_per_cell = mp->min_per_cell;
    k.radial_bits = mp->radial_bits; k.angular_bins = mp->angular_bins; k.massless = mp->massless;
    k.counters = mp->counters;
    const int ntiles = t->tiles_x * t->tiles_y * (d3 ? t->tiles_z : 1);
    if (n == 0) return LPA_OK;
    if (d3) hipLaunchKernelGGL(k_merge<true>, dim3(ntiles), dim3(MG_THREADS), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(k_merge<false>, dim3(ntiles), dim3(MG_THREADS), 0, (hipStream_t)stream, k);
    LPA_CHECK_LAUNCH("lpa_merge");
    return LPA_OK;
}
