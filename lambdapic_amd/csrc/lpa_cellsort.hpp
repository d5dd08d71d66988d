// lpa_cellsort.hpp -- what the per-cell kernels share (lpa_collide.hip, lpa_merge.hip): the sort's cell of a slot, the
// wave-level hand-over fence, the (key, id) ordering of a cell's list by one wave and the grid / tiling check of the
// entry points.  Everything is local to the including translation unit (anonymous namespace).
#pragma once
#include "lpa_common.hpp"

namespace {

constexpr int CL_CELLS = 256;          // cells of a tile, 2-D and 3-D

struct Geom {
    int nx, ny, nz, tiles_y, tiles_z;
    double x0, y0, z0, inv_dx, inv_dy, inv_dz;
};

// the sort's cell of a slot (lpa_sort.hip cell_key, ahead = 0): -1 = not live, else tile * 256 + cell in the tile;
// `gc` = the global cell index of the pairing contract
template <bool D3>
__device__ __forceinline__ int cell_of(const PartV &p, long ip, const Geom &g, int *gc = nullptr) {
    const double x = p.x[ip], y = p.y[ip];
    if ((p.dead && p.dead[ip]) || isnan(x) || isnan(y)) return -1;
    int is = ifloor((x - g.x0) * g.inv_dx + 0.5), js = ifloor((y - g.y0) * g.inv_dy + 0.5);
    is = is < 0 ? 0 : (is >= g.nx ? g.nx - 1 : is);
    js = js < 0 ? 0 : (js >= g.ny ? g.ny - 1 : js);
    if (!D3) {
        if (gc) *gc = is * g.ny + js;
        return ((is / LPA_TILE_X) * g.tiles_y + js / LPA_TILE_Y) * CL_CELLS + (is % LPA_TILE_X) * LPA_TILE_Y + js % LPA_TILE_Y;
    }
    const double z = p.z[ip];
    if (isnan(z)) return -1;
    int ks = ifloor((z - g.z0) * g.inv_dz + 0.5);
    ks = ks < 0 ? 0 : (ks >= g.nz ? g.nz - 1 : ks);
    if (gc) *gc = (is * g.ny + js) * g.nz + ks;
    const int tile = ((is / LPA_TILE3_X) * g.tiles_y + js / LPA_TILE3_Y) * g.tiles_z + ks / LPA_TILE3_Z;
    return tile * CL_CELLS + ((is % LPA_TILE3_X) * LPA_TILE3_Y + js % LPA_TILE3_Y) * LPA_TILE3_Z + ks % LPA_TILE3_Z;
}

// lanes of one wave hand data to each other through LDS / the workspace: order the accesses, no s_barrier needed
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- ordering a cell's list by (key, id) --------------------------------------------------------------------------
__device__ __forceinline__ bool ent_less(unsigned long long ka, unsigned long long ia, unsigned long long kb,
                                         unsigned long long ib) {
    return ka < kb || (ka == kb && ia < ib);
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const int lo = __shfl_xor((int)(uint32_t)v, m, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

// n <= 64: one entry per lane, bitonic network on lane exchanges (five 32-bit ds_bpermute per compare step: the xor
// distance is a loop variable); empty lanes hold the largest entry and stay behind
__device__ __forceinline__ void sort_regs(unsigned long long *key, unsigned long long *id, uint32_t *slot, int n, int lane) {
    unsigned long long k = ~0ull, i = ~0ull;
    uint32_t s = 0;
    if (lane < n) { k = key[lane]; i = id[lane]; s = slot[lane]; }
    for (int size = 2; (size >> 1) < n; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            const unsigned long long ko = shfl_xor_u64(k, j), io = shfl_xor_u64(i, j);
            const uint32_t so = (uint32_t)__shfl_xor((int)s, j, 64);
            const bool keep_min = ((lane & size) == 0) == ((lane & j) == 0);
            const bool other_less = ent_less(ko, io, k, i);
            if (keep_min == other_less && !(ko == k && io == i)) { k = ko; i = io; s = so; }
        }
    wave_sync();
    if (lane < n) { key[lane] = k; id[lane] = i; slot[lane] = s; }
    wave_sync();
}

// n > 64: bitonic network whose compare-exchanges all point the same way (the first step of a merge pairs i with its
// mirror image in the block), so the entries beyond n can be thought of as +infinity and never move
__device__ __forceinline__ void sort_mem(unsigned long long *key, unsigned long long *id, uint32_t *slot, int n, int lane) {
    int P = 128;
    while (P < n) P <<= 1;
    for (int size = 2; size <= P; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = 2 * t - (t & (j - 1));
                const int o = (j == (size >> 1)) ? (i ^ (size - 1)) : (i + j);
                if (o < n) {
                    const unsigned long long ki = key[i], ko = key[o], ii = id[i], io = id[o];
                    if (ent_less(ko, io, ki, ii)) {
                        key[i] = ko; key[o] = ki; id[i] = io; id[o] = ii;
                        const uint32_t si = slot[i];
                        slot[i] = slot[o]; slot[o] = si;
                    }
                }
            }
            wave_sync();
        }
}

__device__ __forceinline__ void sort_list(unsigned long long *key, unsigned long long *id, uint32_t *slot, int n, int lane) {
    if (n <= 1) return;
    if (n <= 64) sort_regs(key, id, slot, n, lane);
    else sort_mem(key, id, slot, n, lane);
}

int fill_geom(Geom *gm, const lpa_grid *g, const lpa_tiling *t, const char *who) {
    LPA_REQUIRE(g && g->nx > 0 && g->ny > 0 && g->dx > 0 && g->dy > 0, "%s: bad grid", who);
    LPA_REQUIRE(t && t->tile_off && t->tiles_x > 0 && t->tiles_y > 0 && t->n_sorted >= 0, "%s: bad tiling", who);
    const bool d3 = t->tiles_z > 0;
    LPA_REQUIRE(!d3 || (g->nz > 0 && g->dz > 0), "%s: 3-D tiling on a 2-D grid", who);
    const int tx = d3 ? LPA_TILE3_X : LPA_TILE_X, ty = d3 ? LPA_TILE3_Y : LPA_TILE_Y;
    LPA_REQUIRE(t->tiles_x == (g->nx + tx - 1) / tx && t->tiles_y == (g->ny + ty - 1) / ty &&
                    (!d3 || t->tiles_z == (g->nz + LPA_TILE3_Z - 1) / LPA_TILE3_Z),
                "%s: the tiling does not belong to this grid", who);
    gm->nx = g->nx; gm->ny = g->ny; gm->nz = d3 ? g->nz : 1; gm->tiles_y = t->tiles_y; gm->tiles_z = d3 ? t->tiles_z : 1;
    gm->x0 = g->x0; gm->y0 = g->y0; gm->z0 = g->z0;
    gm->inv_dx = 1.0 / g->dx; gm->inv_dy = 1.0 / g->dy; gm->inv_dz = d3 ? 1.0 / g->dz : 0.0;
    return LPA_OK;
}

}  // namespace
