"""Particle merging (csrc/lpa_merge.hip) against a plain restatement of the merge contract of include/lambdapic_amd.h:
numpy loops over cells, runs and chunks, in float64 and in np.longdouble; the bin key on the integer view of float64 in both.

Tolerance: ten times the largest float64 / longdouble discrepancy of the restatement itself on the same inputs (floor
1e-13), relative to the packet's sum w |u| for the conserved sums and to pa for a survivor's momentum; the planted packets
have pperp / pa >= 0.01 (asserted), which keeps the square root of the difference well conditioned.  Measured
(restatement float64 against longdouble | kernel against longdouble, momenta | kernel, conserved sums):
    massive   2-D 6.8e-15 | 6.0e-15 | 2.6e-16,  3-D 4.8e-15 | 4.0e-15 | 1.9e-16
    massless  2-D 7.6e-15 | 6.3e-15 | 2.3e-16,  3-D 8.2e-15 | 8.8e-15 | 2.6e-16
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_collide as K
from lambdapic_amd import _lib

pytestmark = pytest.mark.gpu

COUNTS = (0, 2, 3, 4, 5, 33, 64, 65, 130, 300)      # candidates of one bin per cell; 300: beyond the wave's LDS slice
P = dict(min_packet=4, max_packet=32, min_per_cell=8, radial_bits=2, angular_bins=8)
MAGS = (1e-3, 1e-1, 1.0, 30.0, 1e4)

def bin_keys(u):
    """(key, is candidate) of float64 momenta [n][3]: bit operations on s, IEEE division, no log / atan2 / sqrt"""
    rb, ab, rows = P["radial_bits"], P["angular_bins"], np.arange(len(u))
    s = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
    bits = s.view(np.uint64)
    r = (((bits >> np.uint64(52)) & np.uint64(0x7FF)) << np.uint64(rb)) | ((bits >> np.uint64(52 - rb)) & np.uint64((1 << rb) - 1))
    a = np.abs(u)
    axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    um = u[rows, axis]
    with np.errstate(all="ignore"):
        ia, ib = [np.minimum(ab - 1, np.nan_to_num(np.floor((u[rows, (axis + k) % 3] / np.abs(um) + 1) * 0.5 * ab))).astype(np.int64)
                  for k in (1, 2)]
    return r.astype(np.int64) << 13 | (2 * axis + (um < 0)) << 10 | ia << 5 | ib, (s > 0) & np.isfinite(s)

def restate(sp, dim, massless, T):
    """(u [n][3], w [n], dead [n], packets [(members in (key, id) order, pperp / pa, pa)]) after one lpa_merge, in type T"""
    u64 = np.stack([sp["ux"], sp["uy"], sp["uz"]], 1)
    u, w, one = u64.astype(T), sp["w"].astype(T), T(1)
    (key, cand), live = bin_keys(u64), ~np.isnan(sp["x"])
    cells, dead, packets = K.cells_of({a: np.nan_to_num(sp[a]) for a in "xyz"[:dim]}, dim), np.zeros(len(w), bool), []
    for g in np.unique(cells[live]):
        m = np.flatnonzero(live & (cells == g))
        if len(m) < P["min_per_cell"]:
            continue
        m = m[cand[m]]
        m = m[np.lexsort((sp["id"][m], key[m]))]
        for k in np.unique(key[m]):
            run = m[key[m] == k]
            for ch in (run[c:c + P["max_packet"]] for c in range(0, len(run), P["max_packet"])):
                if len(ch) < P["min_packet"]:
                    continue
                s = (u[ch] ** 2).sum(1)
                wt, pv, kin = w[ch].sum(), (w[ch, None] * u[ch]).sum(0), (w[ch] * (np.sqrt(s) if massless else s / (1 + np.sqrt(1 + s)))).sum()
                ka, pn = kin / wt, np.sqrt((pv * pv).sum())
                pa2, pl = ka * ka if massless else ka * (ka + 2), pn / wt
                pperp, face = np.sqrt(max(pa2 - pl * pl, T(0))), int(k >> 10) & 7
                d = np.zeros(3, T)
                d[face >> 1] = -one if face & 1 else one
                e1 = pv / pn if pn > 0 else d
                e3 = d - (d @ e1) * e1
                if e3 @ e3 < 1e-20:
                    d = np.roll(np.abs(d), 1)
                    e3 = d - (d @ e1) * e1
                e3 = e3 / np.sqrt(e3 @ e3)
                u[ch[0]], u[ch[1]], w[ch[:2]], dead[ch[2:]] = pl * e1 + pperp * e3, pl * e1 - pperp * e3, wt / 2, True
                packets.append((ch, float(pperp / np.sqrt(pa2)), np.sqrt(pa2)))
    return u, w, dead, packets

def bunch(rng, n, mag, face):
    """n momenta of one bin: |u|^2 inside one quarter octave near mag^2, the direction spread over most of one angular bin"""
    s = 2.0 ** np.round(np.log2(mag * mag)) * 1.125 * rng.uniform(0.93, 1.07, n)
    v = np.stack([np.ones(n), rng.uniform(0.27, 0.48, n), rng.uniform(0.27, 0.48, n)], 1)
    v = np.roll(v * np.sqrt(s / (v * v).sum(1))[:, None], face >> 1, 1)
    return -v if face & 1 else v

@functools.lru_cache(maxsize=None)
def planted(dim, massless):
    rng, shape = np.random.default_rng(10 * dim + massless), K.SHAPE[dim]
    fill = np.concatenate([np.eye(3), -np.eye(3), 7 * np.eye(3)[:2]]) * 0.37        # eight bins of one particle each
    border = [(7, 5), (8, 5)] if dim == 2 else [(3, 1, 1), (4, 1, 1)]               # neighbours across a tile border
    free = [c for c in rng.permutation(int(np.prod(shape))) if np.unravel_index(c, shape) not in border]
    cell, uu = [], []
    def put(c, u):
        cell.append(np.full(len(u), c)); uu.append(u)
    for j, n in enumerate(COUNTS):                                   # one bin + the fillers that lift the cell over min_per_cell
        put(free[j], np.concatenate([bunch(rng, n, MAGS[j % 5], j % 6), fill]))
    put(free[20], np.concatenate([bunch(rng, 7, 1e-3, 0), bunch(rng, 9, 1e-3, 3), bunch(rng, 40, 30.0, 0), np.zeros((1, 3))]))
    put(free[21], bunch(rng, 5, 1.0, 2))                             # below min_per_cell: left alone
    put(free[20], bunch(rng, 12, 30.0, 0))                           # twelve more of a bin of that cell: the dead slots (below)
    for b in border:                                                 # the same bin on both sides: never one packet
        put(np.ravel_multi_index(b, shape), bunch(np.random.default_rng(3), 10, 1.0, 4))
    cell, uu = np.concatenate(cell), np.concatenate(uu)
    n = len(cell)
    pos = (np.stack(np.unravel_index(cell, shape), 1) + rng.uniform(-0.45, 0.45, (n, dim))) * K.DX
    pos[n - 32:n - 20, 0] = np.nan                                   # dead slots (dead = NaN position in a resident store)
    sp = {"q": 0.0 if massless else K.QE, "m": 0.0 if massless else K.ME, "w": K.DX ** dim * 1e29 * rng.uniform(0.5, 2.0, n),
          "id": rng.permutation(n).astype(np.uint64) + np.uint64(5 << 50), "ux": uu[:, 0], "uy": uu[:, 1], "uz": uu[:, 2]}
    sp.update({a: pos[:, k] for k, a in enumerate("xyz"[:dim])})
    r64, rld = restate(sp, dim, massless, np.float64), restate(sp, dim, massless, np.longdouble)
    assert [list(p[0]) for p in r64[3]] == [list(p[0]) for p in rld[3]] and min(p[1] for p in rld[3]) >= 0.01
    assert {len(p[0]) for p in r64[3]} >= {4, 5, 7, 8, 9, 10, 12, 32} and len(r64[3]) == 27
    surv = np.concatenate([p[0][:2] for p in rld[3]])
    pa = np.repeat([p[2] for p in rld[3]], 2)
    err = float(np.max(np.linalg.norm((r64[0][surv] - rld[0][surv]).astype(float), axis=1) / pa.astype(float)))
    return sp, rld, max(10 * err, 1e-13), err

def merged(dim, massless, perm=None):
    sp = planted(dim, massless)[0]
    eng = K.engine(dim, _lib.LPA_ORDER_STRIPED)
    i = K.load(eng, dim, sp, perm)
    eng.add_merging(i, **P)
    eng.merge(i)
    eng.check_merging()                                # counters read; skipped == 0
    return eng, K.by_id(eng, dim, i), i

@pytest.mark.parametrize("massless", [0, 1])
@pytest.mark.parametrize("dim", [2, 3])
def test_merge_matches_restatement(dim, massless):
    sp, (u, w, dead, packets), tol, err = planted(dim, massless)
    eng, out, i = merged(dim, massless)
    live = ~np.isnan(sp["x"])
    keep = np.flatnonzero(live & ~dead)
    keep = keep[np.argsort(sp["id"][keep])]
    assert np.array_equal(out["_id"].view(np.uint64), sp["id"][keep])                 # who survives, who dies
    for a in "xyz"[:dim]:
        assert np.array_equal(out[a], sp[a][keep]), a                                  # nobody moves
    row = {int(j): k for k, j in enumerate(keep)}
    inpacket = np.concatenate([p[0] for p in packets])
    inpacket = set(inpacket.tolist())
    same = np.array([row[j] for j in keep.tolist() if j not in inpacket])
    for a in ("ux", "uy", "uz", "w"):
        assert np.array_equal(out[a][same], sp[a][keep][same]), a                      # untouched particles: the same bits
    uo = np.stack([out["ux"], out["uy"], out["uz"]], 1).astype(np.longdouble)
    uin, win, worst_u, worst_s = np.stack([sp["ux"], sp["uy"], sp["uz"]], 1).astype(np.longdouble), sp["w"].astype(np.longdouble), 0.0, 0.0
    kin = (lambda v: np.sqrt((v * v).sum(1))) if massless else (lambda v: (v * v).sum(1) / (1 + np.sqrt(1 + (v * v).sum(1))))
    for ch, _, pa in packets:
        a, b = row[ch[0]], row[ch[1]]
        worst_u = max(worst_u, *(float(np.linalg.norm(uo[r] - u[j]) / pa) for r, j in ((a, ch[0]), (b, ch[1]))))
        wo = out["w"][[a, b]].astype(np.longdouble)
        before = np.concatenate([[win[ch].sum()], (win[ch, None] * uin[ch]).sum(0), [(win[ch] * kin(uin[ch])).sum()]])
        after = np.concatenate([[wo.sum()], (wo[:, None] * uo[[a, b]]).sum(0), [(wo * kin(uo[[a, b]])).sum()]])
        scale = (win[ch] * np.sqrt((uin[ch] ** 2).sum(1))).sum()
        worst_s = max(worst_s, float(abs(after[0] - before[0]) / before[0]), float(np.max(np.abs(after[1:] - before[1:])) / scale))
    print(f"merge dim {dim} massless {massless}: restatement {err:.1e}, kernel momenta {worst_u:.1e}, sums {worst_s:.1e}, tol {tol:.1e}")
    assert worst_u <= tol and worst_s <= tol
    assert eng.merging["merged"][i] == len(packets) and eng.merging["removed"][i] == int(dead.sum())

@pytest.mark.parametrize("massless", [0, 1])
@pytest.mark.parametrize("dim", [2, 3])
def test_merge_is_independent_of_the_slot_order(dim, massless):
    n = len(planted(dim, massless)[0]["id"])
    a, b = merged(dim, massless)[1], merged(dim, massless, np.random.default_rng(5).permutation(n))[1]
    assert all(np.array_equal(a[k], b[k]) for k in ("_id", "ux", "uy", "uz", "w") + tuple("xyz"[:dim]))

@pytest.mark.parametrize("dim", [2, 3])
def test_facade_merges_every_other_step_and_restarts(dim, tmp_path):
    import test_gpu_qed as Q
    from lambdapic_amd.restart import RestartDump
    from lambdapic_amd.simulation import Electron, Photon, Simulation, callback
    from lambdapic_amd.simulation3d import Simulation3D

    def sim():
        pho = Photon(density=1e10, ppc=64)
        ele = Electron(radiation="photons", photon=pho)        # (makes `pho` a photon store; no field: nothing is emitted)
        bc = {k: "periodic" for k in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")[:2 * dim]}
        s = Simulation(16, 32, 1.2e-6, 1.2e-6, boundary_conditions=bc, random_seed=4) if dim == 2 else \
            Simulation3D(8, 8, 16, 1.2e-6, 1.2e-6, 1.2e-6, boundary_conditions=bc, random_seed=4)
        s.add_species([pho, ele])
        s.add_merging(pho, every=2, max_packet=8)
        s.totals = []

        @callback(stage="init")
        def setup(s):
            rows = s.engine.species[0].cset.data if dim == 2 else s.engine.species[0]["data"]
            u = torch.from_numpy(bunch(np.random.default_rng(1), rows.shape[1], 3e3, 0)).to(rows.device)
            rows[dim:dim + 3], rows[dim + 3] = u.T, 1 / u.norm(dim=1)

        @callback(stage="end")
        def total(s):
            p = Q._by_id(s, dim, 0)
            w, u = p["w"].astype(np.longdouble), np.stack([p["ux"], p["uy"], p["uz"]], 1).astype(np.longdouble)
            s.totals.append((len(w), np.concatenate([[w.sum()], (w[:, None] * u).sum(0), [(w * np.sqrt((u * u).sum(1))).sum()]])))
        setup.device_native = total.device_native = True
        return s, [setup, total]

    a, cbs = sim()
    a.run(4, callbacks=cbs)
    (n0, t0), (n1, t1), (n2, t2), (n3, t3) = a.totals
    loaded = 64 * (16 * 32 if dim == 2 else 8 * 8 * 16)
    assert n0 < loaded and n1 == n0 and n2 < n1 and n3 == n2                           # steps 0 and 2 merge, 1 and 3 do not
    a.engine.check_merging()
    assert a.engine.merging["removed"][0] == loaded - n3
    for t in (t1, t2, t3):                         # weight | momentum and energy relative to sum w |u|, at the floor of the rule above
        assert float(abs(t[0] - t0[0]) / t0[0]) <= 1e-13 and float(np.max(np.abs(t[1:] - t0[1:])) / t0[4]) <= 1e-13
    b, cbs_b = sim()
    dump = RestartDump(tmp_path, interval=lambda s: s.itime == 1)
    b.run(2, callbacks=cbs_b + [dump])
    (c := RestartDump.load(dump._ckpt_dir(1))).run(2)
    pa, pc = Q._by_id(a, dim, 0), Q._by_id(c, dim, 0)
    assert all(np.array_equal(pa[k], pc[k]) for k in pa)                               # no random draw: bit for bit
