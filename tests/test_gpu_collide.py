"""Binary Coulomb collisions (csrc/lpa_collide.hip) against a plain restatement of the pairing contract of
include/lambdapic_amd.h: numpy Philox + Python loops over cells and pairs, in float64 and in np.longdouble.

Tolerance: ten times the largest float64 / longdouble discrepancy of the reference itself (floor 1e-13), relative to each
PARTICLE's own |u| after the collisions rather than to its pair's |p|: a particle's momentum is never larger than its
pair's, so this asks more (for an electron paired with an ion ~1836 times more).  Measured (float64 against longdouble,
every pair on the same branch in both; the p_perp <= 1e-10 p branch does not occur) and what the kernel gave:
    intra  2-D 2.7e-14, 3-D 3.8e-14, kernel 1.6 / 2.2e-14;   inter  2-D 1.1 .. 1.5e-13, 3-D 1.4 .. 2.6e-13, kernel 1.7 .. 2.2e-13
Stores shaped by absorption (test_collide_on_a_store_shaped_by_absorption; the launches of one collide() chained), reference
float64 against longdouble and what the kernel gave, 2-D / 3-D:
    dead     5.3e-14 / 2.8e-14, kernel 9.2e-14 / 2.3e-14;     partial  2.3e-14 / 3.4e-14, kernel 2.5e-14 / 3.7e-14
    large    8.6e-14 / 8.4e-14, kernel 8.9e-14 / 1.1e-13;     pairs    2.0e-14 / 2.6e-14, kernel 7.1e-14 / 3.2e-14
"""
import functools

import numpy as np
import pytest
import torch

from lambdapic_amd import _lib, constants

pytestmark = pytest.mark.gpu

C, EPS0, H = constants.C_LIGHT, constants.EPSILON_0, 6.62607015e-34
QE, ME, MI = -constants.E_CHARGE, constants.M_E, constants.M_P
COUNTS_A, COUNTS_B = (0, 1, 2, 3, 5, 8, 63, 64, 65, 129), (0, 1, 2, 3, 7, 64, 130)
DX = 2e-8
SHAPE = {2: (16, 64), 3: (8, 8, 32)}
SEED, ITIME, DT = 0x1234567890ABCDEF, 7, 5e-17

def philox(c0, c1, c2, c3, seed=SEED):
    c = [np.uint64(v) for v in (c0, c1, c2, c3)]
    k0, k1, m32 = seed & 0xFFFFFFFF, seed >> 32, np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [int(v) for v in c]

def u01(lo, hi):
    return ((hi << 32 | lo) >> 11) * 2.0 ** -53

def relerr(u, w):
    return float(np.max(np.linalg.norm((u - w).astype(float), axis=1) / np.maximum(np.linalg.norm(w.astype(float), axis=1), 1e-300)))

def cells_of(sp, dim, shape=None):
    shape = shape or SHAPE[dim]
    idx = [np.clip(np.floor(sp[a] / DX + 0.5).astype(int), 0, n - 1) for a, n in zip("xyz", shape)]
    return np.ravel_multi_index(idx, shape)

def reference(dim, a, b, lnl, pidx, T, debye_extra=(), shape=None):
    """momenta [n][3] of a (and b) after one lpa_collide, computed in number type T; + the branch every pair took"""
    inter = b is not None
    sides = [a, b] if inter else [a]
    u = [np.stack([s["ux"], s["uy"], s["uz"]], 1).astype(T) for s in sides]
    cells = [cells_of(s, dim, shape) for s in sides]
    vol, c, one = T(DX) ** dim, T(C), T(1)
    inv_d2 = np.zeros(int(np.prod(shape or SHAPE[dim])), T)
    if lnl <= 0:                         # debye_length_patches + constrain_debye_length_patches over the species passed
        ntot = np.zeros_like(inv_d2)
        extra = [(e, cells_of(e, dim, shape), np.stack([e["ux"], e["uy"], e["uz"]], 1).astype(T)) for e in debye_extra]
        for s, cl, us in list(zip(sides, cells, u)) + extra:
            for g in np.unique(cl):
                k = cl == g
                w = s["w"][k].astype(T)
                d = us[k] - (w[:, None] * us[k]).sum(0) / w.sum()
                u2 = (d * d).sum(1)
                kt = (w * u2 / np.sqrt(1 + u2) / 3).sum() / w.sum() * T(s["m"]) * c * c
                inv_d2[g] += w.sum() / vol * T(s["q"]) ** 2 / (T(EPS0) * kt) if kt > 0 else T(np.inf)
                ntot[g] += w.sum() / vol
        k = inv_d2 > 0
        inv_d2[k] = np.minimum(inv_d2[k], (4 * T(np.pi) * ntot[k] / 3) ** (T(2) / 3))
    branches = []

    def order(side, members, shuffled):
        ids = sides[side]["id"][members]
        keys = [(philox(int(i) & 0xFFFFFFFF, int(i) >> 32, ITIME, pidx << 8 | side) if shuffled else [0, 0]) for i in ids]
        return [members[j] for j in sorted(range(len(ids)), key=lambda j: (keys[j][0] | keys[j][1] << 32, int(ids[j])))]

    def pair(g, i, ia, ib, w_corr, dt_corr):
        sa, sb = sides[0], sides[-1]
        m1, q1, m2, q2 = T(sa["m"]), T(sa["q"]), T(sb["m"]), T(sb["q"])
        u1, u2 = u[0][ia], u[-1][ib]
        w1, w2 = T(sa["w"][ia]) * T(w_corr), T(sb["w"][ib]) * T(w_corr)
        g1, g2 = np.sqrt(1 + u1 @ u1), np.sqrt(1 + u2 @ u2)
        p1, p2, v1, v2 = u1 * m1 * c, u2 * m2 * c, u1 / g1 * c, u2 / g2 * c
        vc = (p1 + p2) / (g1 * m1 + g2 * m2)
        vc2 = vc @ vc
        gc = one / np.sqrt(1 - vc2 / c ** 2)
        fac = (gc - 1) / vc2 if vc2 > 0 else T(0)
        pc = p1 + (fac * (v1 @ vc) - gc) * m1 * g1 * vc
        p = np.sqrt(pc @ pc)
        if p == 0:
            branches.append((g, i, "rest"))
            return
        g1c, g2c = (1 - (vc @ v1) / c ** 2) * gc * g1, (1 - (vc @ v2) / c ** 2) * gc * g2
        shape = m1 * g1c * m2 * g2c / p ** 2 * c ** 2 + 1
        ln = T(lnl)
        if lnl <= 0:
            b0 = abs(q1 * q2) / (4 * T(np.pi) * T(EPS0) * c ** 2) * gc / (m1 * g1c + m2 * g2c) * shape
            bmin = max(T(H) / 2 / p, b0)
            ln = max(T(2), np.log(1 + (1 / inv_d2[g]) / bmin ** 2) / 2) if inv_d2[g] > 0 else T(2)
        s = max(w1, w2) / vol * T(DT) * dt_corr * ln * (q1 * q2) ** 2 / (4 * T(np.pi) * T(EPS0) ** 2 * c ** 4 * m1 * g1 * m2 * g2) \
            * gc * p / (m1 * g1 + m2 * g2) * shape ** 2
        r2, r3 = philox(i, g, ITIME, pidx << 8 | 2), philox(i, g, ITIME, pidx << 8 | 3)
        U, phi, uacc = T(u01(r2[0], r2[1])), 2 * T(np.pi) * T(u01(r2[2], r2[3])), T(u01(r3[0], r3[1]))
        if s < 4:
            al = T(0.37) * s - T(0.005) * s ** 2 - T(0.0064) * s ** 3
            s2 = al * U / np.sqrt((1 - U) + al * al * U)
            cosx, sinx = 1 - 2 * s2, 2 * np.sqrt(s2 * (1 - s2))
        else:
            cosx = 2 * U - 1
            sinx = np.sqrt(1 - cosx * cosx)
        pp, scp, ssp = np.sqrt(pc[0] ** 2 + pc[1] ** 2), sinx * np.cos(phi), sinx * np.sin(phi)
        perp = bool(pp > T(1e-10) * p)
        if perp:
            new = np.array([(pc[0] * pc[2] * scp - pc[1] * p * ssp) / pp + pc[0] * cosx,
                            (pc[1] * pc[2] * scp + pc[0] * p * ssp) / pp + pc[1] * cosx, -pp * scp + pc[2] * cosx])
        else:
            new = np.array([p * scp, p * ssp, p * cosx])
        acc1, acc2 = bool(w2 / max(w1, w2) > uacc), bool(w1 / max(w1, w2) > uacc)
        branches.append((g, i, bool(s < 4), perp, acc1, acc2))
        if acc1:
            u[0][ia] = (new + vc * (fac * (vc @ new) + m1 * g1c * gc)) / m1 / c
        if acc2:
            u[-1][ib] = (-new + vc * (fac * (vc @ -new) + m2 * g2c * gc)) / m2 / c

    for g in np.unique(cells[0]):
        la = np.flatnonzero(cells[0] == g)
        if not inter:
            n = len(la)
            if n < 2:
                continue
            s, npairs = order(0, la, True), (n + 1) // 2
            for i in range(npairs):
                last = n % 2 and i == npairs - 1
                pair(g, i, s[n - 1] if last else s[2 * i], s[0] if last else s[2 * i + 1],
                     0.5 if n % 2 and i in (0, npairs - 1) else 1.0, 2 * npairs - 1)
            continue
        lb = np.flatnonzero(cells[1] == g)
        na, nb = len(la), len(lb)
        if nb == 0:
            continue
        sa, sb = order(0, la, na >= nb), order(1, lb, nb > na)
        nmax, nmin = max(na, nb), min(na, nb)
        for i in range(nmax):
            w_corr = 1 / (nmax // nmin + 1) if i % nmin < nmax % nmin else 1 / (nmax // nmin)
            pair(g, i, sa[i if na >= nb else i % nmin], sb[i % nmin if na >= nb else i], w_corr, nmax)
    return u, branches

def make_species(dim, counts, q, m, rng, stride, wscale):
    """cell g (every ``stride``-th cell) holds counts[k-th populated cell mod len] particles off the cell boundaries"""
    cells = np.arange(0, int(np.prod(SHAPE[dim])), stride)
    return make_cells(dim, SHAPE[dim], cells, [counts[k % len(counts)] for k in range(len(cells))], q, m, rng, wscale)

def make_cells(dim, shape, cells, counts, q, m, rng, wscale):
    """the k-th of ``cells`` (flat indices into ``shape``) holds counts[k] particles off the cell boundaries; the thermal
    spread cycles over three decades, the first four populated cells are exactly at rest"""
    cell, ordinal = np.repeat(cells, counts), np.repeat(np.arange(len(cells)), counts)
    n = len(cell)
    pos = (np.stack(np.unravel_index(cell, shape), 1) + rng.uniform(-0.45, 0.45, (n, dim))) * DX
    sigma = np.array([0.01, 0.3, 3.0])[ordinal % 3]
    uu = rng.normal(size=(n, 3)) * sigma[:, None] + np.array([0.5, 0.0, -0.2]) * sigma[:, None]
    uu[ordinal < 4] = 0.0                         # the first populated cells: pairs exactly at rest
    sp = {"q": q, "m": m, "w": DX ** dim * (wscale * rng.uniform(0.5, 2.0, n) if wscale else np.full(n, 1e29)),
          "id": rng.permutation(n).astype(np.uint64) + np.uint64(5 << 50), "ux": uu[:, 0], "uy": uu[:, 1], "uz": uu[:, 2]}
    sp.update({a: pos[:, k] for k, a in enumerate("xyz"[:dim])})
    return sp

def load(eng, dim, sp, perm=None):
    """put the species into the engine, in the slot order ``perm``"""
    n = len(sp["id"])
    perm = np.arange(n) if perm is None else perm
    cols = dict(sp, inv_gamma=1 / np.sqrt(1 + sp["ux"] ** 2 + sp["uy"] ** 2 + sp["uz"] ** 2), id=sp["id"].view(np.int64))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(cols[a][perm])).to(eng.device)
    if dim == 3:
        data = torch.full((9, n + 64), float("nan"), dtype=torch.float64, device=eng.device)
        for k, a in enumerate(("x", "y", "z", "ux", "uy", "uz", "inv_gamma", "w")):
            data[k, :n] = dev(a)
        return eng.add_species_device(sp["q"], sp["m"], data, n, ids=dev("id"))
    i = eng.add_species(sp["q"], sp["m"], capacity=n + 64)
    s = eng.species[i]
    for a in ("x", "y", "ux", "uy", "uz", "inv_gamma", "w"):
        s.cset.arr(a)[:n] = dev(a)
    s.cset.id[:n] = dev("id")
    s.n, s.n_sorted, s.tiling = n, 0, None
    return i

def engine(dim, order, shape=None):
    from lambdapic_amd.engine import PicEngine2D
    from lambdapic_amd.engine3d import PicEngine3D
    if dim == 2:
        return PicEngine2D(*(shape or SHAPE[2]), DX, DX, order=order)
    eng = PicEngine3D(*(shape or SHAPE[3]), DX, DX, DX)
    eng.order = order
    return eng

def by_id(eng, dim, i):
    d = eng.species[i].download() if dim == 2 else eng.download_species(i)
    o = np.argsort(d["_id"].view(np.uint64))
    return {a: v[o] for a, v in d.items()}

@functools.lru_cache(maxsize=None)
def case_data(dim, case, varying):
    rng = np.random.default_rng(100 * dim + len(case))
    stride = 3 * (dim - 1)
    if case == "intra":                            # equal weights: the conservation check
        a, b = make_species(dim, COUNTS_A, QE, ME, rng, stride, 0.0), None
    else:                                          # electron - ion at the real mass ratio, unequal weights
        a, b = make_species(dim, COUNTS_A, QE, ME, rng, stride, 1e29), make_species(dim, COUNTS_B, -QE, MI, rng, stride, 3e28)
    lnl = 0.0 if varying else 10.0
    (r64, br64), (rld, brld) = reference(dim, a, b, lnl, 0, np.float64), reference(dim, a, b, lnl, 0, np.longdouble)
    assert br64 == brld, "float64 and longdouble took different branches: pick another seed"
    err = max(relerr(x, y) for x, y in zip(r64, rld))
    return a, b, lnl, r64, max(10 * err, 1e-13), br64

def collide(dim, order, a, b, lnl, perms=(None, None)):
    eng = engine(dim, order)
    ia = load(eng, dim, a, perms[0])
    ib = load(eng, dim, b, perms[1]) if b is not None else ia
    eng.add_collision([[ia, ib]], lnLambda=lnl, seed=SEED)
    eng.collision["itime"], eng._coll_launches = ITIME, []
    eng.collide(DT)
    eng.check_collision()                           # skipped == 0
    return eng, [by_id(eng, dim, i) for i in ([ia] if b is None else [ia, ib])]

@pytest.mark.parametrize("case", ["intra", "inter"])
@pytest.mark.parametrize("order", [_lib.LPA_ORDER_STRIPED, _lib.LPA_ORDER_CELL_MAJOR])
@pytest.mark.parametrize("dim", [2, 3])
def test_collide_matches_reference(dim, order, case):
    """engine.collide (sort with look-ahead 0, Debye arrays, lpa_collide) == the contract, per particle id; the Coulomb
    logarithm is fixed for STRIPED intra / CELL_MAJOR inter and varying for the other two (2-D STRIPED: inv_gamma NULL).
    Equal-weight intra-species cells also conserve momentum and energy."""
    a, b, lnl, ref, tol, branches = case_data(dim, case, (order == _lib.LPA_ORDER_CELL_MAJOR) != (case == "inter"))
    assert {"rest"} <= {br[2] for br in branches} and {True, False} <= {br[2] for br in branches}
    eng, out = collide(dim, order, a, b, lnl)
    worst = 0.0
    for sp, got, want in zip([a, b], out, ref):
        o = np.argsort(sp["id"])
        for attr in ("x", "y", "z", "w")[: dim] + ("w",):
            assert np.array_equal(got[attr], sp[attr][o]), attr
        assert np.array_equal(got["_id"].view(np.uint64), sp["id"][o])
        u = np.stack([got["ux"], got["uy"], got["uz"]], 1)
        worst = max(worst, relerr(u, want[o]))
        assert np.allclose(got["inv_gamma"], 1 / np.sqrt(1 + (u * u).sum(1)), rtol=1e-14, atol=0)
        if case == "intra":                           # conservation, needs no Philox: per cell sum p and sum gamma
            cl = cells_of(sp, dim)[o]
            u0 = np.stack([sp["ux"], sp["uy"], sp["uz"]], 1)[o]
            for f in (lambda v: v, lambda v: np.sqrt(1 + (v * v).sum(1, keepdims=True))):
                s0, s1, sc = (np.zeros((cl.max() + 1, f(u).shape[1])) for _ in range(3))
                np.add.at(s0, cl, f(u0)); np.add.at(s1, cl, f(u)); np.add.at(sc, cl, np.abs(f(u0)))
                assert np.max(np.abs(s1 - s0) / np.maximum(sc.sum(1, keepdims=True), 1e-300)) < tol
    print(f"dim {dim} order {order} {case}: worst {worst:.3e} tolerance {tol:.3e}")
    assert worst < tol
    assert len(eng._coll_launches) == 1

@pytest.mark.parametrize("dim", [2, 3])
def test_storage_order_invariance(dim):
    """the same particles in two slot permutations (and two tile orders) give identical momenta per id, bit for bit"""
    a, b, lnl = case_data(dim, "inter", False)[:3]
    rng = np.random.default_rng(1)
    perms = (rng.permutation(len(a["id"])), rng.permutation(len(b["id"])))
    _, first = collide(dim, _lib.LPA_ORDER_STRIPED, a, b, lnl)
    _, second = collide(dim, _lib.LPA_ORDER_COLUMN, a, b, lnl, perms)
    for x, y in zip(first, second):
        for attr in ("ux", "uy", "uz"):
            assert np.array_equal(x[attr], y[attr]), attr

def test_debye_counts_species_outside_the_groups():
    """varying lnLambda: the Debye length sums over ALL species, so a due step re-bins a third species that is in no
    group too -- here one whose last sort binned it far ahead of where its particles are"""
    a, b, _, _, tol, _ = case_data(2, "inter", True)
    c = make_species(2, COUNTS_B, QE, ME, np.random.default_rng(9), 3, 2e28)
    want, _ = reference(2, a, b, 0.0, 0, np.float64, debye_extra=[c])
    eng = engine(2, _lib.LPA_ORDER_STRIPED)
    ia, ib, ic = load(eng, 2, a), load(eng, 2, b), load(eng, 2, c)
    eng._dt_hint = 40 * DX / C                       # the sorter's look-ahead: up to 20 sort intervals x 8 steps of cells
    eng.sort(ic)
    assert eng.species[ic].sort_ahead_used > 0
    eng.add_collision([[ia, ib]], lnLambda=0.0, seed=SEED)
    eng.collision["itime"] = ITIME
    eng.collide(DT)
    eng.check_collision()
    assert eng.species[ic].sort_ahead_used == 0
    for sp, i, w in zip((a, b), (ia, ib), want):
        got = by_id(eng, 2, i)
        assert relerr(np.stack([got["ux"], got["uy"], got["uz"]], 1), w[np.argsort(sp["id"])]) < tol

def _sim(dim, collide):
    from lambdapic_amd.simulation import Simulation, Species
    from lambdapic_amd.simulation3d import Simulation3D
    if dim == 2:
        sim = Simulation(64, 64, DX, DX, npatch_x=2, npatch_y=2, random_seed=3, sort_interval=8,
                         boundary_conditions={k: "periodic" for k in ("xmin", "xmax", "ymin", "ymax")})
    else:
        sim = Simulation3D(16, 16, 32, DX, DX, DX, npatch_x=2, random_seed=3, sort_interval=8,
                           boundary_conditions={k: "periodic" for k in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")})
    e = Species("e", charge=-1, mass=1, density=lambda x, *_: 1e28 + 0 * x, ppc=8, momentum_sigma=0.02)
    ion = Species("p", charge=1, mass=1836.0, density=lambda x, *_: 1e28 + 0 * x, ppc=4)
    sim.add_species([e, ion])
    if collide:
        sim.add_collision([[e, e, ion]], every=2)
    sim.initialize()
    sim.engine._coll_launches = []
    return sim

def _momenta(sim, dim):
    out = []
    for i in range(2):
        d = sim.engine.species[i].download() if dim == 2 else sim.engine.download_species(i)
        out.append(np.stack([d["ux"], d["uy"], d["uz"]], 1)[np.argsort(d["_id"].view(np.uint64))])
    return out

def _close(us, vs, tol):
    return all(relerr(u, v) < tol for u, v in zip(us, vs))

DUE = [(t, a, b) for t in (0, 2, 4) for a, b in ((0, 0), (0, 1))]

def test_simulation_step_integration(tmp_path):
    """Simulation.add_collision([[e, e, ion]], every=2), five steps on the fused lpa_step path: the pairs are launched on
    steps 0, 2 and 4 only; the momenta differ from the run without collisions; rho carried by the continuity equation
    equals a real deposit (1e-12 of its maximum, the bound of test_rho_from_continuity_matches_deposited_rho) after the
    continuity step 3 and at the end; a RestartDump taken at step 2 resumes to the same momenta per id"""
    from lambdapic_amd.restart import RestartDump
    tol = case_data(2, "inter", True)[4]
    sim, real = _sim(2, True), _sim(2, True)
    real.engine.rho_continuity = False
    for n in (4, 1):
        sim.run(n), real.run(n)
        ra, rb = sim.engine.grid.view("rho"), real.engine.grid.view("rho")
        assert (ra - rb).abs().max().item() <= 1e-12 * rb.abs().max().item()
    assert sim.engine._coll_launches == DUE and sim.engine.rho_steps["continuity"] == 2
    ux = _momenta(sim, 2)
    plain = _sim(2, False)
    plain.run(5)
    assert not _close(ux, _momenta(plain, 2), 1e-6)
    part = _sim(2, True)
    dump = RestartDump(tmp_path, interval=lambda s: s.itime == 1)
    part.run(2, callbacks=[dump])
    resumed = RestartDump.load(dump._ckpt_dir(1))
    assert resumed.itime == 2 and resumed.engine.collision["itime"] == 1
    resumed.run(3)
    assert _close(_momenta(resumed, 2), ux, tol)

def test_simulation3d_staged_step_collides():
    """a Simulation3D step that cannot be fused (a callback at 'maxwell_1') collides like the fused one: same launches,
    same momenta up to the order of the FP64 atomics of the deposits (1e-9, the bound the suite uses between the two
    step drivers)"""
    from lambdapic_amd.simulation import callback
    seen = []

    @callback(stage="maxwell_1", interval=1)
    def probe(s):
        seen.append(s.itime)

    staged, fused = _sim(3, True), _sim(3, True)
    staged.run(5, callbacks=[probe])
    fused.run(5)
    assert seen == list(range(5))
    assert staged.engine._coll_launches == DUE == fused.engine._coll_launches
    assert _close(_momenta(staged, 3), _momenta(fused, 3), 1e-9)

# ---- stores that absorption has shaped: dead slots, grids ending in partial tiles, deep cells, pair_index > 0 -----------------
# Grids that are no multiple of the 8 x 32 / 4 x 4 x 16 tiles; the populated cells include the last, partial tile along every axis.
SHAPE_P = {2: (12, 40), 3: (6, 6, 20)}
CELLS_P = {2: [(0, 0), (3, 5), (7, 31), (8, 0), (11, 10), (5, 32), (2, 39), (9, 33), (11, 39), (8, 32), (10, 38), (4, 17)],
           3: [(0, 0, 0), (3, 3, 15), (4, 0, 0), (5, 2, 7), (0, 4, 3), (2, 5, 9), (1, 1, 16), (3, 2, 19), (4, 4, 16), (5, 5, 19),
               (4, 5, 17), (0, 5, 18)]}
COUNTS_PA, COUNTS_PB = (2, 3, 5, 8, 1, 64, 7, 65, 9, 4, 33, 2), (1, 2, 7, 3, 4, 9, 0, 5, 66, 2, 1, 6)
BIG = 300           # one cell deeper than the 256 the LDS path holds: global-memory pairing, sort_mem at P = 512

def _sub(sp, keep):
    return {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in sp.items()}

def _with_u(sp, u):
    return dict(sp, ux=u[:, 0], uy=u[:, 1], uz=u[:, 2])

@functools.lru_cache(maxsize=None)
def shaped_data(dim, case):
    """(a, b, dead ids of a / of b, launches [(side a, side b or None, lnLambda, pair index)], expected momenta per species
    in float64 chained over the launches, tolerance, branches) -- all of it computed on the CPU.  Every launch list is what
    ONE engine.collide() does for the groups of the case, in its launch order."""
    rng = np.random.default_rng(1000 * dim + {"dead": 1, "partial": 2, "large": 3, "pairs": 4}[case])
    shape = SHAPE_P[dim]
    cells = [int(np.ravel_multi_index(c, shape)) for c in CELLS_P[dim]]
    ca, cb = list(COUNTS_PA), list(COUNTS_PB)
    if case == "large":                                # cell 5: 300 electrons (intra) and 300 + 5 (inter: rep = 60, rem = 0);
        ca[5], cb[5] = BIG, 5                          # cell 8: 7 + 300 the other way round (rep = 42, rem = 6)
        ca[8], cb[8] = 7, BIG
    a = make_cells(dim, shape, cells, ca, QE, ME, rng, 1e29)
    b = make_cells(dim, shape, cells, cb, -QE, MI, rng, 3e28)
    dead = [np.zeros(0, np.uint64), np.zeros(0, np.uint64)]
    if case == "dead":                                 # ~10 % of each species, scattered: most populated cells lose some
        dead = [np.sort(rng.choice(s["id"], size=len(s["id"]) // 10, replace=False)) for s in (a, b)]
    launches = {"dead": [(0, 0, 10.0, 0), (0, 1, 10.0, 1)], "partial": [(0, 1, 0.0, 0)],
                "large": [(0, 0, 10.0, 0), (0, 1, 10.0, 1)], "pairs": [(0, 0, 10.0, 0), (0, 1, 10.0, 1), (1, 1, 10.0, 2)]}[case]
    out, err, branches = {}, 0.0, {}
    for T in (np.float64, np.longdouble):
        live = [_sub(s, ~np.isin(s["id"], d)) for s, d in zip((a, b), dead)]
        branches[T] = []
        for sa, sb, lnl, pidx in launches:
            u, br = reference(dim, live[sa], live[sb] if sb != sa else None, lnl, pidx, T, shape=shape)
            live[sa] = _with_u(live[sa], u[0])
            if sb != sa:
                live[sb] = _with_u(live[sb], u[1])
            branches[T].append(br)
        out[T] = [np.stack([s["ux"], s["uy"], s["uz"]], 1) for s in live]
    assert branches[np.float64] == branches[np.longdouble], "float64 and longdouble took different branches: pick another seed"
    err = max(relerr(x, y) for x, y in zip(out[np.float64], out[np.longdouble]))
    ids = [s["id"][~np.isin(s["id"], d)] for s, d in zip((a, b), dead)]
    return a, b, dead, launches, out[np.float64], ids, max(10 * err, 1e-13), err, branches[np.float64]

def _kill(eng, dim, i, ids):
    """blank the positions of the particles ``ids`` in the SORTED store ``i``, as the push does to a particle it absorbs;
    -> (slot mask, what those slots hold besides the position)"""
    want = torch.from_numpy(ids.view(np.int64)).to(eng.device)
    if dim == 2:
        sp = eng.species[i]
        mask = torch.isin(sp.cset.id[: sp.n], want)
        for a in "xy":
            sp.cset.arr(a)[: sp.n][mask] = float("nan")
        rest = lambda: torch.stack([sp.cset.arr(a)[: sp.n][mask] for a in ("ux", "uy", "uz", "w")] +
                                   [sp.cset.id[: sp.n][mask].view(torch.float64)])
        pos = lambda: torch.stack([sp.cset.arr(a)[: sp.n][mask] for a in "xy"])
    else:
        sp = eng.species[i]
        data = sp["data"][:, : sp["n"]]
        mask = torch.isin(data[8].view(torch.int64), want)
        data[:3, mask] = float("nan")
        rest = lambda: torch.stack([data[k][mask] for k in (3, 4, 5, 7, 8)])
        pos = lambda: data[:3][:, mask]
    assert int(mask.sum().item()) == len(ids)
    return rest, pos, rest().clone()

@pytest.mark.parametrize("case", ["dead", "partial", "large", "pairs"])
@pytest.mark.parametrize("dim", [2, 3])
def test_collide_on_a_store_shaped_by_absorption(dim, case):
    """lpa_collide on what a run with open faces hands it, against the same contract restatement and with the same
    tolerance rule as above (ten times the float64 / longdouble discrepancy of the reference on THESE inputs, floor 1e-13):
      dead     ~10 % of the slots of both sorted stores are dead the way the push leaves an absorbed particle (position
               NaN), some inside populated cells: the reference pairs the others, the dead slots come back untouched;
      partial  grids of 12 x 40 / 6 x 6 x 20 cells, populated cells in the last partial tile along every axis, varying lnLambda;
      large    a cell of 300 electrons (intra-species) and cells of 300 + 5 and 7 + 300 (inter-species): the global-memory
               pairing, the sort at P = 512 and weight corrections with quotients of 60 and 42 (remainder 6);
      pairs    groups [[e, e, i], [i, i]] in one collide(): pair_index 0, 1, 2 in launch order, each launch working on
               what the one before left."""
    a, b, dead, launches, want, ids, tol, err, branches = shaped_data(dim, case)
    shape = SHAPE_P[dim]
    eng = engine(dim, _lib.LPA_ORDER_STRIPED, shape)
    ia, ib = load(eng, dim, a), load(eng, dim, b)
    groups = {"dead": [[ia, ia, ib]], "partial": [[ia, ib]], "large": [[ia, ia, ib]], "pairs": [[ia, ia, ib], [ib, ib]]}[case]
    eng.add_collision(groups, lnLambda=launches[0][2], seed=SEED)
    eng.collision["itime"], eng._coll_launches = ITIME, []
    kept = []
    if case == "dead":                                   # sort as a due step does (look-ahead 0), then absorb
        eng._coll_sorting = True
        eng.sort(ia), eng.sort(ib)
        eng._coll_sorting = False
        kept = [_kill(eng, dim, i, d) for i, d in ((ia, dead[0]), (ib, dead[1]))]
    eng.collide(DT)
    eng.check_collision()
    assert eng._coll_launches == [(ITIME, (ia, ib)[sa], (ia, ib)[sb]) for sa, sb, _, _ in launches]
    assert [eng.collision["pairs"].index((x, y)) for _, x, y in eng._coll_launches] == [l[3] for l in launches]
    worst = 0.0
    for sp, i, w, live_ids in zip((a, b), (ia, ib), want, ids):
        got = by_id(eng, dim, i)
        o = np.argsort(live_ids)
        assert np.array_equal(got["_id"].view(np.uint64), live_ids[o])
        sel = np.flatnonzero(np.isin(sp["id"], live_ids))[o]
        for attr in ("x", "y", "z")[: dim] + ("w",):
            assert np.array_equal(got[attr], sp[attr][sel]), attr
        worst = max(worst, relerr(np.stack([got["ux"], got["uy"], got["uz"]], 1), w[o]))
    for rest, pos, before in kept:                       # dead slots: still dead, nothing else touched
        assert torch.isnan(pos()).all() and torch.equal(rest().view(torch.int64), before.view(torch.int64))
    kinds = {br[2] for launch in branches for br in launch}
    assert True in kinds and (False in kinds or case == "partial")      # both scattering-angle branches occur
    print(f"shaped dim {dim} {case}: reference f64 / longdouble {err:.3e} worst {worst:.3e} tolerance {tol:.3e}")
    assert worst < tol
