"""Binary Coulomb collisions (csrc/lpa_collide.hip) against a plain restatement of the pairing contract of
include/lambdapic_amd.h: numpy Philox + Python loops over cells and pairs, in float64 and in np.longdouble.

Tolerance: ten times the largest float64 / longdouble discrepancy of the reference itself (floor 1e-13), relative to each
PARTICLE's own |u| after the collisions rather than to its pair's |p|: a particle's momentum is never larger than its
pair's, so this asks more (for an electron paired with an ion ~1836 times more).  Measured (float64 against longdouble,
every pair on the same branch in both; the p_perp <= 1e-10 p branch does not occur) and what the kernel gave:
    intra  2-D 2.7e-14, 3-D 3.8e-14, kernel 1.6 / 2.2e-14;   inter  2-D 1.1 .. 1.5e-13, 3-D 1.4 .. 2.6e-13, kernel 1.7 .. 2.2e-13
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

def cells_of(sp, dim):
    shape = SHAPE[dim]
    idx = [np.clip(np.floor(sp[a] / DX + 0.5).astype(int), 0, n - 1) for a, n in zip("xyz", shape)]
    return np.ravel_multi_index(idx, shape)

def reference(dim, a, b, lnl, pidx, T, debye_extra=()):
    """momenta [n][3] of a (and b) after one lpa_collide, computed in number type T; + the branch every pair took"""
    inter = b is not None
    sides = [a, b] if inter else [a]
    u = [np.stack([s["ux"], s["uy"], s["uz"]], 1).astype(T) for s in sides]
    cells = [cells_of(s, dim) for s in sides]
    vol, c, one = T(DX) ** dim, T(C), T(1)
    inv_d2 = np.zeros(int(np.prod(SHAPE[dim])), T)
    if lnl <= 0:                         # debye_length_patches + constrain_debye_length_patches over the species passed
        ntot = np.zeros_like(inv_d2)
        extra = [(e, cells_of(e, dim), np.stack([e["ux"], e["uy"], e["uz"]], 1).astype(T)) for e in debye_extra]
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
    shape = SHAPE[dim]
    cell = np.repeat(np.arange(0, int(np.prod(shape)), stride), [counts[k % len(counts)] for k in range(len(range(0, int(np.prod(shape)), stride)))])
    n = len(cell)
    pos = (np.stack(np.unravel_index(cell, shape), 1) + rng.uniform(-0.45, 0.45, (n, dim))) * DX
    sigma = np.array([0.01, 0.3, 3.0])[(cell // stride) % 3]
    uu = rng.normal(size=(n, 3)) * sigma[:, None] + np.array([0.5, 0.0, -0.2]) * sigma[:, None]
    uu[cell < 4 * stride] = 0.0                   # the first populated cells: pairs exactly at rest
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

def engine(dim, order):
    from lambdapic_amd.engine import PicEngine2D
    from lambdapic_amd.engine3d import PicEngine3D
    if dim == 2:
        return PicEngine2D(*SHAPE[2], DX, DX, order=order)
    eng = PicEngine3D(*SHAPE[3], DX, DX, DX)
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
