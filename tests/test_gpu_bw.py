"""Breit-Wheeler pair production (csrc/lpa_bw.hip): push + event against a numpy restatement of the header's contract in float64
and np.longdouble (tolerances: four times the restatement's own discrepancy) and against lpa_push_photons; create; the facades."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch
import test_gpu_qed as Q
from lambdapic_amd import _lib, qed

pytestmark = pytest.mark.gpu
N, DEV, dev, DT, DX = 4096 + 37, Q.DEV, Q.dev, Q.DT, Q.DX

def tabs(chi_n=256, delta_n=1024, lo=-3.0, k=24.0):     # synthetic monotone tables: R dtau = k chi / |u|
    i, j = np.arange(chi_n), np.arange(delta_n)
    return {"chi_N": chi_n, "delta_N": delta_n, "log_chi_range": (lo, 2.0), "log_delta_range": (-3.0, 0.0),
            "photon_prob_rate_total": k / DT * np.logspace(lo, 2, chi_n),
            "integral_photon_prob_along_delta": np.outer(1 + i / (chi_n - 1), (j + 1.0) ** 0.7) + np.outer(np.sin(i) ** 2, j * 1e-3)}

@functools.lru_cache(maxsize=None)
def case(dim):
    """the fields of test_gpu_qed.case, N photons: |u| log-uniform over 10 .. 1e4, 5 % of the slots dead"""
    rng, c = np.random.default_rng(30 + dim), dict(Q.case(dim))
    d = rng.normal(size=(N, 3))
    u = d / np.linalg.norm(d, axis=1)[:, None] * 10 ** rng.uniform(1, 4, (N, 1))
    c.update({a: rng.uniform(-0.5, n - 0.5, N) * DX for a, n in zip("xyz", Q.SHAPE[dim])})
    c.update(ux=u[:, 0], uy=u[:, 1], uz=u[:, 2], inv_gamma=(u ** 2).sum(axis=1) ** -0.5, w=rng.uniform(1, 2, N),
             id=rng.integers(0, 2 ** 64, N, dtype=np.uint64), live=rng.uniform(size=N) > 0.05)
    return {k: v for k, v in c.items() if not k.endswith("_part")}

def restate(c, T, tb):
    """chi, R dtau, threshold, event flag, delta of every slot in dtype ``T``; j = #{nodes below r} - 1 (searchsorted)"""
    chi, ig = Q.restate(c, T, False)[0], c["inv_gamma"].astype(T)     # (chi at mid step: the same arithmetic)
    nc, nd, (lo, hi), (dlo, dhi) = tb["chi_N"], tb["delta_N"], tb["log_chi_range"], tb["log_delta_range"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = c["live"] & (chi >= T(10.0 ** lo))
        dlc, dld = (T(hi) - T(lo)) / (nc - 1), (T(dhi) - T(dlo)) / (nd - 1)
        lc = np.minimum(np.log10(np.where(ok, chi, 1)), T(hi))
        row = np.clip(np.floor(((lc - T(lo)) / dlc).astype(np.float64)).astype(int), 0, nc - 2)
        left, (rate, cum) = T(lo) + row * dlc, (tb["photon_prob_rate_total"].astype(T), tb["integral_photon_prob_along_delta"].astype(T))
        rdt = (rate[row] + (rate[row + 1] - rate[row]) / dlc * (lc - left)) * (T(DT) * ig)
        w = Q.philox(c["id"] & np.uint64(0xFFFFFFFF), c["id"] >> np.uint64(32), Q.ITIME, _lib.LPA_BW_PHILOX_TAG, Q.SEED)
        u1, u2 = (((hi_ << np.uint64(32) | lo_) >> np.uint64(11)).astype(T) * T(2.0) ** -53 for lo_, hi_ in (w[:2], w[2:]))
        thr, t = -np.log1p(-u1), ((lc - left) / dlc)[:, None]
        val = cum[row] * (1 - t) + cum[row + 1] * t
        r = u2 * (val[:, -1] - val[:, 0]) + val[:, 0]
        j, n = np.clip((val < r[:, None]).sum(axis=1) - 1, 0, nd - 2), np.arange(len(r))
        y1, y2 = val[n, j], val[n, j + 1]
        delta = np.power(T(10), T(dlo) + j * dld + np.where(y2 > y1, dld / (y2 - y1), 0) * (r - y1))
    event = ok & (thr < rdt)
    return chi, rdt, thr, event, np.where(event, delta, 0)

def run(c, tb, open_x=False, perm=None):
    """lpa_bw_push_event on the case and lpa_push_photons on a copy: delta, chi, counters, positions of both"""
    L, dim = _lib.lib(), c["dim"]
    (p, keep), (p2, keep2) = Q.particles(c, perm), Q.particles(c, perm)
    g, pp = _lib.lpa_grid(), _lib.lpa_push_params()
    g.nx, g.ny, g.nz, g.ng, g.dx, g.dy, g.dz = *(*Q.SHAPE[dim], 1)[:3], Q.NG, DX, DX, DX if dim == 3 else 0.0
    for a in Q.STAG:
        keep["f" + a] = dev(c["fields"][a])
        setattr(g, a, keep["f" + a].data_ptr())
    pp.dt, pp.wrap = DT, (6 | _lib.LPA_ABSORB_X) if open_x else 7
    for a, n in enumerate(Q.SHAPE[dim]):
        pp.lo[a] = pp.alo[a] = -0.5 * DX
        pp.hi[a] = pp.ahi[a] = (n - 0.5) * DX
    rate, cum = dev(tb["photon_prob_rate_total"]), dev(tb["integral_photon_prob_along_delta"])
    out, cnt = {k: torch.full((p.n,), -1.0, dtype=torch.float64, device=DEV) for k in "dc"}, torch.zeros(4, dtype=torch.int32, device=DEV)
    qp = qed.qed_params(tb, rate, cum, DT, Q.SEED, Q.ITIME)
    qp.chi_out = out["c"].data_ptr()
    _lib.check(L.lpa_bw_push_event(C.byref(g), C.byref(p), C.byref(pp), C.byref(qp), out["d"].data_ptr(), cnt.data_ptr(), None), "bw")
    _lib.check(L.lpa_push_photons(C.byref(p2), C.byref(pp), DT, None), "push")
    torch.cuda.synchronize()
    pos = lambda k: np.stack([k[a].cpu().numpy() for a in "xyz"[:dim]])
    return out["d"].cpu().numpy(), out["c"].cpu().numpy(), cnt.tolist(), pos(keep), pos(keep2)

@pytest.mark.parametrize("dim,chi_n,delta_n,open_x", [(2, 256, 1024, False), (3, 256, 1024, True), (2, 16, 100, True)])
def test_push_event_matches_restatement(dim, chi_n, delta_n, open_x):
    c, tb = case(dim), tabs(chi_n, delta_n)
    chi64, rdt64, thr64, ev64, d64 = restate(c, np.float64, tb)
    chiL, rdtL, thrL, evL, dL = restate(c, np.longdouble, tb)
    live = c["live"] & np.isfinite(chiL.astype(float))
    rel = lambda a, b, m: float(np.max(np.abs((a[m] - b[m]) / b[m]).astype(float)))
    tol_chi, tol_delta = 4 * rel(chi64, chiL, live), 4 * rel(d64, dL, ev64 & evL)
    edge = live & (np.abs(thrL - rdtL) <= tol_chi * rdtL)
    assert edge.sum() <= 0.01 * live.sum() and (ev64 == evL)[live & ~edge].all()      # the seed suits float64 already
    delta, chi, cnt, pos, ref = run(c, tb, open_x)
    assert np.array_equal(pos, ref, equal_nan=True)                      # the positions of lpa_push_photons, bit for bit
    gone = c["live"] & np.isnan(ref[0])                                 # absorbed at the open face in this step: no event
    assert gone.any() == open_x and not (delta[gone] != 0).any()
    live, ev = live & ~gone, delta > 0
    print(f"dim {dim} tables {chi_n}x{delta_n}: tol chi {tol_chi:.2e} delta {tol_delta:.2e}; kernel chi {rel(chi, chiL, live):.2e} "
          f"delta {rel(delta, dL, ev & evL):.2e}")
    assert rel(chi, chiL, live) <= tol_chi
    assert (ev == evL)[live & ~edge].all() and not delta[~c["live"]].any() and (delta >= 0).all()
    assert 0.05 * N < ev.sum() < 0.9 * N and cnt[0] == ev.sum()
    assert rel(delta, dL, ev & evL) <= tol_delta and (delta[ev] > 1e-3 * (1 - 1e-9)).all() and (delta[ev] < 1).all()

def test_queue_extremes():      # every lane of every workgroup has an event (the queue is full) / none has
    c, full = dict(case(2), live=np.ones(N, bool)), tabs(16, 100, lo=-12.0, k=1e12)
    delta, _, cnt, _, _ = run(c, full)
    assert cnt[0] == N and (delta > 1e-3 * (1 - 1e-9)).all() and (delta < 1).all()
    d64, dL = restate(c, np.float64, full)[4], restate(c, np.longdouble, full)[4]
    assert np.max(np.abs(delta / dL - 1)) <= 4 * np.max(np.abs(d64 / dL - 1))      # every entry of the queue was resolved
    delta, _, cnt, _, _ = run(c, tabs(16, 100, k=0.0))
    assert cnt[0] == 0 and not delta.any()

@pytest.mark.parametrize("dim", [2, 3])
def test_create(dim):
    L, rng, n, n0, cap, base = _lib.lib(), np.random.default_rng(6), 1000, (300, 170), 1400, (5000, 9000)
    c = {a: rng.normal(size=n) for a in ("x", "y", "z", "ux", "uy", "uz") if dim == 3 or a != "z"}
    c.update(live=rng.uniform(size=n) > 0.1, w=1.0 + np.arange(n), id=np.arange(n, dtype=np.uint64) + np.uint64(77), dim=dim)
    c["inv_gamma"] = (c["ux"] ** 2 + c["uy"] ** 2 + c["uz"] ** 2) ** -0.5
    delta = np.where(rng.uniform(size=n) < 0.4, rng.uniform(1e-3, 0.99, n), 0.0)
    ph, tph = Q.particles(c)
    before = {a: v.cpu().numpy() for a, v in tph.items()}
    host = [dict({a: rng.normal(size=cap) for a in tph if a != "id"}, id=np.arange(cap, dtype=np.uint64) + np.uint64(10 ** 6),
                 live=np.ones(cap, bool)) for _ in range(2)]
    part, tens = zip(*[Q.particles(h) for h in host])
    part[0].n, part[1].n = n0                                             # two target stores with n0[s] slots in use
    cnt, parent = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
    _lib.check(L.lpa_bw_create(C.byref(ph), C.byref(part[0]), C.byref(part[1]), cap, cap, dev(delta).data_ptr(), *base,
                               parent.data_ptr(), cnt.data_ptr(), None), "create")
    torch.cuda.synchronize()
    made = c["live"] & (delta > 0)
    k, d, new = int(made.sum()), delta[made], []
    assert cnt.tolist()[:3] == [0, k, 0]
    for s in range(2):
        got, lo = {a: v.cpu().numpy() for a, v in tens[s].items()}, n0[s]
        for a in got:                                                     # untouched slots are bit-identical
            assert np.array_equal(got[a][:lo], host[s][a][:lo]) and np.array_equal(got[a][lo + k:], host[s][a][lo + k:])
        new.append({a: v[lo:lo + k] for a, v in got.items()})
        assert sorted(new[s]["id"]) == list(range(base[s], base[s] + k))
    assert np.array_equal(new[0]["id"] - base[0], new[1]["id"] - base[1])  # the same k in both stores
    o = np.argsort(new[0]["w"])                                           # keyed by the parent's unique weight
    for s, f in enumerate((d, 1 - d)):
        for a in ("ux", "uy", "uz"):
            np.testing.assert_allclose(new[s][a][o], f * c[a][made], rtol=1e-14)
            np.testing.assert_allclose(new[0][a][o] + new[1][a][o], c[a][made], rtol=4e-16, atol=0)
        assert all(np.array_equal(new[s][a][o], c[a][made]) for a in "xyz"[:dim] + "w")
        u2 = sum((f * c[a][made]) ** 2 for a in ("ux", "uy", "uz"))
        np.testing.assert_allclose(new[s]["inv_gamma"][o], (1 + u2) ** -0.5, rtol=1e-14)
    assert np.array_equal(parent[:k].cpu().numpy()[new[0]["id"][o] - base[0]], c["id"].view(np.int64)[made])
    after = {a: v.cpu().numpy() for a, v in tph.items()}                  # the photons died; delta = 0 and dead: untouched
    assert all(np.isnan(after[a][made]).all() for a in "xyz"[:dim])
    assert all(np.array_equal(after[a][~made | (a not in "xyz")], before[a][~made | (a not in "xyz")], equal_nan=True) for a in after)

def test_rate_and_order_invariance():
    n, u, tb = 1 << 16, 1e3, tabs()
    c = {"dim": 2, "live": np.ones(n, bool), "x": np.full(n, 3.3 * DX), "y": np.full(n, 4.1 * DX), "ux": np.full(n, u),
         "uy": np.zeros(n), "uz": np.zeros(n), "w": np.ones(n), "inv_gamma": np.full(n, 1 / u),
         "id": np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15),
         "fields": {a: np.full((16 + 2 * Q.NG,) * 2, 4.4e6 if a == "bz" else 0.0) for a in Q.STAG}}
    rdt = restate(c, np.float64, tb)[1]
    p, perm = 1 - np.exp(-rdt[0]), np.random.default_rng(1).permutation(n)
    assert 0.01 < p < 0.95 and np.ptp(rdt) <= 1e-12 * rdt[0]
    delta, _, cnt, _, _ = run(c, tb)
    sigma = np.sqrt(n * p * (1 - p))                       # binomial: n independent draws
    print(f"events {cnt[0]} expected {n * p:.1f} sigma {sigma:.1f}")
    assert abs(cnt[0] - n * p) < 5 * sigma
    delta_p, _, cnt_p, _, _ = run(c, tb, perm=perm)
    assert cnt_p[0] == cnt[0] and np.array_equal(delta_p, delta[perm])

def _sim(dim, link):
    """|u| = 3e3 photons across a uniform Bz (chi = 3; R dtau = 1.1 / 0.9 per step in 2-D / 3-D: more than half of the loaded
    photons decay in step 1, before any lepton has radiated, so the store MUST be compacted), leptons that radiate"""
    from lambdapic_amd.simulation import Electron, Photon, Positron, Simulation, callback
    from lambdapic_amd.simulation3d import Simulation3D
    pho = Photon(density=1e10, ppc=16 if dim == 2 else 32)
    ele, pos = Electron(radiation="photons", photon=pho), Positron(radiation="photons", photon=pho)
    pho.set_bw_pair(electron=ele if link else None, positron=pos if link else None)
    bc = {k: "periodic" for k in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")[:2 * dim]}
    sim = Simulation(32, 32, 1.2e-6, 1.2e-6, boundary_conditions=bc, random_seed=4) if dim == 2 else \
        Simulation3D(8, 8, 8, 1.2e-6, 1.2e-6, 1.2e-6, boundary_conditions=bc, random_seed=4)
    sim.add_species([pho, ele, pos])
    sim.dead_share, sim.slots = [], []

    @callback(stage="init")
    def setup(s):
        eng, s.engine._rad_launches = s.engine, []
        (eng.grid.view if dim == 2 else eng.view)("bz").fill_(4.4e6)
        rows = eng.species[0].cset.data if dim == 2 else eng.species[0]["data"]
        rows[2 if dim == 2 else 3], rows[5 if dim == 2 else 6] = 3e3, 1 / 3e3

    @callback(stage="end")
    def share(s):
        n = s.engine._rad_part(0, False).n
        s.dead_share.append(float(torch.isnan(s.engine._rad_rows(0)[0][0, :n]).double().mean()))
        s.slots.append(n)
    setup.device_native = share.device_native = True
    return sim, [setup, share]

@pytest.mark.parametrize("dim", [2, 3])
def test_facade_cascade_and_restart(dim, tmp_path):
    from lambdapic_amd.restart import RestartDump
    from lambdapic_amd.simulation import callback
    a, cbs = _sim(dim, True)
    a.run(6, callbacks=cbs)
    st, loaded = a.engine.radiation, 32 * 32 * 16 if dim == 2 else 8 ** 3 * 32
    created, emitted = sum(st["created"].values()), sum(st["emitted"].values())
    part = [Q._by_id(a, dim, i) for i in range(3)]
    assert created > 100 and len(part[1]["x"]) == len(part[2]["x"]) == created
    assert emitted > 0 and len(part[0]["x"]) == loaded + emitted - created       # second-generation photons: the cascade closed
    assert all(len(set(p["_id"].view(np.int64).tolist())) == len(p["x"]) for p in part)
    assert max(a.dead_share) <= 0.5 and len(a.dead_share) == 6 and a.slots[0] < loaded      # (n drops only in _bw_compact)
    names = [(k, i) for _, k, i in a.engine._rad_launches]
    assert names.count(("lpa_bw_push_event", 0)) == names.count(("lpa_bw_create", 0)) == 6 and ("lpa_push_photons", 0) not in names
    b, cbs_b = _sim(dim, True)
    dump = RestartDump(tmp_path, interval=lambda s: s.itime == 2)
    b.run(3, callbacks=cbs_b + [dump])
    (c := RestartDump.load(dump._ckpt_dir(2))).run(3)
    for i in range(3):          # every particle by id, at the run-to-run bound of the atomic deposits
        pa, pc = part[i], Q._by_id(c, dim, i)
        assert np.array_equal(pa["_id"], pc["_id"])
        for k in pa:
            np.testing.assert_allclose(pc[k], pa[k], rtol=1e-9, atol=1e-9 * np.abs(pa[k]).max(), err_msg=k)
    with pytest.raises(NotImplementedError):     # a host callback between the photons' push and the create: refused, loudly
        _sim(dim, True)[0].run(1, callbacks=cbs + [callback(stage="current_deposition")(lambda s: None)])
    plain, cbs_p = _sim(dim, False)
    plain.run(2, callbacks=cbs_p)
    assert not [k for _, k, _ in plain.engine._rad_launches if k.startswith("lpa_bw")]      # no link: no lpa_bw_* launch
