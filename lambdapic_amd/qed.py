"""Nonlinear Compton photon emission of the resident engines -- the host side of csrc/lpa_qed.hip, shared by
``PicEngine2D`` and ``PicEngine3D`` (the reference's ``NonlinearComptonLCFA`` radiation stages,
`simulation/simulation.py:1013-1016,1048-1061`, `core/qed/radiation.py`).

A step with radiation registered runs the per-stage calls (never the one-call ``lpa_step`` route): ``lpa_qed_event`` in
front of a radiating species' fused push, ``lpa_qed_emit`` behind the last species' deposit, ``lpa_push_photons`` for a
photon species in place of the Boris push.  Photon species carry no charge: they are left out of the sort, the deposit
and the rho bookkeeping.  Events are a function of (seed, step, particle id) -- there is no optical-depth array, nothing is
added to the sort, the migration messages or a checkpoint, and a restart continues exactly.  Two small host reads per
radiating species and step: the event count (the photon store is grown to hold it before the emit launch, with the
reference's 25 % slack) and the emitted count (by which the photon store's ``n`` advances).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, constants, qed_tables
from ._lib import check


def chi_factor():
    """e hbar / (m_e^2 c^3) (`core/qed/inline.py:6`) from the constants the rest of the package uses"""
    try:
        from scipy.constants import hbar
    except Exception:      # scipy absent
        hbar = 1.054571817e-34
    return constants.E_CHARGE * hbar / (constants.M_E ** 2 * constants.C_LIGHT ** 3)


def qed_params(tabs, rate_dev, cum_dev, dt, seed, itime, stored_eb=False):
    """``lpa_qed_params`` for tables ``tabs`` (``qed_tables`` dict) whose arrays live in ``rate_dev`` / ``cum_dev``"""
    qp = _lib.lpa_qed_params()
    qp.dt, qp.chi_factor, qp.chi_min = dt, chi_factor(), 10.0 ** tabs["log_chi_range"][0]
    qp.rate, qp.cum = rate_dev.data_ptr(), cum_dev.data_ptr()
    qp.chi_n, qp.delta_n = tabs["chi_N"], tabs["delta_N"]
    qp.log_chi_min, qp.log_chi_max = tabs["log_chi_range"]
    qp.log_delta_min, qp.log_delta_max = tabs["log_delta_range"]
    qp.seed, qp.itime = int(seed) & ((1 << 64) - 1), int(itime) & 0xFFFFFFFF
    qp.flags = _lib.LPA_QED_STORED_EB if stored_eb else 0
    return qp


class RadiationMixin:
    """needs from the engine: ``species``, ``_g()``, ``stream``, ``comm``, ``device``, ``L`` and the store hooks
    ``_rad_part(i, eb)`` -> lpa_particles of the slots in use, ``_rad_capacity(i)``, ``_rad_reserve(i, capacity)``,
    ``_rad_set_n(i, n)``, ``_rad_ids(i)`` (int64 view of the id row), ``_rad_mark_photon(i)``, ``_rad_pp(i, dt)`` and
    ``_rad_id_base(i, k)`` (first of ``k`` fresh ids of species ``i``)"""

    radiation = None        # {"pairs": [(ispec, photon_ispec)], "seed", "itime", "id_next", "emitted", "tables"}: pickled
    _rad_scratch = None     # tables on the device, delta rows, counters: rebuilt on load
    _rad_launches = None    # optional log (set it to a list): (itime, kernel name, ispec) of every lpa_qed_* launch

    def add_radiation(self, ispec, photon_ispec, seed=0, tables=None):
        """species ``ispec`` radiates photons into species ``photon_ispec`` (q = 0; from here on moved by
        ``lpa_push_photons``, never sorted or deposited).  ``tables``: a table file (``qed_tables.load_tables``), default
        the generated ones"""
        if self.comm.size > 1:
            raise NotImplementedError("radiation on a slab chain (comm.size > 1) is not implemented: the photon store "
                                      "has no migration")
        ispec, photon_ispec = int(ispec), int(photon_ispec)
        for i in (ispec, photon_ispec):
            if not 0 <= i < len(self.species):
                raise IndexError(f"add_radiation names species {i}; the engine has {len(self.species)}")
        if ispec == photon_ispec or self.is_photon(ispec):
            raise ValueError("a photon species cannot radiate")
        seed = int(seed) & ((1 << 64) - 1)
        st = self.radiation or {"pairs": [], "itime": -1, "id_next": {}, "tables": tables, "seed": seed}
        if any(a == ispec for a, _ in st["pairs"]):
            raise ValueError(f"species {ispec} radiates already")
        if (st["seed"], st["tables"]) != (seed, tables):       # one seed and one set of tables (uploaded once) per engine
            raise ValueError("add_radiation: seed and tables must be the same for every radiating species of an engine")
        st["pairs"].append((ispec, photon_ispec))
        self._rad_mark_photon(photon_ispec)
        self.radiation = st

    def is_photon(self, i):
        return self.radiation is not None and any(b == i for _, b in self.radiation["pairs"])

    def _rad_state(self, a):
        """device scratch of radiating species ``a``: the tables (once per engine), its delta row and counters"""
        sc = self.__dict__.get("_rad_scratch") or {}
        self._rad_scratch = sc
        if "tabs" not in sc:
            tabs = qed_tables.tables(self.radiation["tables"])
            sc["tabs"] = tabs
            sc["rate"] = torch.from_numpy(tabs["photon_prob_rate_total"]).to(self.device)
            sc["cum"] = torch.from_numpy(tabs["integral_photon_prob_along_delta"]).to(self.device)
        s = sc.setdefault(a, {"counters": torch.zeros(4, dtype=torch.int32, device=self.device), "delta": None,
                              "parent": None, "pending": False})
        need = self._rad_capacity(a)
        if s["delta"] is None or s["delta"].numel() < need:
            s["delta"] = torch.zeros(need, dtype=torch.float64, device=self.device)
        return sc, s

    def _rad_log(self, name, i):
        if self._rad_launches is not None:
            self._rad_launches.append((self.radiation["itime"], name, i))

    # ---- the step's side -----------------------------------------------------------------------------------------
    def _radiation_begin(self):
        """called once per step by the step drivers; counts the steps (``itime`` = the index of the running step)"""
        if self.radiation is not None:
            self.radiation["itime"] += 1

    def radiation_event(self, a, dt, stored_eb=False):
        """``lpa_qed_event`` for species ``a`` if it radiates: before its push (``stored_eb``: from the ex_part .. bz_part
        rows, behind the split path's interpolation)"""
        st = self.radiation
        if st is None or not any(p[0] == a for p in st["pairs"]):
            return
        pc = self._rad_part(a, stored_eb)
        if pc.n == 0:
            return
        sc, s = self._rad_state(a)
        s["counters"].zero_()
        qp = qed_params(sc["tabs"], sc["rate"], sc["cum"], dt, st["seed"], st["itime"], stored_eb)
        check(self.L.lpa_qed_event(self._g(), C.byref(pc), C.byref(qp), s["delta"].data_ptr(),
                                   s["counters"].data_ptr(), self.stream), "lpa_qed_event")
        s["pending"] = True
        self._rad_log("lpa_qed_event", a)

    def radiation_emit(self):
        """``lpa_qed_emit`` for every species whose event kernel ran in this step: behind the last deposit.  Returns the
        emitted counts per radiating species"""
        st, out = self.radiation, {}
        if st is None:
            return out
        for a, b in st["pairs"]:
            s = (self.__dict__.get("_rad_scratch") or {}).get(a)
            if s is None or not s["pending"]:
                continue
            s["pending"] = False
            events = int(s["counters"][0].item())           # host read 1 (behind the push: it has to finish anyway)
            out[a] = 0
            if events == 0:
                continue
            n = self._rad_part(b, False).n
            if n + events > self._rad_capacity(b):
                self._rad_reserve(b, int(1.25 * (n + events)))      # (the reference's extend slack, core/particles.py:141-168)
            if s["parent"] is None or s["parent"].numel() < events:
                s["parent"] = torch.empty(int(1.25 * events), dtype=torch.int64, device=self.device)
            base = self._rad_id_base(b, events)
            pe, pp = self._rad_part(a, False), self._rad_part(b, False)
            check(self.L.lpa_qed_emit(C.byref(pe), C.byref(pp), self._rad_capacity(b), s["delta"].data_ptr(), base,
                                      s["parent"].data_ptr(), s["counters"].data_ptr(), self.stream), "lpa_qed_emit")
            self._rad_log("lpa_qed_emit", a)
            cnt = s["counters"].tolist()                   # host read 2
            k = cnt[1]
            if cnt[2] or k > events:
                raise _lib.LpaError(f"lpa_qed_emit: {cnt[2]} photons beyond the store, {k} emitted for {events} events")
            if k:
                # ids in the order of the parents' ids: the kernel numbers the photons in the order its waves arrive,
                # which differs from run to run; this makes a photon's id a function of the run's history alone
                ids = self._rad_ids(b)[n:n + k]
                ids[torch.argsort(s["parent"][:k])] = base + torch.arange(k, dtype=torch.int64, device=self.device)
            self._rad_set_n(b, n + k)
            out[a] = k
            st.setdefault("emitted", {})[a] = st.setdefault("emitted", {}).get(a, 0) + k       # running total per species
        return out

    def push_photons(self, i, dt):
        pc = self._rad_part(i, False)
        if pc.n == 0:
            return
        pp = self._rad_pp(i, dt)
        check(self.L.lpa_push_photons(C.byref(pc), C.byref(pp), dt, self.stream), "lpa_push_photons")
        self._rad_log("lpa_push_photons", i)


class SimulationRadiationMixin:
    """the radiation links of the ``Simulation`` / ``Simulation3D`` facades: ``Electron(radiation="photons", photon=pho)``
    (`core/species.py:185-243`) becomes ``engine.add_radiation`` in ``initialize()`` (`simulation/simulation.py:425-470`).
    ``chi``, ``tau`` and ``event`` mirrors do not exist (no optical depth is stored); ``delta`` is mirrored for '_qed'."""

    def _init_radiation(self):
        eng = self.engine
        for s in self.species:
            kind = getattr(s, "radiation", None)
            if kind is None:
                continue
            if kind != "photons":
                raise NotImplementedError(f"radiation={kind!r}: only 'photons' is implemented")
            if s.photon is None or not any(s.photon is t for t in self.species):
                raise ValueError(f"Species {s.name}: radiation='photons' needs photon= a species added to the simulation")
            eng.add_radiation(s.ispec, s.photon.ispec, seed=getattr(self, "random_seed", None) or 0)
        if eng.radiation is not None and hasattr(self, "_next_ids"):
            self._next_ids(0)                               # (2-D: the facade issues the ids -- ONE counter for both)
            eng.radiation["id_next"] = self._id_next

    def _delta_row(self, ispec):
        s = (self.engine.__dict__.get("_rad_scratch") or {}).get(ispec)
        return s["delta"] if s is not None and s["pending"] else None

    def _delta_mirror(self, ispec):
        """{"delta": host array over the live slots} while an event launch of this step awaits its emit, else {}"""
        row, sp = self._delta_row(ispec), self.engine.species[ispec]
        if row is None:
            return {}
        x = sp.cset.arr("x")[: sp.n]
        return {"delta": row[: sp.n][~torch.isnan(x)].cpu().numpy()}

    def _delta_upload(self, ispec, mirrors):
        """after a host callback: the store was rebuilt from the mirrors' live particles; delta follows in that order"""
        import numpy as np
        row = self._delta_row(ispec)
        if row is None or not all(hasattr(m, "delta") for m in mirrors):
            return
        parts = [m.delta[~m.is_dead & ~np.isnan(m.x) & ~np.isnan(m.y)] for m in mirrors]
        d = torch.from_numpy(np.ascontiguousarray(np.concatenate(parts), dtype=np.float64))
        row[: d.numel()] = d.to(row.device)
