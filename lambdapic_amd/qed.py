"""Nonlinear Compton photon emission and Breit-Wheeler pair production of the resident engines -- the host side of
csrc/lpa_qed.hip and csrc/lpa_bw.hip, shared by ``PicEngine2D`` and ``PicEngine3D`` (the reference's
``NonlinearComptonLCFA`` and ``NonlinearPairProductionLCFA`` stages, `simulation/simulation.py:1013-1016,1048-1065`,
`core/qed/radiation.py`, `core/qed/pair_production.py`).

A step with radiation registered runs the per-stage calls (never the one-call ``lpa_step`` route): ``lpa_qed_event`` in
front of a radiating species' fused push, ``lpa_qed_emit`` behind the last species' deposit, ``lpa_push_photons`` for a
photon species in place of the Boris push.  Photon species carry no charge: they are left out of the sorter stage (only
a merge step sorts them, merging.py), the deposit and the rho bookkeeping.  Events are a function of (seed, step, particle id) -- there is no optical-depth array, nothing is
added to the sort, the migration messages or a checkpoint, and a restart continues exactly.  Two small host reads per
radiating species and step: the event count (the photon store is grown to hold it before the emit launch, with the
reference's 25 % slack) and the emitted count (by which the photon store's ``n`` advances).

A photon species linked to an electron and a positron species (``add_pair_production``) is moved by
``lpa_bw_push_event`` instead -- the push and the pair event test at mid step in one pass over the store --, and
``lpa_bw_create`` behind ``lpa_qed_emit`` writes the pairs into the loose tails of both target stores (which are then
re-sorted) and kills the photons.  The same seed, tables file, host reads and restart rule; the dead photons are
compacted away once they are more than half of the store.
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
    ``_rad_id_base(i, k)`` (first of ``k`` fresh ids of species ``i``); for pair production also ``_rad_mass(i)``,
    ``_rad_arrival_area()`` (slots a sorted store keeps free behind ``n``), ``_rad_appended(i)`` (particles were written
    behind the sorted part: force the re-sort, as the engines' ``_append_device`` does) and ``_rad_rows(i)`` (the store's
    tensors, slot axis last, the row tensor whose row 0 is x first)"""

    # {"pairs": [(ispec, photon_ispec)], "seed", "itime", "id_next", "emitted", "tables"; with pair production also
    # "bw": [(photon, electron, positron)], "created", "bw_dead"}: pickled
    radiation = None
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
        return self.radiation is not None and (any(b == i for _, b in self.radiation["pairs"]) or self.is_pair_source(i))

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
        """the photon pusher of species ``i``: ``lpa_bw_push_event`` if it produces pairs, else ``lpa_push_photons``"""
        if self.is_pair_source(i):
            return self.bw_push_event(i, dt)
        pc = self._rad_part(i, False)
        if pc.n == 0:
            return
        pp = self._rad_pp(i, dt)
        check(self.L.lpa_push_photons(C.byref(pc), C.byref(pp), dt, self.stream), "lpa_push_photons")
        self._rad_log("lpa_push_photons", i)

    # ---- Breit-Wheeler pair production (csrc/lpa_bw.hip) ---------------------------------------------------------
    def add_pair_production(self, photon_ispec, electron_ispec, positron_ispec, seed=0, tables=None):
        """photons of species ``photon_ispec`` decay into pairs: the electron into ``electron_ispec``, the positron into
        ``positron_ispec`` (`Photon.set_bw_pair`, `NonlinearPairProductionLCFA`).  The photon species is from here on
        moved by ``lpa_bw_push_event``; seed and tables are the engine's one set (see ``add_radiation``)"""
        if self.comm.size > 1:
            raise NotImplementedError("pair production on a slab chain (comm.size > 1) is not implemented: the photon "
                                      "store has no migration")
        trio = (int(photon_ispec), int(electron_ispec), int(positron_ispec))
        for i in trio:
            if not 0 <= i < len(self.species):
                raise IndexError(f"add_pair_production names species {i}; the engine has {len(self.species)}")
        if len(set(trio)) != 3:
            raise ValueError("add_pair_production: photon, electron and positron species must differ")
        if any(self._rad_mass(i) <= 0 or self.is_photon(i) for i in trio[1:]):
            raise ValueError("add_pair_production: the electron and positron species must be massive")
        seed = int(seed) & ((1 << 64) - 1)
        st = self.radiation or {"pairs": [], "itime": -1, "id_next": {}, "tables": tables, "seed": seed}
        if (st["seed"], st["tables"]) != (seed, tables):
            raise ValueError("add_pair_production: seed and tables must be those of the engine's radiation")
        if any(t[0] == trio[0] for t in st.get("bw", [])):
            raise ValueError(f"species {trio[0]} produces pairs already")
        if trio[0] in [a for a, _ in st["pairs"]]:
            raise ValueError("a radiating species cannot be a photon species")
        st.setdefault("bw", []).append(trio)
        st.setdefault("created", {})
        self.radiation = st
        self._rad_mark_photon(trio[0])

    def is_pair_source(self, i):
        return self.radiation is not None and any(t[0] == i for t in self.radiation.get("bw", ()))

    def _bw_state(self, a):
        """device scratch of pair-producing photon species ``a``: the pair tables (once per engine), its delta row,
        counters and the count of dead slots its store holds"""
        sc = self.__dict__.get("_rad_scratch") or {}
        self._rad_scratch = sc
        if "pair_rate" not in sc:
            tabs = qed_tables.tables(self.radiation["tables"])
            if "pair_prob_rate_total" not in tabs:
                raise ValueError(f"the table file {self.radiation['tables']} has no pair-production tables")
            sc["pair_tabs"] = tabs
            sc["pair_rate"] = torch.from_numpy(tabs["pair_prob_rate_total"]).to(self.device)
            sc["pair_cum"] = torch.from_numpy(tabs["integral_pair_prob_along_delta"]).to(self.device)
        s = sc.setdefault(("bw", a), {"counters": torch.zeros(4, dtype=torch.int32, device=self.device), "delta": None,
                                      "parent": None, "pending": False})
        need = self._rad_capacity(a)
        if s["delta"] is None or s["delta"].numel() != need:       # (resized with the store: grown or compacted)
            s["delta"] = torch.zeros(need, dtype=torch.float64, device=self.device)
        return sc, s

    def bw_push_event(self, a, dt):
        """``lpa_bw_push_event`` for photon species ``a``: its push and its pair event test in one pass"""
        st = self.radiation
        pc = self._rad_part(a, False)
        if pc.n == 0:
            return
        sc, s = self._bw_state(a)
        s["counters"].zero_()
        qp = qed_params(sc["pair_tabs"], sc["pair_rate"], sc["pair_cum"], dt, st["seed"], st["itime"])
        pp = self._rad_pp(a, dt)
        check(self.L.lpa_bw_push_event(self._g(), C.byref(pc), C.byref(pp), C.byref(qp), s["delta"].data_ptr(),
                                       s["counters"].data_ptr(), self.stream), "lpa_bw_push_event")
        # the photons this step's emit appends behind these pc.n slots carry no delta of this step
        s["pending"], s["n_event"] = True, pc.n
        self._rad_log("lpa_bw_push_event", a)

    def bw_create(self):
        """``lpa_bw_create`` for every photon species whose event kernel ran in this step: behind ``radiation_emit``
        (the reference's order: emission, then pairs).  Returns the pair counts per photon species"""
        st, out = self.radiation, {}
        if st is None:
            return out
        for a, e, p in st.get("bw", ()):
            s = (self.__dict__.get("_rad_scratch") or {}).get(("bw", a))
            if s is None or not s["pending"]:
                continue
            s["pending"] = False
            events = int(s["counters"][0].item())           # host read 1
            out[a] = 0
            if events == 0:
                continue
            n0 = {}
            for b in (e, p):
                n0[b] = self._rad_part(b, False).n
                if n0[b] + events + self._rad_arrival_area() > self._rad_capacity(b):
                    self._rad_reserve(b, int(1.25 * (n0[b] + events)) + self._rad_arrival_area())
            if s["parent"] is None or s["parent"].numel() < events:
                s["parent"] = torch.empty(int(1.25 * events), dtype=torch.int64, device=self.device)
            base = {b: self._rad_id_base(b, events) for b in (e, p)}
            pe, pq = self._rad_part(e, False), self._rad_part(p, False)
            pa = _lib.lpa_particles.from_buffer_copy(self._rad_part(a, False))     # (a copy: the engine may cache its struct)
            pa.n = s["n_event"]
            check(self.L.lpa_bw_create(C.byref(pa), C.byref(pe), C.byref(pq), self._rad_capacity(e), self._rad_capacity(p),
                                       s["delta"].data_ptr(), base[e], base[p], s["parent"].data_ptr(),
                                       s["counters"].data_ptr(), self.stream), "lpa_bw_create")
            self._rad_log("lpa_bw_create", a)
            cnt = s["counters"].tolist()                   # host read 2
            k = cnt[1]
            if cnt[2] or k > events:
                raise _lib.LpaError(f"lpa_bw_create: {cnt[2]} pairs beyond a store, {k} created for {events} events")
            if k:
                # ids in the order of the parents' ids, as radiation_emit does; the kernel used ONE k for both stores, so
                # the same permutation serves both and a pair's ids are a function of the run's history alone
                order = torch.argsort(s["parent"][:k])
                fresh = torch.arange(k, dtype=torch.int64, device=self.device)
                for b in (e, p):
                    self._rad_ids(b)[n0[b]:n0[b] + k][order] = base[b] + fresh
                    self._rad_set_n(b, n0[b] + k)
                    self._rad_appended(b)              # loose tail -> forced re-sort, as _append_device does
            out[a] = k
            st["created"][a] = st["created"].get(a, 0) + k                   # running total per photon species
            # photons consumed by pairs since the store was last compacted (photons absorbed at open faces leave dead slots
            # too and are not counted: the bound "at most half dead" is on the slots consumed by pairs)
            dead = st.setdefault("bw_dead", {})
            dead[a] = dead.get(a, 0) + k
            if 2 * dead[a] > self._rad_part(a, False).n:
                self._bw_compact(a)
                dead[a] = 0
        return out

    def bw_refuse_rebuild(self):
        """called by whoever is about to rebuild the particle stores (the facades' ``upload()`` behind a host callback).
        Between ``lpa_bw_push_event`` and ``lpa_bw_create`` a photon's delta lives in a row indexed by SLOT; a rebuild
        re-packs the live photons and would silently pair the row with other photons"""
        sc = self.__dict__.get("_rad_scratch") or {}
        if any(isinstance(k, tuple) and s["pending"] for k, s in sc.items()):
            raise NotImplementedError("a host (not device_native) callback between the push of a pair-producing photon "
                                      "species and 'qed_create_particles' rebuilds the stores; the pending pair events "
                                      "are indexed by slot and cannot follow.  Use a device_native callback, or a stage "
                                      "outside the species loop")

    def _bw_compact(self, a):
        """drop the dead slots of photon store ``a`` -- it is never sorted, so they accumulate -- keeping the order of
        the live ones: plumbing off the hot path.  The store keeps its capacity (and the delta row its size)"""
        rows = self._rad_rows(a)
        n = self._rad_part(a, False).n
        live = ~torch.isnan(rows[0][0, :n])
        m = int(live.sum().item())
        for t in rows:
            t[..., :m] = t[..., :n][..., live]
        rows[0][:, m:n] = float("nan")
        self._rad_set_n(a, m)


class SimulationRadiationMixin:
    """the radiation links of the ``Simulation`` / ``Simulation3D`` facades: ``Electron(radiation="photons", photon=pho)``
    (`core/species.py:185-243`) becomes ``engine.add_radiation`` in ``initialize()`` (`simulation/simulation.py:425-470`),
    ``Photon.set_bw_pair(electron=, positron=)`` becomes ``engine.add_pair_production``.
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
        for s in self.species:          # (`core/species.py:233-243`: Photon.set_bw_pair)
            pair = getattr(s, "electron", None), getattr(s, "positron", None)
            if pair == (None, None):
                continue
            if any(t is None or not any(t is o for o in self.species) for t in pair):
                raise ValueError(f"Species {s.name}: set_bw_pair needs electron= and positron= species added to the simulation")
            eng.add_pair_production(s.ispec, pair[0].ispec, pair[1].ispec, seed=getattr(self, "random_seed", None) or 0)
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
