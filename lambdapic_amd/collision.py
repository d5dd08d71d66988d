"""Binary Coulomb collisions of the resident engines -- the host side of csrc/lpa_collide.hip, shared by ``PicEngine2D``
and ``PicEngine3D`` (the reference's ``Collision``, `core/collision/collision.py:22-207`, driven by
``Simulation.add_collision`` / the collision stage of ``Simulation.run``, `simulation/simulation.py:577-636,974-978`).

A step on which collisions are due (``itime % every == 0``) is a forced sort step for every species in a group: the sort
bins by the current positions (look-ahead 0) on the engine's stream, then -- before the push -- the Debye arrays are
filled (varying Coulomb logarithm only, which makes it a sort step for EVERY species: the Debye length sums over all) and one ``lpa_collide`` launch per species pair follows, each covering
``dt * every``.  The pairing is a function of (seed, itime, pair index, particle ids): no generator state exists, and a
restart continues exactly.  ``every`` has no twin in the reference, which sorts and collides in every step.
"""
from __future__ import annotations

import ctypes as C
from itertools import combinations

import torch

from . import _lib
from ._lib import check


class CollisionMixin:
    """needs from the engine: ``species``, ``sort(i)``, ``_g()``, ``stream``, ``eps0``, ``comm``, ``device`` and the two
    hooks ``_coll_store(i)`` -> (lpa_particles, lpa_tiling or None, q, m) and ``_coll_fresh(i)`` (is store ``i`` binned
    by its current positions?)"""

    collision = None        # {"pairs": [(i, j)], "enabled": {pair: bool}, "lnLambda", "every", "seed", "itime"}: pickled
    _coll_sorting = False   # a collision sort is running: look-ahead 0 (``_sort_ahead``)
    _coll_launches = None   # optional log (set it to a list): (itime, a, b) of every lpa_collide launch; not pickled

    def add_collision(self, groups, lnLambda=0.0, every=1, seed=0):
        """``groups``: lists of species indices; every unordered pair of a group collides, a species listed twice with
        itself (`collision.py:53-63`).  ``lnLambda`` <= 0: the varying Coulomb logarithm with the Debye length of ALL
        species.  Calling it again adds pairs (the other settings are replaced)."""
        if self.comm.size > 1:
            raise NotImplementedError("collisions on a slab chain (comm.size > 1) are not implemented: a cell's pairs "
                                      "need every particle of the cell on one rank at the collision stage")
        if int(every) < 1:
            raise ValueError("every must be >= 1")
        st = self.collision or {"pairs": [], "enabled": {}, "itime": -1}
        for group in groups:
            for a, b in combinations([int(i) for i in group], 2):
                if not (0 <= a < len(self.species) and 0 <= b < len(self.species)):
                    raise IndexError(f"collision group names species {max(a, b)}; the engine has {len(self.species)}")
                pair = (a, b) if a < b else (b, a)
                if pair not in st["enabled"]:
                    st["pairs"].append(pair)
                    st["enabled"][pair] = True
        st.update(lnLambda=float(lnLambda), every=int(every), seed=int(seed) & ((1 << 64) - 1))
        self.collision = st

    def _coll_pair(self, a, b):
        pair = (int(a), int(b)) if a < b else (int(b), int(a))
        if self.collision is None or pair not in self.collision["enabled"]:
            raise ValueError(f"collision pair {pair} not found")
        return pair

    def enable_collision(self, a, b):
        self.collision["enabled"][self._coll_pair(a, b)] = True

    def disable_collision(self, a, b):
        self.collision["enabled"][self._coll_pair(a, b)] = False

    # ---- the step's side -----------------------------------------------------------------------------------------
    def _coll_species(self):
        """the species a due step sorts by their current positions: those of the enabled pairs -- and, with the varying
        Coulomb logarithm, every species: the Debye length sums over all of them (`collision.py:153-167`)"""
        st = self.collision
        if st["lnLambda"] <= 0 and any(st["enabled"].values()):
            photon = getattr(self, "is_photon", lambda i: False)      # (qed.py: photon stores are never sorted)
            return [i for i in range(len(self.species)) if not photon(i)]
        return sorted({i for p in st["pairs"] if st["enabled"][p] for i in p})

    def check_collision(self):
        """raise if a collision launch since the last check met live particles outside the tile of their cell (device
        counter; one host read -- ``collide`` calls it behind its sorts, whose read-back has synchronised anyway)"""
        cnt = self.__dict__.get("_coll_scratch", {}).get("skipped")
        skipped = int(cnt.item()) if cnt is not None else 0
        if skipped:
            cnt.zero_()
            raise _lib.LpaError(f"lpa_collide: {skipped} live particles were not in the tile of their cell -- a store "
                                "was not sorted by its current positions")

    def _coll_due(self):
        st = self.collision
        return st is not None and st["itime"] % st["every"] == 0 and any(st["enabled"].values())

    def _collision_stage(self, dt):
        """called by the step drivers in front of the sorter stage; counts the steps (``itime`` = the index of the step
        that is running, for all of it).  A due step sorts its species itself (``collide``), with look-ahead 0: the
        sorter that follows finds them fresh"""
        st = self.collision
        if st is None:
            return
        st["itime"] += 1
        if self._coll_due():
            self.collide(dt * st["every"])

    def collide(self, dt):
        """collide every enabled pair once over ``dt``, with the draws of the current collision step"""
        st = self.collision
        if st is None:
            raise _lib.LpaError("no collision registered: add_collision first")
        pairs = [p for p in st["pairs"] if st["enabled"][p]]
        self._coll_sorting = True
        try:
            for i in self._coll_species():
                if not self._coll_fresh(i):
                    self.sort(i)
        finally:
            self._coll_sorting = False
        self.check_collision()          # (the previous collision step's launches)
        stores = {}

        def store(i):
            if i not in stores:
                stores[i] = self._coll_store(i)
            return stores[i]

        scratch = self.__dict__.setdefault("_coll_scratch", {})
        cp = _lib.lpa_collide_params()
        cp.dt, cp.lnLambda, cp.eps0, cp.seed, cp.itime = dt, st["lnLambda"], self.eps0, st["seed"], st["itime"] & 0xFFFFFFFF
        if scratch.get("skipped") is None:
            scratch["skipped"] = torch.zeros(1, dtype=torch.int32, device=self.device)
        cp.skipped = scratch["skipped"].data_ptr()
        if st["lnLambda"] <= 0:
            live = [store(i) for i in range(len(self.species))]
            live = [s for s in live if s[1] is not None]
            ncell = self._coll_ncells()
            if scratch.get("debye") is None or scratch["debye"].shape[1] != ncell:
                scratch["debye"] = torch.zeros((2, ncell), dtype=torch.float64, device=self.device)
            n = len(live)
            if n:
                ps = (C.POINTER(_lib.lpa_particles) * n)(*[C.pointer(s[0]) for s in live])
                ts = (C.POINTER(_lib.lpa_tiling) * n)(*[C.pointer(s[1]) for s in live])
                qs, ms = (C.c_double * n)(*[s[2] for s in live]), (C.c_double * n)(*[s[3] for s in live])
                check(self.L.lpa_collide_debye(self._g(), n, ps, ts, qs, ms, self.eps0, scratch["debye"][0].data_ptr(),
                                               scratch["debye"][1].data_ptr(), cp.skipped, self.stream), "lpa_collide_debye")
            cp.inv_d2 = scratch["debye"][0].data_ptr()
        for index, (a, b) in enumerate(st["pairs"]):
            if (a, b) not in pairs:
                continue
            pa, ta, qa, ma = store(a)
            pb, tb, qb, mb = store(b)
            if ta is None or tb is None:          # an empty store was never sorted: nothing to pair
                continue
            need = self.L.lpa_collide_workspace_bytes(self._g(), ta.n_sorted, tb.n_sorted if a != b else 0)
            if scratch.get("ws") is None or scratch["ws"].numel() < need:
                scratch["ws"] = torch.empty(max(int(need), 256), dtype=torch.uint8, device=self.device)
            cp.pair_index = index
            check(self.L.lpa_collide(self._g(), C.byref(pa), C.byref(ta), qa, ma, C.byref(pb), C.byref(tb), qb, mb,
                                     C.byref(cp), scratch["ws"].data_ptr(), scratch["ws"].numel(), self.stream), "lpa_collide")
            if self._coll_launches is not None:
                self._coll_launches.append((st["itime"], a, b))


class SimulationCollisionMixin:
    """``add_collision`` of the ``Simulation`` / ``Simulation3D`` facades (`simulation/simulation.py:577-636`)"""

    def add_collision(self, collision_groups, lnLambda=0.0, every=1):
        """register collision groups of ``Species``: every unordered pair of a group collides, a species listed twice
        with itself; also after ``initialize()``.  A second call replaces the groups, as in the reference.
        ``lnLambda`` <= 0: varying; ``every``: collide every that many steps over ``dt * every`` (the reference: every
        step)"""
        for group in collision_groups:
            for s in group:
                if not any(s is t for t in self.species):
                    raise ValueError(f"Species {getattr(s, 'name', s)} not added to simulation")
        self._collision_groups = (collision_groups, float(lnLambda), int(every))
        if self.initialized:
            self._init_collision()

    def _init_collision(self):
        cg = getattr(self, "_collision_groups", None)
        if cg:
            self.engine.collision = None
            self.engine.add_collision([[s.ispec for s in g] for g in cg[0]], lnLambda=cg[1], every=cg[2],
                                      seed=getattr(self, "random_seed", None) or 0)
