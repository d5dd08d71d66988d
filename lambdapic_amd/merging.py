"""Particle merging of the resident engines -- the host side of csrc/lpa_merge.hip, shared by ``PicEngine2D`` and
``PicEngine3D``.  The reference has no merging; the behaviour is the merge contract of include/lambdapic_amd.h (Vranic et
al., CPC 191 (2015) 65-73: the particles of a cell that share a momentum bin become two with the same weight, momentum
and energy).

A step on which a species is due (``itime % every == 0``) sorts it by its current positions (look-ahead 0, the collision
sort's switch) on the engine's stream, then -- before the push -- launches ``lpa_merge`` once.  The sort drops dead slots,
so the particles a merge removed leave the store at the species' next merge (or sort); a photon store, which nothing else
sorts, is compacted on the way.  The merge is a function of the particles alone: no generator state exists, and a restart
continues exactly.  Merging a charged species moves charge inside a cell: the step is a real-deposit step of the
continuity-rho bookkeeping, and Gauss's law holds only up to that displacement afterwards.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check

PARAMS = ("min_packet", "max_packet", "min_per_cell", "radial_bits", "angular_bins")


class MergingMixin:
    """needs from the engine: ``species``, ``sort(i)``, ``_g()``, ``stream``, ``comm``, ``device``, ``L``, the hooks of
    ``CollisionMixin`` (``_coll_store``, ``_coll_fresh``, ``_coll_sorting``) and ``_merge_unsorted(i)`` (declare that
    store ``i`` has no order a re-sort could build on)"""

    merging = None          # {"species": {ispec: {"every", *PARAMS}}, "itime", "merged": {}, "removed": {}}: pickled
    _merge_scratch = None   # workspace and counters: rebuilt on load
    _merge_launches = None  # optional log (set it to a list): (itime, ispec) of every lpa_merge launch; not pickled

    def add_merging(self, ispec, every=1, min_packet=4, max_packet=32, min_per_cell=8, radial_bits=2, angular_bins=8):
        """merge species ``ispec`` every ``every`` steps (massive or photons).  A packet is ``min_packet`` ..
        ``max_packet`` particles of one cell and one momentum bin (``2 ** radial_bits`` shells per octave of |u|^2,
        ``angular_bins`` x ``angular_bins`` directions per cube face); cells below ``min_per_cell`` are left alone.
        Calling it again for the same species replaces its settings"""
        if self.comm.size > 1:
            raise NotImplementedError("merging on a slab chain (comm.size > 1) is not implemented: a cell's packets need "
                                      "every particle of the cell on one rank, and the photon store has no migration")
        ispec = int(ispec)
        if not 0 <= ispec < len(self.species):
            raise IndexError(f"add_merging names species {ispec}; the engine has {len(self.species)}")
        p = dict(every=int(every), min_packet=int(min_packet), max_packet=int(max_packet), min_per_cell=int(min_per_cell),
                 radial_bits=int(radial_bits), angular_bins=int(angular_bins))
        if p["every"] < 1:
            raise ValueError("every must be >= 1")
        if not (3 <= p["min_packet"] <= p["max_packet"] <= 64 and p["min_per_cell"] >= 0 and 0 <= p["radial_bits"] <= 8
                and 1 <= p["angular_bins"] <= 32):
            raise ValueError("add_merging: need 3 <= min_packet <= max_packet <= 64, min_per_cell >= 0, radial_bits in "
                             "0..8 and angular_bins in 1..32")
        st = self.merging or {"species": {}, "itime": -1, "merged": {}, "removed": {}}
        st["species"][ispec] = p
        st["merged"].setdefault(ispec, 0)
        st["removed"].setdefault(ispec, 0)
        self.merging = st

    def check_merging(self):
        """add the device counters of the merge launches since the last call to the running totals
        ``merging["merged"]`` (packets) and ``["removed"]`` (particles) -- one host read per species; ``merge`` calls it
        behind its sort, whose read-back has synchronised anyway -- and raise if a launch met live particles outside
        the tile of their cell"""
        st = self.merging
        for i, cnt in (self.__dict__.get("_merge_scratch") or {}).get("counters", {}).items():
            merged, removed, skipped, _ = cnt.tolist()
            cnt.zero_()
            st["merged"][i] += merged
            st["removed"][i] += removed
            if skipped:
                raise _lib.LpaError(f"lpa_merge: {skipped} live particles of species {i} were not in the tile of their "
                                    "cell -- the store was not sorted by its current positions")

    def _merging_stage(self):
        """called by the step drivers behind the collision stage and in front of the sorter stage; counts the steps.  A
        due species is sorted here (look-ahead 0): the sorter that follows finds it fresh"""
        st = self.merging
        if st is None:
            return
        st["itime"] += 1
        for i, p in st["species"].items():
            if st["itime"] % p["every"] == 0:
                self.merge(i)

    def merge(self, i):
        """sort species ``i`` by its current positions and merge it once"""
        st = self.merging
        if st is None or i not in st["species"]:
            raise _lib.LpaError(f"no merging registered for species {i}: add_merging first")
        sc = self.__dict__.get("_rad_scratch") or {}
        if any(isinstance(s, dict) and s.get("pending") for s in sc.values()):
            raise _lib.LpaError("lpa_merge with emission or pair events pending: their delta rows are indexed by slot, and "
                                "the merge sort moves the slots")
        pc, _, q, m = self._coll_store(i)
        if pc.n == 0:
            return
        photon = getattr(self, "is_photon", lambda i: False)(i)
        self._coll_sorting = True
        try:
            if photon:
                # nothing else sorts a photon store: its order is as old as its last merge, _bw_compact has re-packed it
                # and the emit kernels have appended to it -- a full sort, no prefix the sort could take over
                self._merge_unsorted(i)
                self.sort(i)
                dead = (self.radiation or {}).get("bw_dead")
                if dead is not None and i in dead:
                    dead[i] = 0                     # (the sort dropped the dead slots)
            elif not self._coll_fresh(i):
                self.sort(i)
        finally:
            self._coll_sorting = False
        self.check_merging()                        # (the previous merge steps' launches)
        pc, tiling, q, m = self._coll_store(i)
        if tiling is None or tiling.n_sorted == 0:
            return
        if q != 0.0:
            self._anchor_pending = True             # rho.py: charge moves inside the cell -- the push that follows re-deposits rho
        scratch = self.__dict__.get("_merge_scratch") or {"counters": {}}
        self._merge_scratch = scratch
        need = self.L.lpa_merge_workspace_bytes(self._g(), tiling.n_sorted)
        if scratch.get("ws") is None or scratch["ws"].numel() < need:
            scratch["ws"] = torch.empty(max(int(1.25 * need), 256), dtype=torch.uint8, device=self.device)
        if i not in scratch["counters"]:
            scratch["counters"][i] = torch.zeros(4, dtype=torch.int32, device=self.device)
        mp = _lib.lpa_merge_params()
        for name in PARAMS:
            setattr(mp, name, st["species"][i][name])
        mp.massless = int(photon or m == 0.0)
        mp.counters = scratch["counters"][i].data_ptr()
        check(self.L.lpa_merge(self._g(), C.byref(pc), C.byref(tiling), C.byref(mp), scratch["ws"].data_ptr(),
                               scratch["ws"].numel(), self.stream), "lpa_merge")
        if self._merge_launches is not None:
            self._merge_launches.append((st["itime"], i))


class SimulationMergingMixin:
    """``add_merging`` of the ``Simulation`` / ``Simulation3D`` facades (no reference counterpart)"""

    def add_merging(self, species, **settings):
        """merge ``species`` (a ``Species`` of this simulation) with the settings of ``MergingMixin.add_merging``; also
        after ``initialize()``.  A second call for the same species replaces its settings"""
        if not any(species is t for t in self.species):
            raise ValueError(f"Species {getattr(species, 'name', species)} not added to simulation")
        regs = self.__dict__.setdefault("_merging", [])
        regs[:] = [r for r in regs if r[0] is not species] + [(species, settings)]
        if self.initialized:
            self._init_merging()

    def _init_merging(self):
        for s, settings in getattr(self, "_merging", ()):
            self.engine.add_merging(s.ispec, **settings)
