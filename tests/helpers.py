"""Shared builders for the parity tests: rebuild field / particle bags from golden fixtures."""
from __future__ import annotations

import numpy as np

from lambdapic_amd.fields import Fields2D, Fields3D
from lambdapic_amd.particles import ParticlesBase

PATTRS = ["x", "y", "z", "w", "ux", "uy", "uz", "inv_gamma"]
PEB = ["ex_part", "ey_part", "ez_part", "bx_part", "by_part", "bz_part"]


def fields2d_from(g, prefix, x0, y0):
    f = Fields2D(int(g["nx"]), int(g["ny"]), float(g["dx"]), float(g["dy"]), float(x0), float(y0),
                 int(g["ng"]))
    for a in f.attrs:
        if prefix + a in g:
            getattr(f, a)[...] = g[prefix + a]
    return f


def fields3d_from(g, prefix):
    f = Fields3D(int(g["nx"]), int(g["ny"]), int(g["nz"]), float(g["dx"]), float(g["dy"]),
                 float(g["dz"]), float(g["x0"]), float(g["y0"]), float(g["z0"]), int(g["ng"]))
    for a in f.attrs:
        if prefix + a in g:
            getattr(f, a)[...] = g[prefix + a]
    return f


def particles_from(g, prefix, names=None):
    names = names or [a for a in PATTRS if prefix + a in g]
    n = g[prefix + names[0]].size
    p = ParticlesBase(0, 0)
    p.initialize(n)
    for a in names:
        getattr(p, a)[:] = g[prefix + a]
    if prefix + "is_dead" in g:
        p.is_dead[:] = g[prefix + "is_dead"]
    if prefix + "_id" in g:
        p._id[:] = g[prefix + "_id"]
    return p


OPEN_FIXTURES = {2: "g18_sync_particles_open_2d", 3: "g19_sync_particles_open_3d"}
OPEN_CASES = [(dim, mix) for dim in (2, 3) for mix in "ab"]


def open_patches(g, mix, load=True):
    """mirror patches of one boundary mix of g18 (2-D) / g19 (3-D) with their PML faces attached and, with ``load``,
    the recorded input particles; -> (patches, spacings, boundary conditions)"""
    from lambdapic_amd.patch import make_patches_2d, make_patches_3d
    npp, npatch = tuple(int(v) for v in g["npp"]), tuple(int(v) for v in g["npatch"])
    d, th, dim = tuple(float(v) for v in g["d"]), int(g["thickness"]), len(npp)
    axes = "xyz"[:dim]
    bc = {a + s: ("periodic" if per else "pml") for a, per in zip(axes, g[mix + "_periodic"]) for s in ("min", "max")}
    n = tuple(a * b for a, b in zip(npp, npatch))
    P = make_patches_2d(*n, *d, *npatch, 3, boundary_conditions=bc, cpml_thickness=th) if dim == 2 else \
        make_patches_3d(n, d, npatch, 3, boundary_conditions=bc, cpml_thickness=th)
    assert np.array_equal(np.stack([p.neighbor_ipatch for p in P]), g[mix + "_neighbor_ipatch"])
    if load:
        for k, p in enumerate(P):
            q = p.particles[0]
            q.initialize(g[f"{mix}_pin{k}_x"].size)
            for a in list(axes) + ["ux", "w", "_id", "is_dead"]:
                getattr(q, a)[:] = g[f"{mix}_pin{k}_{a}"]
    return P, d, bc


def check_open_out(g, mix, P):
    """the particle bags after one sync == the reference's, slot for slot and bit for bit: is_dead, every attribute of
    the live slots, and NaN exactly where the reference has NaN"""
    axes = "xyz"[: len(g["npp"])]
    for k, p in enumerate(P):
        q = p.particles[0]
        assert q.npart == g[f"{mix}_pout{k}_x"].size, k
        assert np.array_equal(q.is_dead, g[f"{mix}_pout{k}_is_dead"]), k
        live = ~q.is_dead
        for a in list(axes) + ["ux", "w", "_id"]:
            assert np.array_equal(getattr(q, a)[live].view(np.uint64), g[f"{mix}_pout{k}_{a}"][live].view(np.uint64)), (k, a)
        for a in axes:
            assert np.array_equal(np.isnan(getattr(q, a)), np.isnan(g[f"{mix}_pout{k}_{a}"])), (k, a)


def assert_close(actual, expected, rtol, scale=None, what=""):
    """|a-e| <= rtol * scale, scale defaulting to max|e|; NaN patterns must coincide."""
    a, e = np.asarray(actual, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    assert a.shape == e.shape, what
    na, ne = np.isnan(a), np.isnan(e)
    assert np.array_equal(na, ne), f"{what}: NaN pattern differs"
    if scale is None:
        scale = np.max(np.abs(e[~ne])) if (~ne).any() else 1.0
    if scale == 0:
        scale = 1.0
    err = np.max(np.abs(a[~ne] - e[~ne])) / scale if (~ne).any() else 0.0
    assert err <= rtol, f"{what}: err {err:.3e} > {rtol:.1e} (scale {scale:.3e})"
    return err
