"""Tables of nonlinear Compton emission in the locally-constant-field approximation, in the reference's layout
(`core/qed/optical_depth_tables.py:114-218`): the total rate R(chi) on chi_N = 256 nodes, log10(chi) in [-3, 2], and the
cumulative rate along the photon's energy fraction delta on delta_N = 1024 nodes, log10(delta) in [-3, 0].

    dR/d delta = -(alpha m_e c^2 / hbar) [ Ai1(z) + (2 / z + chi delta sqrt(z)) Ai'(z) ],
    z = (delta / (chi (1 - delta)))^(2/3),   Ai1(z) = int_z^inf Ai

The cumulative rule is the reference's: the first node is ``quad`` over [0, delta_0], every further node adds the
left-Riemann step P(delta_i) (delta_i - delta_{i-1}) -- so a row does not end on the total rate, and the sampler
(csrc/lpa_qed.hip) draws between the row's own first and last node.  The spectrum is evaluated on the whole delta grid at
once (``scipy.special.airy`` / ``airye`` on arrays); what is left per chi are two ``quad`` calls, well under a minute
for all 256 rows on one core; ``generate(workers=...)`` spreads the rows over at most 16 fresh interpreters.

The Breit-Wheeler pair tables have the same layout over the photon's chi and the electron's share delta of its energy
(`optical_depth_tables.py:135-144`; the sampler is csrc/lpa_bw.hip):

    dR/d delta = +(alpha m_e c^2 / hbar) [ Ai1(z) + (2 / z - chi sqrt(z)) Ai'(z) ],   z = (1 / (chi delta (1 - delta)))^(2/3)

The spectrum is symmetric in delta <-> 1 - delta and has no end-point singularity; Ai(z) ~ exp(-8 / (3 chi)) underflows
to exactly 0 for small chi: such rows are all zeros, and that is valid.  The sigmoid sampling variant of the reference
is not part of this module.
"""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np

CHI_N, LOG_CHI_RANGE = 256, (-3.0, 2.0)
DELTA_N, LOG_DELTA_RANGE = 1024, (-3.0, 0.0)
CACHE_PATH = Path(__file__).resolve().parent / "qed_tables_cache.npz"     # next to the built library; not in git

PAIR_KEYS = ("pair_prob_rate_total", "integral_pair_prob_along_delta")

_TABLES = None


_GL = np.polynomial.legendre.leggauss(32)


def airy_tail(z):
    """Ai1(z) = int_z^inf Ai(t) dt for z >= 0, on arrays.  (``scipy.special.itairy`` is good to six digits at z = 1 and
    wrong by orders of magnitude near z = 8, so the tail is integrated here: 32-point Gauss-Legendre on [z, z + S] with S
    chosen so that the integrand has dropped by e^-40 at the far end, on the exponentially scaled ``airye`` -- the
    integrand is entire and decays like exp(-2/3 t^1.5), for which the rule converges to rounding.)"""
    from scipy.special import airye
    z = np.asarray(z, dtype=np.float64)[..., None]
    zeta = 2.0 / 3.0 * z ** 1.5
    span = (1.5 * (zeta + 40.0)) ** (2.0 / 3.0) - z
    t = z + 0.5 * span * (_GL[0] + 1.0)
    with np.errstate(under="ignore"):
        f = airye(t)[0] * np.exp(zeta - 2.0 / 3.0 * t ** 1.5)
        return (0.5 * span * f @ _GL[1])[..., None][..., 0] * np.exp(-zeta[..., 0])


def photon_spectrum(chi, delta):
    """dR / d delta (per unit proper time) of an electron with quantum parameter ``chi``; ``delta`` scalar or array"""
    from scipy.constants import alpha, c, hbar, m_e
    from scipy.special import airy
    delta = np.asarray(delta, dtype=np.float64)
    inner = delta < 1.0                                   # (the reference: P(1) = 0)
    d = np.where(inner, delta, 0.5)
    z = (d / (chi * (1.0 - d))) ** (2.0 / 3.0)
    p = -alpha * m_e * c ** 2 / hbar * (airy_tail(z) + (2.0 / z + chi * d * np.sqrt(z)) * airy(z)[1])
    return np.where(inner, p, 0.0)


def pair_spectrum(chi, delta):
    """dR / d delta (per unit proper time) of a photon with quantum parameter ``chi`` into an electron that takes the
    share ``delta`` of its energy; ``delta`` scalar or array.  P(0) = P(1) = 0"""
    from scipy.constants import alpha, c, hbar, m_e
    from scipy.special import airy
    delta = np.asarray(delta, dtype=np.float64)
    inner = (delta > 0.0) & (delta < 1.0)
    d = np.where(inner, delta, 0.5)
    with np.errstate(under="ignore"):
        z = (1.0 / (chi * d * (1.0 - d))) ** (2.0 / 3.0)
        p = alpha * m_e * c ** 2 / hbar * (airy_tail(z) + (2.0 / z - chi * np.sqrt(z)) * airy(z)[1])
    return np.where(inner, p, 0.0)


def _integral(spectrum, chi, upper, cube, limit=50):
    """int_0^upper of ``spectrum(chi, .)``; ``cube``: through delta = s^3, which takes a delta^(-2/3) end-point
    singularity out of the integrand"""
    from scipy.integrate import quad
    if cube:
        return quad(lambda s: 3.0 * s * s * float(spectrum(chi, s ** 3)), 0.0, upper ** (1.0 / 3.0), epsabs=0.0,
                    epsrel=1e-12, limit=limit)[0]
    import warnings
    from scipy.integrate import IntegrationWarning
    with warnings.catch_warnings():
        # rows next to the underflow edge: the integrand is a few denormals, of which quad cannot make twelve digits
        warnings.simplefilter("ignore", IntegrationWarning)
        return quad(lambda d: float(spectrum(chi, d)), 0.0, upper, epsabs=0.0, epsrel=1e-12, limit=limit)[0]


def total_rate(chi):
    """int_0^1 of the photon spectrum"""
    return _integral(photon_spectrum, chi, 1.0, True, limit=200)


def pair_total_rate(chi):
    """int_0^1 of the pair spectrum (plain ``quad``: no singularity); exactly 0 where the spectrum underflows"""
    return _integral(pair_spectrum, chi, 1.0, False, limit=200)


def cumulative_row(chi, delta_n=DELTA_N, log_delta_min=LOG_DELTA_RANGE[0], spectrum=photon_spectrum):
    """the reference's rule for either spectrum: ``quad`` up to the first node, then left-Riemann steps"""
    delta = np.logspace(log_delta_min, 0.0, delta_n)
    steps = spectrum(chi, delta[1:]) * np.diff(delta)
    first = _integral(spectrum, chi, delta[0], spectrum is photon_spectrum)
    return np.concatenate([[first], first + np.cumsum(steps)])


def _row(args):
    chi, delta_n, log_delta_min = args
    return (total_rate(chi), cumulative_row(chi, delta_n, log_delta_min),
            pair_total_rate(chi), cumulative_row(chi, delta_n, log_delta_min, pair_spectrum))


_ROW_KEYS = ("rate", "cum", "pair_rate", "pair_cum")


def _rows_in_workers(jobs, workers):
    """the rows of ``jobs`` from ``workers`` fresh interpreters (``python -m lambdapic_amd.qed_tables first stop file``),
    each writing its share to a file; None if one of them fails (the caller then computes serially)"""
    import subprocess
    import sys
    import tempfile
    chi = [j[0] for j in jobs]
    bounds = np.linspace(0, len(jobs), workers + 1).astype(int)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(Path(__file__).resolve().parents[1]), os.environ.get("PYTHONPATH", "")]))
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "chi.npy"), np.array(chi))
        procs = [subprocess.Popen([sys.executable, "-m", "lambdapic_amd.qed_tables", tmp, str(a), str(b), str(jobs[0][1]),
                                   repr(jobs[0][2])], env=env, stdout=subprocess.DEVNULL)
                 for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
        try:
            failed = any(p.wait(timeout=600) != 0 for p in procs)
        except subprocess.TimeoutExpired:
            failed = True
        if failed:
            for p in procs:
                p.kill()
            return None
        parts = [np.load(os.path.join(tmp, f"rows_{a}.npz")) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
        return tuple(np.concatenate([f[k] for f in parts]) for k in _ROW_KEYS)


def generate(chi_n=CHI_N, log_chi_range=LOG_CHI_RANGE, delta_n=DELTA_N, log_delta_range=LOG_DELTA_RANGE, workers=1):
    """dict with the reference's key names (``table_gen``'s file).  ``workers`` > 1: the rows are
    spread over that many fresh interpreters (at most 16); should one of them fail, the rows are computed here"""
    jobs = [(x, delta_n, log_delta_range[0]) for x in np.logspace(log_chi_range[0], log_chi_range[1], chi_n)]
    done = _rows_in_workers(jobs, min(int(workers), 16, chi_n)) if workers > 1 else None
    if done is None:
        rows = [_row(j) for j in jobs]
        done = tuple(np.array([r[k] for r in rows]) for k in range(len(_ROW_KEYS)))
    return {
        "photon_prob_rate_total": done[0],
        "integral_photon_prob_along_delta": done[1],
        "pair_prob_rate_total": done[2],
        "integral_pair_prob_along_delta": done[3],
        "chi_N": chi_n, "log_chi_range": tuple(log_chi_range),
        "log_chi_delta": (log_chi_range[1] - log_chi_range[0]) / (chi_n - 1),
        "delta_N": delta_n, "log_delta_range": tuple(log_delta_range),
        "log_delta_delta": (log_delta_range[1] - log_delta_range[0]) / (delta_n - 1),
    }


def load_tables(path):
    """read a table file -- this module's cache or one written by the reference's ``table_gen`` (same key names; the
    pair arrays are read when the file has them)"""
    with np.load(path) as f:
        t = {"photon_prob_rate_total": np.ascontiguousarray(f["photon_prob_rate_total"], dtype=np.float64),
             "integral_photon_prob_along_delta": np.ascontiguousarray(f["integral_photon_prob_along_delta"], dtype=np.float64),
             "chi_N": int(f["chi_N"]), "delta_N": int(f["delta_N"]),
             "log_chi_range": tuple(float(v) for v in f["log_chi_range"]),
             "log_delta_range": tuple(float(v) for v in f["log_delta_range"])}
        for k in PAIR_KEYS:
            if k in f.files:
                t[k] = np.ascontiguousarray(f[k], dtype=np.float64)
    t["log_chi_delta"] = (t["log_chi_range"][1] - t["log_chi_range"][0]) / (t["chi_N"] - 1)
    t["log_delta_delta"] = (t["log_delta_range"][1] - t["log_delta_range"][0]) / (t["delta_N"] - 1)
    if t["photon_prob_rate_total"].shape != (t["chi_N"],) or \
            t["integral_photon_prob_along_delta"].shape != (t["chi_N"], t["delta_N"]):
        raise ValueError(f"{path}: table shapes do not match chi_N / delta_N")
    if not (np.diff(t["integral_photon_prob_along_delta"], axis=1) >= 0).all():      # (flat where the spectrum underflows)
        raise ValueError(f"{path}: a cumulative row decreases")
    if any(k in t for k in PAIR_KEYS):
        if not all(k in t for k in PAIR_KEYS) or t[PAIR_KEYS[0]].shape != (t["chi_N"],) or \
                t[PAIR_KEYS[1]].shape != (t["chi_N"], t["delta_N"]):
            raise ValueError(f"{path}: pair table shapes do not match chi_N / delta_N")
        if not (np.diff(t[PAIR_KEYS[1]], axis=1) >= 0).all():      # (all-zero rows where the spectrum underflows)
            raise ValueError(f"{path}: a cumulative pair row decreases")
    return t


def save_tables(path, t):
    np.savez(path, **t)


def _has_pair_tables(path):
    with np.load(path) as f:
        return all(k in f.files for k in PAIR_KEYS)


def tables(path=None, workers=1):
    """the tables of this process: ``path`` if given, else the cache next to the library, generated on first use
    (``python -m lambdapic_amd.build`` does that with a worker pool; a process that holds a GPU generates serially)"""
    global _TABLES
    if path is not None:
        return load_tables(path)
    if _TABLES is None:
        if not CACHE_PATH.exists() or not _has_pair_tables(CACHE_PATH):      # (a cache from before the pair tables)
            tmp = CACHE_PATH.with_suffix(f".{os.getpid()}.tmp.npz")
            save_tables(tmp, generate(workers=workers))
            os.replace(tmp, CACHE_PATH)
        _TABLES = load_tables(CACHE_PATH)
    return _TABLES


if __name__ == "__main__":      # a worker of generate(): rows [first, stop) of the chi list in `tmp`
    import sys
    _tmp, _a, _b, _dn, _ldm = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5])
    _rows = [_row((x, _dn, _ldm)) for x in np.load(os.path.join(_tmp, "chi.npy"))[_a:_b]]
    np.savez(os.path.join(_tmp, f"rows_{_a}.npz"), **{k: np.array([r[i] for r in _rows]) for i, k in enumerate(_ROW_KEYS)})
