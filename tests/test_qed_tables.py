"""LCFA emission tables (lambdapic_amd/qed_tables.py) against a direct ``quad`` of the LCFA integrand, nested like the
reference's own ``int_Ai`` (`core/qed/optical_depth_tables.py:114-133`), and the round trip of a file with the reference's
keys."""
import numpy as np
import pytest
from scipy.constants import alpha, c, hbar, m_e
from scipy.integrate import quad
from scipy.special import airy

from lambdapic_amd import qed_tables

Q = dict(epsabs=0, epsrel=1e-10, limit=200)

def spectrum(chi, delta):
    if delta == 1.0:
        return 0.0
    z = (delta / (chi * (1 - delta))) ** (2 / 3)
    tail = quad(lambda t: airy(t)[0], z, np.inf, **Q)[0]
    return -alpha * m_e * c ** 2 / hbar * (tail + (2 / z + chi * delta * np.sqrt(z)) * airy(z)[1])

def direct(chi, j):
    """entry j of the cumulative row (the contract: quad up to the first node, left-Riemann steps behind it); j = None:
    the total rate"""
    if j is None:
        return quad(lambda s: 3 * s * s * spectrum(chi, s ** 3), 0, 1, **Q)[0]
    delta = np.logspace(-3, 0, qed_tables.DELTA_N)
    first = quad(lambda s: 3 * s * s * spectrum(chi, s ** 3), 0, delta[0] ** (1 / 3), **Q)[0]
    return first + sum(spectrum(chi, delta[i]) * (delta[i] - delta[i - 1]) for i in range(1, j + 1))

# corners, the edges chi = 1e-3 and 1e2, mid-range: (row, column or None for the total rate)
ENTRIES = [(0, None), (255, None), (128, None), (77, None), (0, 0), (0, 1023), (255, 0), (255, 1023), (0, 300), (255, 700),
           (128, 512), (200, 40)]

@pytest.mark.parametrize("row,col", ENTRIES)
def test_entries_match_direct_quadrature(row, col):
    chi = np.logspace(-3, 2, qed_tables.CHI_N)[row]
    got = qed_tables.total_rate(chi) if col is None else qed_tables.cumulative_row(chi)[col]
    want = direct(chi, col)
    print(row, col, abs(got / want - 1))
    # measured agreement over the twelve entries: <= 1.4e-15 (both sides put the same quad rule on integrands that
    # differ only in how the Airy tail is integrated); ten times that
    assert abs(got / want - 1) <= 1.4e-14

def test_load_tables_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    rate, cum = rng.uniform(size=16), np.cumsum(rng.uniform(size=(16, 32)), axis=1)
    np.savez(tmp_path / "optical_depth_tables.npz", photon_prob_rate_total=rate, pair_prob_rate_total=rate,
             integral_photon_prob_along_delta=cum, integral_pair_prob_along_delta=cum, chi_N=16, log_chi_range=(-3.0, 2.0),
             log_chi_delta=5 / 15, delta_N=32, log_delta_range=(-3, 0), log_delta_delta=3 / 31)
    t = qed_tables.load_tables(tmp_path / "optical_depth_tables.npz")
    assert np.array_equal(t["photon_prob_rate_total"], rate) and np.array_equal(t["integral_photon_prob_along_delta"], cum)
    assert (t["chi_N"], t["delta_N"], t["log_chi_range"], t["log_delta_range"]) == (16, 32, (-3.0, 2.0), (-3.0, 0.0))
    qed_tables.save_tables(tmp_path / "again.npz", t)
    u = qed_tables.load_tables(tmp_path / "again.npz")
    assert all(np.array_equal(t[k], u[k]) for k in t)
