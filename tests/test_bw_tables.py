"""LCFA pair tables (lambdapic_amd/qed_tables.py) against a direct nested ``quad`` of the Breit-Wheeler integrand
(`core/qed/optical_depth_tables.py:114-144`); rows with chi >= 0.1 only (below, the rate underflows)."""
import numpy as np
import pytest
from scipy.constants import alpha, c, hbar, m_e
from scipy.integrate import quad
from scipy.special import airy

from lambdapic_amd import qed_tables

Q = dict(epsabs=0, epsrel=1e-10, limit=200)
CHI = np.logspace(-3, 2, qed_tables.CHI_N)

def spectrum(chi, delta):
    if delta in (0.0, 1.0):
        return 0.0
    z = (1 / (chi * delta * (1 - delta))) ** (2 / 3)
    tail = quad(lambda t: airy(t)[0], z, np.inf, **Q)[0]
    return alpha * m_e * c ** 2 / hbar * (tail + (2 / z - chi * np.sqrt(z)) * airy(z)[1])

def direct(chi, j):     # entry j of the cumulative row (quad up to the first node, left-Riemann steps); None: the total rate
    if j is None:
        return quad(lambda d: spectrum(chi, d), 0, 1, **Q)[0]
    delta = np.logspace(-3, 0, qed_tables.DELTA_N)
    first = quad(lambda d: spectrum(chi, d), 0, delta[0], **Q)[0]
    return first + sum(spectrum(chi, delta[i]) * (delta[i] - delta[i - 1]) for i in range(1, j + 1))

# the edges chi = 0.1 (row 103) and 1e2, mid-range: (row, column or None for the total rate)
ENTRIES = [(103, None), (128, None), (200, None), (255, None), (103, 1023), (128, 512), (200, 300), (255, 0), (255, 1023),
           (180, 700)]

@pytest.mark.parametrize("row,col", ENTRIES)
def test_entries_match_direct_quadrature(row, col):
    chi = CHI[row]
    got, want = qed_tables.pair_total_rate(chi) if col is None else qed_tables.cumulative_row(chi, spectrum=qed_tables.pair_spectrum)[col], direct(chi, col)
    # measured agreement over the ten entries: <= 1.3e-15 (both sides put the same quad rule on integrands that differ
    # only in how the Airy tail is integrated); ten times that, the rule of test_qed_tables.py
    assert abs(got / want - 1) <= 1.3e-14

def test_symmetry_underflow_and_round_trip(tmp_path):
    for chi, d in [(0.3, 0.1), (1.0, 0.3), (30.0, 0.01)]:
        # delta (1 - delta) is formed from a rounded 1 - delta: relative error eps, amplified by the exponent
        # (4 / 3) z^1.5 = 4 / (3 chi delta (1 - delta)) of the Airy factors
        amp = 1 + 4 / (3 * chi * d * (1 - d))
        assert abs(qed_tables.pair_spectrum(chi, d) / qed_tables.pair_spectrum(chi, 1 - d) - 1) <= 4 * amp * 2.2e-16
    row0 = qed_tables.cumulative_row(CHI[0], spectrum=qed_tables.pair_spectrum)
    assert qed_tables.pair_total_rate(CHI[0]) == 0.0 and not row0.any() and np.isfinite(row0).all()
    t = qed_tables.generate(chi_n=3, log_chi_range=(-3.0, 1.0), delta_n=8)
    assert t["pair_prob_rate_total"].shape == (3,) and t["integral_pair_prob_along_delta"].shape == (3, 8)
    assert t["pair_prob_rate_total"][0] == 0 and t["pair_prob_rate_total"][2] > 0
    qed_tables.save_tables(tmp_path / "t.npz", t)
    u = qed_tables.load_tables(tmp_path / "t.npz")
    assert all(np.array_equal(t[k], u[k]) for k in qed_tables.PAIR_KEYS)
