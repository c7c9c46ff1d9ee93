"""Per-cell histograms of the fine-element values (include/hmg.h: hmg_cell_histogram, hmg_histogram_bin), stated on the CPU
without any code of the library.

Bins are floating-point buckets: emin < emax and sub_bits s give nreg = (emax - emin) 2^s regular bins with the edges

    E_i = 2^(emin + i div 2^s) (1 + (i mod 2^s) / 2^s),    i = 0 .. nreg        (np.ldexp: every edge an exact double)

and bin(q) = np.searchsorted(E, q, side="right") for every q that is no NaN -- 0 below the first edge, nreg + 1 from the last
edge up --, nreg + 2 for a NaN: nbins = nreg + 3.  The element values q_T are those of tests/_cell_extrema_form.py
(element_values)."""
import numpy as np

PARAMETER_SETS = [(-6, 8, 3), (-20, 12, 5), (0, 1, 0), (-1022, 1023, 0)]


def nreg(emin, emax, sub_bits):
    return (emax - emin) << sub_bits


def nbins(emin, emax, sub_bits):
    return nreg(emin, emax, sub_bits) + 3


def edges(emin, emax, sub_bits):
    i = np.arange(nreg(emin, emax, sub_bits) + 1)
    sub = 1 << sub_bits
    return np.ldexp(1.0 + (i % sub) / float(sub), emin + i // sub)


def bins(q, E):
    """bin of every entry of q for the edges E"""
    q = np.asarray(q, dtype=np.float64)
    b = np.searchsorted(E, q, side="right")
    return np.where(np.isnan(q), len(E) + 1, b).astype(np.int64)


def cell_counts(q, E):
    """counts (Ne, nbins) of the element values q (Ne, nt)"""
    b = bins(q, E)
    n = len(E) + 2
    out = np.zeros((q.shape[0], n), dtype=np.int64)
    for c in range(q.shape[0]):
        out[c] = np.bincount(b[c], minlength=n)
    return out


def value_set(E, seed=0, n=20000):
    """what a binning rule is tried on: n log-uniform values over more than the edges' range, every edge with its predecessor
    and its successor, zeros, infinities and NaNs of either sign, the smallest denormal and the largest double"""
    rng = np.random.default_rng(seed)
    lo, hi = max(np.log2(E[0]) - 3.0, -1070.0), min(np.log2(E[-1]) + 3.0, 1023.9)
    body = np.exp2(rng.uniform(lo, hi, n))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 5e-324, np.finfo(np.float64).max, -1.0, 1.0])
    nan_payload = np.array([0x7ff0000000000001, 0xfff0000000000001, 0x7ff8000000000000, 0xfff8000000000000],
                           dtype=np.uint64).view(np.float64)          # signalling NaNs carry their payload in the low word alone
    return np.concatenate([body, -body[:100], E, np.nextafter(E, -np.inf), np.nextafter(E, np.inf), special, nan_payload])


def quantile_rule(q, sub_bits=3, lo=0.05, hi=0.95):
    """(emin, emax, sub_bits) from the element values themselves: the octaves that hold their 5 % and 95 % quantiles, so that both
    end bins are populated"""
    a, b = np.quantile(q, [lo, hi])
    return int(np.floor(np.log2(a))), int(np.ceil(np.log2(b))), sub_bits


def tail(counts):
    """elements at or above each edge, (Ne, nreg + 1), from counts (Ne, nbins); the NaN bin takes no part"""
    return np.cumsum(counts[:, -2:0:-1], axis=1)[:, ::-1]


def tail_bounds(q, E, delta):
    """per cell and edge the number of elements with q >= E + delta and with q >= E - delta: (Ne, nreg + 1) each"""
    s = np.sort(q, axis=1)
    nt = q.shape[1]
    lower = np.stack([nt - np.searchsorted(row, E + delta, side="left") for row in s])
    upper = np.stack([nt - np.searchsorted(row, E - delta, side="left") for row in s])
    return lower, upper
