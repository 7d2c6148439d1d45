"""Shared by the float-channel tests: the numpy restatement of the generator
(ldpcgputegra_amd/csrc/awgn_f32.h), the way a test reaches a chosen u through
first_cw, and the committed tail indices."""
import numpy as np
from scipy.stats import norm as _norm

M64 = (1 << 64) - 1
KEY_MUL = 0xD1B54A32D192ED03
_C0, _C1, _C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_I1, _I2 = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)

# the generator's region boundary (AWGN_F32_U_LO / _U_HI of awgn_f32.h): the last
# u of the lower tail and the last u of the central region
U_LO, U_HI = 322122546, 3972844748

SIGMA_1DB = 0.8912509381337456    # sigma of Eb/N0 = 1 dB at rate 1/2
QPSK = 0.707106781


def splitmix64(x):
    """numpy uint64 array -> uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(_C0)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(_C1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(_C2)
        return x ^ (x >> np.uint64(31))


def _unsplitmix64(x):
    """Python int inverse of splitmix64 (it is a bijection of 64-bit words)."""
    x ^= (x >> 31) ^ (x >> 62)
    x = (x * _I2) & M64
    x ^= (x >> 27) ^ (x >> 54)
    x = (x * _I1) & M64
    x ^= (x >> 30) ^ (x >> 60)
    return (x - _C0) & M64


def index_of(u, seed, low=0):
    """An element index whose u is `u` under `seed` (low: the hash's other 32 bits)."""
    return _unsplitmix64(((int(u) << 32) | low) & M64) ^ ((seed * KEY_MUL) & M64)


def u_of(n, batch, seed, first_cw=0):
    """u [batch, n] of codewords first_cw .., in uint64 arithmetic."""
    with np.errstate(over="ignore"):
        idx = (np.uint64(first_cw & M64) + np.arange(batch, dtype=np.uint64))[:, None] * np.uint64(n) \
            + np.arange(n, dtype=np.uint64)[None, :]
        return splitmix64(idx ^ np.uint64((seed * KEY_MUL) & M64)) >> np.uint64(32)


def t_of(u, sigma, amp, norm):
    """The restatement's double t for bit 0: norm * (-amp + sigma * ppf((u + 0.5) 2^-32))."""
    z = _norm.ppf((u.astype(np.float64) + 0.5) * 2.0 ** -32)
    return norm * (-amp + sigma * z)


def near_rounding_boundary(t, rel=1e-9):
    """True where the double t lies within rel * |t| of a midpoint between two
    adjacent floats: there a 1e-9 error of Phi^-1 may round the other way."""
    f = t.astype(np.float32)
    lo = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2
    hi = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    return np.minimum(np.abs(t - lo), np.abs(t - hi)) <= rel * np.abs(t)


def restate(n, batch, seed, sigma, amp=1.0, norm=1.0, first_cw=0, codeword=None):
    """(y float32 [batch, n], excusable bool [batch, n]) of the numpy restatement."""
    t = t_of(u_of(n, batch, seed, first_cw), sigma, amp, norm)
    y = t.astype(np.float32)
    if codeword is not None:
        y = np.where(np.asarray(codeword).reshape(batch, n) != 0, -y, y)
    return y, near_rounding_boundary(t)


def quantize(y, factor=8, sat=31):
    """CFastFixConversion::generate's rule: the float product truncated, then clamped."""
    return np.clip(np.trunc(np.float32(factor) * y), -sat, sat).astype(np.int8)


# Elements of the 648-bit code whose u lies below 2^6 or above 2^32 - 2^6, under
# seed TAIL_SEED: (first_cw, position, u).  Found once by inverting the hash
# (index_of) for the wanted u; the tests recompute u from (first_cw, position).
TAIL_SEED = 7
TAIL_N = 648
TAILS = (
    (12643602617101592, 529, 0),
    (7281682647109159, 165, 1),
    (2212076598667685, 400, 5),
    (24998565656156327, 245, 63),
    (3693462697742761, 413, 4294967295),
    (17534135450225974, 293, 4294967294),
    (18994746187046492, 6, 4294967289),
    (1918400548589032, 25, 4294967232),
)

# the (seed, Eb/N0, frames) of the ldpc_sim comparison of the -f32q chain with the default one, 648x324
SIM_SEED, SIM_EBN0, SIM_FRAMES = 1, 2.0, 2048
