"""fp64 numpy restatement of optimal combining: array_covariance, combine_weights and array_combine as
include/gsmcal.h defines them, their a-priori error bounds, and the designed four-dongle case with a co-channel interferer.

  cov[w][i][j] = sum_{n in window w} x_i[n] conj(x_j[n])                        not divided by len
  weights      = dominant eigenvector of Rs, or dominant generalised eigenvector of Rs w = lambda Rn w (numpy.linalg.eigh and
                 cholesky: Rn = L L^H, eigh(L^-1 Rs L^-H), w = L^-H u); |w| = 1, w[ref] real and >= 0
  out[b][n]    = sum_g conj(weights[b][g]) x_g[n]
"""
import numpy as np

U53 = 2.0 ** -53
S_WEIGHTS_SINGULAR = 18


def array_covariance(x, rows, windows):
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    wn = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    sel = x[np.asarray(rows, dtype=int)]
    out = np.zeros((len(wn), len(sel), len(sel)), dtype=np.complex128)
    for w, (start, ln) in enumerate(wn):
        seg = sel[:, start:start + ln]
        with np.errstate(invalid="ignore"):
            out[w] = seg @ seg.conj().T
    return out


def covariance_bound(x, rows, windows):
    """(len + 8) 2^-53 sum_n (|Re x_i| + |Im x_i|)(|Re x_j| + |Im x_j|): the a-priori bound of an fp64 sum of these products in any
    order, with or without fused multiply-adds"""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    wn = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    sel = x[np.asarray(rows, dtype=int)]
    mag = np.abs(sel.real) + np.abs(sel.imag)
    out = np.zeros((len(wn), len(sel), len(sel)))
    for w, (start, ln) in enumerate(wn):
        seg = mag[:, start:start + ln]
        out[w] = (ln + 8) * U53 * (seg @ seg.T)
    return out


def hermitian_from_upper(m):
    """the matrix the library reads: the upper triangle (i <= j) and the real part of the diagonal"""
    m = np.asarray(m, dtype=np.complex128)
    up = np.triu(m, 1)
    return up + up.conj().T + np.diag(np.diag(m).real)


def combine_weights(cov_signal, cov_noise=None, ref=0):
    """-> (weights, info) with info = {status, lambda_1, lambda_2}"""
    rs = hermitian_from_upper(cov_signal)
    g = len(rs)
    nan_out = (np.full(g, np.nan + 1j * np.nan), {"status": S_WEIGHTS_SINGULAR, "lambda_1": np.nan, "lambda_2": np.nan})
    if not np.all(np.isfinite(rs)):
        return nan_out
    if cov_noise is not None:
        rn = hermitian_from_upper(cov_noise)
        if not np.all(np.isfinite(rn)):
            return nan_out
        try:
            L = np.linalg.cholesky(rn)
        except np.linalg.LinAlgError:
            return nan_out
        li = np.linalg.inv(L)
        c = li @ rs @ li.conj().T
        c = 0.5 * (c + c.conj().T)
        lam, v = np.linalg.eigh(c)
        w = np.linalg.solve(L.conj().T, v[:, -1])
    else:
        lam, v = np.linalg.eigh(rs)
        w = v[:, -1]
    if not lam[-1] > 0:
        return nan_out
    w = w / np.linalg.norm(w)
    if abs(w[ref]) > 0:
        w = w * (np.conj(w[ref]) / abs(w[ref]))
    return w, {"status": 0, "lambda_1": float(lam[-1]), "lambda_2": float(lam[-2]) if g > 1 else np.nan}


def sin_angle(w1, w2):
    """sine of the angle between two vectors (the part of w1 outside span(w2): no cancellation near zero)"""
    w1, w2 = w1 / np.linalg.norm(w1), w2 / np.linalg.norm(w2)
    return float(np.linalg.norm(w1 - w2 * np.vdot(w2, w1)))


def array_combine(x, rows, weights, out_len=None):
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    w = np.atleast_2d(np.asarray(weights, dtype=np.complex128))
    out_len = x.shape[1] if out_len is None else out_len
    sel = x[np.asarray(rows, dtype=int), :out_len]
    return w.conj() @ sel


def combine_bound(x, rows, weights, out_len=None):
    """(G + 4) 2^-52 sum_g (|Re w| + |Im w|)(|Re x| + |Im x|) per sample"""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex128))
    w = np.atleast_2d(np.asarray(weights, dtype=np.complex128))
    out_len = x.shape[1] if out_len is None else out_len
    sel = x[np.asarray(rows, dtype=int), :out_len]
    return (w.shape[1] + 4) * 2.0 ** -52 * ((np.abs(w.real) + np.abs(w.imag)) @ (np.abs(sel.real) + np.abs(sel.imag)))


# ---- designed Hermitian matrices for the solver ----------------------------------------------------------------------
def _unitary(rng, g):
    q, r = np.linalg.qr(rng.standard_normal((g, g)) + 1j * rng.standard_normal((g, g)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def designed_matrices(g, seed, general, gap=0.2, cond=300.0):
    """(Rs, Rn or None) with the (generalised) eigenvalues 1, 1 - gap, then down to -0.3 (Rs need not be definite), and
    cond(Rn) = `cond` with log-spaced eigenvalues"""
    rng = np.random.Generator(np.random.Philox(key=[21, seed]))
    lam = np.concatenate([[1.0], np.linspace(1.0 - gap, -0.3, g - 1)]) if g > 1 else np.array([1.0])
    q = _unitary(rng, g)
    c = (q * lam) @ q.conj().T
    c = 0.5 * (c + c.conj().T)
    if not general:
        return c, None
    v = _unitary(rng, g)
    mu = np.logspace(0.0, -np.log10(cond), g) if g > 1 else np.array([0.7])
    rn = (v * mu) @ v.conj().T
    rn = 0.5 * (rn + rn.conj().T)
    L = np.linalg.cholesky(rn)
    rs = L @ c @ L.conj().T
    return 0.5 * (rs + rs.conj().T), rn


# ---- the designed case: four dongles, one wanted signal, one co-channel interferer ----------------------------------
A = np.array([1.0, 0.8 * np.exp(1j * 1.0), 0.5 * np.exp(-1j * 2.0), np.exp(1j * 0.3)])
B = np.array([1.0, np.exp(1j * 2.1), np.exp(-1j * 0.7), np.exp(1j * 1.4)])
NOISE = np.array([0.1, 0.1, 0.1, 1.0])
NWIN = 2048


def true_rn():
    return np.outer(B, B.conj()) + np.diag(NOISE)


def designed_case(seed=0):
    """-> dict: x (4, 2 NWIN): window 0 = signal + interferer + noise, window 1 = interferer + noise; windows; s, the wanted
    signal of window 0 (a unit-modulus +-pi/2 phase walk)"""
    rng = np.random.Generator(np.random.Philox(key=[2100, seed]))
    n = 2 * NWIN
    steps = rng.integers(0, 2, NWIN) * 2 - 1
    s = np.exp(1j * (np.pi / 2) * np.cumsum(steps))
    intf = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    noise = (rng.standard_normal((4, n)) + 1j * rng.standard_normal((4, n))) * np.sqrt(NOISE / 2.0)[:, None]
    x = np.outer(B, intf) + noise
    x[:, :NWIN] += np.outer(A, s)
    return {"x": x, "windows": np.array([[0, NWIN], [NWIN, NWIN]], dtype=np.int64), "s": s}


def sinr_db(w, rn=None):
    """output SINR of the beam w^H x for a unit-power wanted signal with gains A, against the true Rn"""
    rn = true_rn() if rn is None else rn
    return 10.0 * np.log10(abs(np.vdot(w, A)) ** 2 / np.vdot(w, rn @ w).real)


def optimum_sinr_db():
    return 10.0 * np.log10(np.vdot(A, np.linalg.solve(true_rn(), A)).real)


def equal_gain_weights():
    return np.exp(1j * np.angle(A)) / 2.0


def measured_sinr_db(y, s):
    """SINR of a combined stream y over the signal window: the part along the known wanted signal s against the rest"""
    g = np.vdot(s, y) / np.vdot(s, s).real
    rest = y - g * s
    return 10.0 * np.log10(abs(g) ** 2 * np.vdot(s, s).real / np.vdot(rest, rest).real)
