"""CPU tests of optimal combining: properties of the fp64 restatement in tests/array_ref.py, the library's
host-side gsmcal_combine_weights against it, and the designed four-dongle case.  (The solver header on its own under the
sanitizers: tests/test_array_solver_cpu.py.)

Bars, with their origin:
  weights and lambda_1   sin(angle between the library's and the restatement's weights) and |lambda_1 - ref| / lambda_1
                         <= 100 G 2^-53 cond(Rn) / gap, gap = (lambda_1 - lambda_2) / lambda_1 (cond = 1 without Rn, gap = 1 at G = 1):
                         the first-order perturbation bound of a backward-stable solver; the 100 is an allowance for the solver's
                         constants, not a derived or measured figure.  Largest observed / bar: see DESIGN.md section 21 (printed here)
  residual               |Rs w - lambda_1 Rn w| <= the same factor x |Rs|_F, with no reference involved
  designed case          SINR of the generalised weights (evaluated against the true Rn) within 0.1 dB of the analytic optimum
                         Rn^-1 a -- five times the worst shortfall seen over 20 seeds when the case was designed -- and at least
                         8 dB above co-phased equal gain (measured: 9.6 dB)
"""
import numpy as np
import pytest

import array_ref as ref

SIZES = (1, 2, 5, 17, 64)
worst = {}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_is_hermitian_rank_one_and_additive():
    rng = np.random.Generator(np.random.Philox(key=[21, 1]))
    x = rng.standard_normal((6, 500)) + 1j * rng.standard_normal((6, 500))
    rows = [4, 0, 5, 0]                                            # a row named twice
    c = ref.array_covariance(x, rows, [[0, 500], [0, 200], [200, 300], [7, 0]])
    assert c.shape == (4, 4, 4)
    assert np.array_equal(c[0], c[0].conj().T) and np.all(np.diag(c[0]).imag == 0) and np.all(np.diag(c[0]).real > 0)
    assert np.array_equal(c[0][1], c[0][3]) and c[0][1, 3] == c[0][1, 1]      # the repeated row repeats
    assert not c[3].any()                                          # len = 0
    assert np.all(np.abs(c[1] + c[2] - c[0]) <= 3 * ref.covariance_bound(x, rows, [[0, 500]])[0])       # adjacent windows add up
    # rank one: every row a multiple of one sequence
    gains = np.array([1.0, 2.0 - 1.0j, -0.5j])
    r1 = ref.array_covariance(np.outer(gains, x[0]), [0, 1, 2], [[0, 500]])[0]
    e = np.vdot(x[0], x[0]).real
    assert np.allclose(r1, e * np.outer(gains, gains.conj()), rtol=1e-13, atol=0)
    assert np.linalg.matrix_rank(r1, tol=1e-9 * e) == 1
    w, info = ref.combine_weights(r1)
    assert info["status"] == 0 and ref.sin_angle(w, gains) <= 1e-14 and abs(info["lambda_1"] - e * np.vdot(gains, gains).real) <= 1e-12 * e
    # the beam of that weight vector adds the rows in phase
    y = ref.array_combine(np.outer(gains, x[0]), [0, 1, 2], w)
    assert y.shape == (1, 500) and np.allclose(y[0], np.linalg.norm(gains) * x[0], rtol=1e-13)


# ---- gsmcal_combine_weights against the restatement ------------------------------------------------------------------
def tolerance(g, rn, lam1, lam2):
    cond = 1.0 if rn is None else np.linalg.cond(rn)
    gap = 1.0 if g == 1 else (lam1 - lam2) / lam1
    return 100.0 * g * 2.0 ** -53 * cond / gap, cond, gap


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("G", SIZES)
def test_combine_weights_against_the_restatement(gsmcal_mod, G, general):
    for seed in range(3):
        rs, rn = ref.designed_matrices(G, seed, general)
        refi = G // 2
        want, winfo = ref.combine_weights(rs, rn, refi)
        tol, cond, gap = tolerance(G, rn, winfo["lambda_1"], winfo["lambda_2"])
        assert (G == 1 or gap >= 0.1) and cond <= 1e3
        w, info = gsmcal_mod.combine_weights(rs, rn, ref=refi)
        assert info["status"] == 0 and w.shape == (G,)
        sin, dlam = ref.sin_angle(w, want), abs(info["lambda_1"] - winfo["lambda_1"]) / winfo["lambda_1"]
        rn_ = np.eye(G) if rn is None else rn
        resid = np.linalg.norm(rs @ w - info["lambda_1"] * (rn_ @ w)) / np.linalg.norm(rs)
        key = ("general" if general else "plain", G)
        worst[key] = max(worst.get(key, 0.0), sin / tol, dlam / tol, resid / tol)
        print(f"G {G} general {general} seed {seed}: sin {sin:.3g} dlambda {dlam:.3g} residual {resid:.3g} bar {tol:.3g} sweeps {info['sweeps']}")
        assert sin <= tol and dlam <= tol and resid <= tol
        assert abs(np.linalg.norm(w) - 1.0) <= 8 * 2.0 ** -53 * max(G, 4)                          # the norm
        assert w[refi].imag == 0.0 and w[refi].real >= 0.0                                          # the phase convention
        if G > 1:
            assert abs(info["lambda_2"] - winfo["lambda_2"]) <= tol * winfo["lambda_1"] and 1 <= info["sweeps"] <= 30
        else:
            assert np.isnan(info["lambda_2"]) and w[0] == 1.0
    print("largest observed / bar:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_combine_weights_reads_the_upper_triangle_only(gsmcal_mod):
    rs, rn = ref.designed_matrices(5, 9, True)
    w0, i0 = gsmcal_mod.combine_weights(rs, rn, ref=1)
    junk_s, junk_n = rs.copy(), rn.copy()
    low = np.tril_indices(5, -1)
    junk_s[low], junk_n[low] = np.nan, np.inf
    for i in range(5):                                             # the diagonal's imaginary part is not read either
        junk_s[i, i] = complex(rs[i, i].real, np.nan)
        junk_n[i, i] = complex(rn[i, i].real, 3.0)
    w1, i1 = gsmcal_mod.combine_weights(junk_s, junk_n, ref=1)
    assert i1["status"] == 0 and np.array_equal(w0, w1) and i0 == i1


def test_combine_weights_left_as_found_when_the_reference_weight_is_zero(gsmcal_mod):
    rs = np.diag([3.0, 1.0, 2.0]).astype(np.complex128)            # dominant eigenvector e_0: w[1] is exactly 0
    w, info = gsmcal_mod.combine_weights(rs, ref=1)
    assert info["status"] == 0 and info["lambda_1"] == 3.0 and info["lambda_2"] == 2.0 and abs(w[0]) == 1.0 and w[1] == 0 and w[2] == 0


def test_singular_and_non_finite_inputs_give_status_18_and_nan_weights(gsmcal_mod):
    G = 5
    rs, rn = ref.designed_matrices(G, 4, True)
    bad = []
    for val in (np.nan, np.inf, -np.inf):
        for where in ((0, 0), (1, 3), (4, 4)):
            m = rs.copy(); m[where] = val; bad.append((m, rn)); bad.append((m, None))
            m = rn.copy(); m[where] = val; bad.append((rs, m))
        m = rs.copy(); m[0, 2] = 1.0 + 1j * val; bad.append((m, None))
    bad.append((rs, np.zeros((G, G))))                             # a pivot that is 0
    bad.append((rs, -rn))                                          # ... negative
    semi = rn.copy(); v = np.linalg.eigh(rn)[1][:, 0]; semi = semi - 2.0 * np.linalg.eigh(rn)[0][0] * np.outer(v, v.conj())
    bad.append((rs, semi))                                         # ... negative at the last pivot only (one negative eigenvalue)
    bad.append((-np.eye(G), None))                                 # lambda_1 < 0
    bad.append((np.zeros((G, G)), None))                           # lambda_1 = 0
    bad.append((-np.eye(G), rn))
    bad.append((np.array([[-2.0]]), None))
    bad.append((np.array([[1.0]]), np.array([[0.0]])))
    for m, n in bad:
        w, info = gsmcal_mod.combine_weights(m, n, ref=0)
        assert info["status"] == gsmcal_mod.S_WEIGHTS_SINGULAR == 18 and np.isnan(w.real).all() and np.isnan(w.imag).all(), (m, n, w, info)
        assert ref.combine_weights(m, n, 0)[1]["status"] == 18     # the restatement agrees


def test_combine_weights_argument_errors(gsmcal_mod):
    import ctypes as C
    lib = gsmcal_mod.load()
    ok = np.eye(3, dtype=np.complex128)
    for g, r in ((3, -1), (3, 3), (0, 0), (65, 0), (-1, 0)):
        big = np.eye(max(g, 1), dtype=np.complex128)
        w, info = np.full(2 * max(g, 1), 7.0), np.full(4, 7.0)
        dp = lambda a: a.ctypes.data_as(gsmcal_mod._lib.c_double_p)
        assert lib.gsmcal_combine_weights(dp(big), None, g, r, dp(w), dp(info)) == -1
        assert np.all(w == 7.0) and np.all(info == 7.0)
    w, info = np.full(6, 7.0), np.full(4, 7.0)
    dp = lambda a: a.ctypes.data_as(gsmcal_mod._lib.c_double_p)
    assert lib.gsmcal_combine_weights(None, None, 3, 0, dp(w), dp(info)) == -1
    assert lib.gsmcal_combine_weights(dp(ok), None, 3, 0, None, dp(info)) == -1
    assert lib.gsmcal_combine_weights(dp(ok), None, 3, 0, dp(w), None) == -1
    assert np.all(w == 7.0) and np.all(info == 7.0)
    for kw in (dict(ref=3), dict(ref=-1)):
        with pytest.raises(gsmcal_mod.GsmcalError, match="failed with -1 "):
            gsmcal_mod.combine_weights(ok, **kw)
    with pytest.raises(gsmcal_mod.GsmcalError, match="failed with -1 "):
        gsmcal_mod.combine_weights(np.eye(65))
    assert gsmcal_mod.combine_weights(np.eye(64))[1]["status"] == 0
    assert C.sizeof(C.c_double) == 8


# ---- the designed case ------------------------------------------------------------------------------------------------
def test_designed_case_generalised_weights_reach_the_optimum(gsmcal_mod):
    opt = ref.optimum_sinr_db()
    eg = ref.sinr_db(ref.equal_gain_weights())
    assert abs(opt - 8.644) <= 2e-3 and abs(eg - (-0.96)) <= 5e-3   # the figures of the definition
    case = ref.designed_case(0)
    cov = ref.array_covariance(case["x"], [0, 1, 2, 3], case["windows"])
    w, info = gsmcal_mod.combine_weights(cov[0], cov[1], ref=0)
    want, _ = ref.combine_weights(cov[0], cov[1], 0)
    plain, _ = gsmcal_mod.combine_weights(cov[0], ref=0)
    got = ref.sinr_db(w)
    print(f"optimum {opt:.3f} dB, generalised weights {got:.3f} dB, dominant eigenvector {ref.sinr_db(plain):.3f} dB, equal gain {eg:.3f} dB; "
          f"sin(angle to the restatement) {ref.sin_angle(w, want):.3g}")
    assert info["status"] == 0
    assert opt - got <= 0.1 and got <= opt + 1e-9
    assert got - eg >= 8.0
    assert ref.sinr_db(plain) < eg + 3.0                           # why the noise window is needed: the interferer dominates Rs
