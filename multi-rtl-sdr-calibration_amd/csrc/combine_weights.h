// combine_weights.h -- the host arithmetic of gsmcal_combine_weights: the weights that maximise the SNR (dominant
// eigenvector of a Hermitian covariance) or the SINR (dominant generalised eigenvector of a signal-window covariance against a
// noise-window covariance) of a sum of up to 64 streams.  Plain C++: nothing of HIP and nothing of the library is included, so a
// stand-alone program can use it on its own (tests/test_array_cpu.py builds one under the sanitizers).
//
//   Rs w = lambda Rn w   through   Rn = L L^H (Cholesky),  C = L^-1 Rs L^-H,  C u = lambda u (cyclic complex Jacobi),  w = L^-H u
// Without Rn, C = Rs and w = u.  w is scaled to |w|_2 = 1 and turned so that w[ref] is real and >= 0 (left as found when it is 0).
// Matrices are [G][G] complex, row-major, interleaved re / im; only the upper triangle (i <= j) and the real part of the diagonal
// are read.
#pragma once
#include <cmath>
#include <complex>
#include <vector>

namespace gsmcal_cw {

typedef std::complex<double> cd;

enum { CW_OK = 0, CW_SINGULAR = 18, CW_MAX_G = 64, CW_MAX_SWEEPS = 60 };

// the Hermitian matrix the upper triangle stands for; false when a value read is not finite
inline bool load_hermitian(const double* m, int G, std::vector<cd>& a) {
    a.assign((size_t)G * G, cd(0.0, 0.0));
    for (int i = 0; i < G; ++i)
        for (int j = i; j < G; ++j) {
            const double re = m[2 * ((size_t)i * G + j)], im = i == j ? 0.0 : m[2 * ((size_t)i * G + j) + 1];
            if (!std::isfinite(re) || !std::isfinite(im)) return false;
            a[(size_t)i * G + j] = cd(re, im);
            a[(size_t)j * G + i] = cd(re, -im);
        }
    return true;
}

// a = L L^H, L lower triangular with a real positive diagonal, written over the lower triangle of a (the rest is set to zero);
// false at a pivot that is <= 0 or not finite
inline bool cholesky(std::vector<cd>& a, int G) {
    for (int j = 0; j < G; ++j) {
        double d = a[(size_t)j * G + j].real();
        for (int k = 0; k < j; ++k) d -= std::norm(a[(size_t)j * G + k]);
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double l = std::sqrt(d);
        a[(size_t)j * G + j] = cd(l, 0.0);
        for (int i = j + 1; i < G; ++i) {
            cd s = a[(size_t)i * G + j];
            for (int k = 0; k < j; ++k) s -= a[(size_t)i * G + k] * std::conj(a[(size_t)j * G + k]);
            a[(size_t)i * G + j] = s / l;
        }
        for (int i = 0; i < j; ++i) a[(size_t)i * G + j] = cd(0.0, 0.0);
    }
    return true;
}

// b <- L^-1 b, column by column (b: [G][G])
inline void solve_lower(const std::vector<cd>& L, std::vector<cd>& b, int G) {
    for (int i = 0; i < G; ++i) {
        for (int k = 0; k < i; ++k) {
            const cd l = L[(size_t)i * G + k];
            for (int c = 0; c < G; ++c) b[(size_t)i * G + c] -= l * b[(size_t)k * G + c];
        }
        const double d = L[(size_t)i * G + i].real();
        for (int c = 0; c < G; ++c) b[(size_t)i * G + c] /= d;
    }
}

inline void conj_transpose(std::vector<cd>& a, int G) {
    for (int i = 0; i < G; ++i) {
        a[(size_t)i * G + i] = std::conj(a[(size_t)i * G + i]);
        for (int j = i + 1; j < G; ++j) {
            const cd t = a[(size_t)i * G + j];
            a[(size_t)i * G + j] = std::conj(a[(size_t)j * G + i]);
            a[(size_t)j * G + i] = std::conj(t);
        }
    }
}

// Cyclic Jacobi on the Hermitian a (destroyed: its diagonal ends as the eigenvalues), v = the eigenvectors in columns.  A pivot
// a_pq = |a_pq| e^{j phi} is turned real by diag(1, e^{-j phi}) and annihilated by the real rotation of tan(2 theta) =
// 2 |a_pq| / (a_pp - a_qq), the smaller angle.  A pivot is skipped at |a_pq| <= 2^-53 |a|_F / G: what is left off the diagonal is
// then below 2^-53 |a|_F.  Returns the sweeps taken, -1 when CW_MAX_SWEEPS did not suffice.
inline int jacobi_hermitian(std::vector<cd>& a, std::vector<cd>& v, int G) {
    v.assign((size_t)G * G, cd(0.0, 0.0));
    for (int i = 0; i < G; ++i) v[(size_t)i * G + i] = cd(1.0, 0.0);
    double fro = 0.0;
    for (const cd& z : a) fro += std::norm(z);
    const double tol = std::ldexp(std::sqrt(fro), -53) / G;
    for (int sweep = 0; sweep < CW_MAX_SWEEPS; ++sweep) {
        int turned = 0;
        for (int p = 0; p < G - 1; ++p)
            for (int q = p + 1; q < G; ++q) {
                const cd apq = a[(size_t)p * G + q];
                const double mag = std::abs(apq);
                if (!(mag > tol)) continue;
                ++turned;
                const double app = a[(size_t)p * G + p].real(), aqq = a[(size_t)q * G + q].real();
                const double tau = (aqq - app) / (2.0 * mag);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                const cd e = std::conj(apq) / mag;                 // e^{-j phi}
                const cd se = s * e, ce = c * e;
                // a <- a J, v <- v J with J_pp = c, J_pq = s, J_qp = -s e^{-j phi}, J_qq = c e^{-j phi}
                for (int k = 0; k < G; ++k) {
                    const cd akp = a[(size_t)k * G + p], akq = a[(size_t)k * G + q];
                    a[(size_t)k * G + p] = c * akp - se * akq;
                    a[(size_t)k * G + q] = s * akp + ce * akq;
                    const cd vkp = v[(size_t)k * G + p], vkq = v[(size_t)k * G + q];
                    v[(size_t)k * G + p] = c * vkp - se * vkq;
                    v[(size_t)k * G + q] = s * vkp + ce * vkq;
                }
                // a <- J^H a
                const cd sec = std::conj(se), cec = std::conj(ce);
                for (int k = 0; k < G; ++k) {
                    const cd apk = a[(size_t)p * G + k], aqk = a[(size_t)q * G + k];
                    a[(size_t)p * G + k] = c * apk - sec * aqk;
                    a[(size_t)q * G + k] = s * apk + cec * aqk;
                }
                a[(size_t)p * G + q] = cd(0.0, 0.0);
                a[(size_t)q * G + p] = cd(0.0, 0.0);
                a[(size_t)p * G + p] = cd(a[(size_t)p * G + p].real(), 0.0);
                a[(size_t)q * G + q] = cd(a[(size_t)q * G + q].real(), 0.0);
            }
        if (turned == 0) return sweep;
    }
    return -1;
}

// weights: [G] complex; info: {status, lambda_1, lambda_2, sweeps}.  Returns the status: CW_OK or CW_SINGULAR (weights all NaN).
// The caller has checked 1 <= G <= CW_MAX_G, 0 <= ref < G and the pointers.
inline int combine_weights(const double* cov_signal, const double* cov_noise, int G, int ref, double* weights, double* info) {
    const double nan = std::nan("");
    for (int i = 0; i < 2 * G; ++i) weights[i] = nan;
    info[0] = CW_SINGULAR; info[1] = nan; info[2] = nan; info[3] = 0.0;
    std::vector<cd> c, L, v;
    if (!load_hermitian(cov_signal, G, c)) return CW_SINGULAR;
    if (cov_noise) {
        if (!load_hermitian(cov_noise, G, L) || !cholesky(L, G)) return CW_SINGULAR;
        solve_lower(L, c, G);                                      // L^-1 Rs
        conj_transpose(c, G);                                      // Rs L^-H
        solve_lower(L, c, G);                                      // L^-1 Rs L^-H (Hermitian but for rounding)
        for (int i = 0; i < G; ++i) {
            c[(size_t)i * G + i] = cd(c[(size_t)i * G + i].real(), 0.0);
            for (int j = i + 1; j < G; ++j) {
                const cd m = 0.5 * (c[(size_t)i * G + j] + std::conj(c[(size_t)j * G + i]));
                c[(size_t)i * G + j] = m;
                c[(size_t)j * G + i] = std::conj(m);
            }
        }
        for (const cd& z : c)
            if (!std::isfinite(z.real()) || !std::isfinite(z.imag())) return CW_SINGULAR;
    }
    const int sweeps = jacobi_hermitian(c, v, G);
    info[3] = sweeps < 0 ? (double)CW_MAX_SWEEPS : (double)sweeps;
    if (sweeps < 0) return CW_SINGULAR;
    int top = 0, second = -1;
    for (int i = 1; i < G; ++i)
        if (c[(size_t)i * G + i].real() > c[(size_t)top * G + top].real()) top = i;
    for (int i = 0; i < G; ++i)
        if (i != top && (second < 0 || c[(size_t)i * G + i].real() > c[(size_t)second * G + second].real())) second = i;
    const double l1 = c[(size_t)top * G + top].real();
    info[1] = l1;
    info[2] = second < 0 ? nan : c[(size_t)second * G + second].real();
    if (!(l1 > 0.0) || !std::isfinite(l1)) return CW_SINGULAR;
    std::vector<cd> w((size_t)G);
    for (int i = 0; i < G; ++i) w[i] = v[(size_t)i * G + top];
    if (cov_noise)                                                 // w = L^-H u: back substitution with the upper triangular L^H
        for (int i = G - 1; i >= 0; --i) {
            cd s = w[i];
            for (int k = i + 1; k < G; ++k) s -= std::conj(L[(size_t)k * G + i]) * w[k];
            w[i] = s / L[(size_t)i * G + i].real();
        }
    double nrm = 0.0;
    for (const cd& z : w) nrm += std::norm(z);
    nrm = std::sqrt(nrm);
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return CW_SINGULAR;
    const double mref = std::abs(w[ref]);
    const cd turn = mref > 0.0 ? std::conj(w[ref]) / mref : cd(1.0, 0.0);
    for (int i = 0; i < G; ++i) {
        const cd z = w[i] * turn / nrm;
        weights[2 * i] = z.real();
        weights[2 * i + 1] = i == ref && mref > 0.0 ? 0.0 : z.imag();
    }
    if (mref > 0.0) weights[2 * ref] = std::fabs(weights[2 * ref]);
    info[0] = CW_OK;
    return CW_OK;
}

}  // namespace gsmcal_cw
