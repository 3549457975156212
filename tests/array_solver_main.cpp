// Stand-alone driver of csrc/combine_weights.h for tests/test_array_cpu.py: the solver on G = 1 and G = 64, with and without a noise
// covariance, built there with -fsanitize=address,undefined.  Nothing of HIP or of libgsmcal.so is needed.
#include <cstdio>
#include <vector>

#include "combine_weights.h"

using gsmcal_cw::cd;

// a Hermitian positive definite matrix: diag + a few rank-one terms from a small generator
static std::vector<double> designed(int G, unsigned seed, double diag) {
    std::vector<cd> m((size_t)G * G, cd(0.0, 0.0));
    unsigned s = seed;
    auto next = [&s]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0 - 0.5; };
    for (int k = 0; k < 3; ++k) {
        std::vector<cd> v((size_t)G);
        for (cd& z : v) z = cd(next(), next());
        for (int i = 0; i < G; ++i)
            for (int j = 0; j < G; ++j) m[(size_t)i * G + j] += (3.0 - k) * v[i] * std::conj(v[j]);
    }
    std::vector<double> out((size_t)2 * G * G);
    for (int i = 0; i < G; ++i)
        for (int j = 0; j < G; ++j) {
            const cd z = m[(size_t)i * G + j] + (i == j ? cd(diag * (1.0 + 0.01 * i), 0.0) : cd(0.0, 0.0));
            out[2 * ((size_t)i * G + j)] = z.real();
            out[2 * ((size_t)i * G + j) + 1] = z.imag();
        }
    return out;
}

static int run(int G, bool general) {
    const std::vector<double> rs = designed(G, 7u + G, 0.05), rn = designed(G, 99u + G, 1.0);
    std::vector<double> w((size_t)2 * G);
    double info[4];
    const int rc = gsmcal_cw::combine_weights(rs.data(), general ? rn.data() : nullptr, G, G - 1, w.data(), info);
    double nrm = 0.0;
    for (double v : w) nrm += v * v;
    printf("G %d general %d status %d lambda_1 %.6g lambda_2 %.6g sweeps %g |w|^2 %.17g w[ref] %.6g %+.6g\n", G, (int)general, rc, info[1], info[2], info[3],
           nrm, w[2 * (G - 1)], w[2 * (G - 1) + 1]);
    if (rc != 0 || !(std::fabs(nrm - 1.0) < 1e-12) || !(w[2 * (G - 1)] >= 0.0) || w[2 * (G - 1) + 1] != 0.0) return 1;
    // a singular noise covariance ends with the status and NaN weights, whatever the size
    std::vector<double> zero((size_t)2 * G * G, 0.0);
    if (gsmcal_cw::combine_weights(rs.data(), zero.data(), G, 0, w.data(), info) != gsmcal_cw::CW_SINGULAR || w[0] == w[0]) return 2;
    return 0;
}

int main() {
    for (int G : {1, 64})
        for (bool general : {false, true}) {
            const int rc = run(G, general);
            if (rc) { printf("failed: %d\n", rc); return rc; }
        }
    puts("solver ok");
    return 0;
}
