// The three-point solver of csrc/rr_p3p.h on the CPU: the same statements the kernels run, over seeded
// random minimal samples, every solution checked against its own three points.  A program of its own,
// meant to be built with -fsanitize=address,undefined (tests/test_host_pnp.py does): no GPU, no library.
//   p3p_host [samples] [seed]
// Scenes: a 900 px camera, depths 4 .. 12, rotations up to +-0.3 rad per axis, noise-free image points.
// Prints one line:
//   samples N solutions S histogram h0 h1 h2 h3 h4 planted_found F worst_residual R
// and exits 1 where a solution is not a rotation, lies past the solution count without being zero, puts a
// point behind the camera, or does not reproject its three points.  The residual (normalised coordinates) of
// a solution is its root's error times the sample's conditioning: 1e-16 on a simple root, but up to
// sqrt(2^-52) = 1.5e-8 times the conditioning on a root about to merge with its neighbour, which no bound on
// the input excludes.  So: every residual below 1e-3 (a wrong solution is off by 0.1 .. 1), and all but
// 1 % of the 3 S point residuals below 1e-9.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define __host__
#define __device__
#define __forceinline__ inline
#include "rr_p3p.h"

namespace {

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(next() >> 11) * 0x1p-53; }
};

void rot_xyz(double rx, double ry, double rz, double (&R)[9]) {   // Rz Ry Rx
    const double cx = cos(rx), sx = sin(rx), cy = cos(ry), sy = sin(ry), cz = cos(rz), sz = sin(rz);
    R[0] = cz * cy; R[1] = cz * sy * sx - sz * cx; R[2] = cz * sy * cx + sz * sx;
    R[3] = sz * cy; R[4] = sz * sy * sx + cz * cx; R[5] = sz * sy * cx - cz * sx;
    R[6] = -sy;     R[7] = cy * sx;                R[8] = cy * cx;
}

}  // namespace

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 4000;
    Rng rng{argc > 2 ? (uint64_t)atoll(argv[2]) : 9500ull};
    int hist[5] = {0, 0, 0, 0, 0}, total = 0, found = 0, bad = 0, loose = 0;
    double worst = 0.0;
    for (int s = 0; s < n; ++s) {
        double Rt[9], tt[3], h[3][3], X[3][3];
        rot_xyz(rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), Rt);
        for (int i = 0; i < 3; ++i) tt[i] = rng.uniform(-1.0, 1.0);
        for (int k = 0; k < 3; ++k) {
            h[k][0] = (rng.uniform(0.0, 1024.0) - 512.0) / 900.0;
            h[k][1] = (rng.uniform(0.0, 768.0) - 384.0) / 900.0;
            h[k][2] = 1.0;
            const double z = rng.uniform(4.0, 12.0);
            const double xc[3] = {h[k][0] * z - tt[0], h[k][1] * z - tt[1], z - tt[2]};
            for (int i = 0; i < 3; ++i) X[k][i] = Rt[i] * xc[0] + Rt[3 + i] * xc[1] + Rt[6 + i] * xc[2];   // R^T (Xc - t)
        }
        double R[rr::P3P_SOLS][9], t[rr::P3P_SOLS][3];
        const int ns = rr::p3p(h, X, R, t);
        if (ns < 0 || ns > rr::P3P_SOLS) { ++bad; continue; }
        ++hist[ns];
        total += ns;
        bool planted = false;
        for (int k = 0; k < rr::P3P_SOLS; ++k) {
            if (k >= ns) {
                for (int i = 0; i < 9; ++i) bad += R[k][i] != 0.0;
                for (int i = 0; i < 3; ++i) bad += t[k][i] != 0.0;
                continue;
            }
            double ortho = 0.0, dist = 0.0;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    double d = 0.0;
                    for (int c = 0; c < 3; ++c) d += R[k][3 * i + c] * R[k][3 * j + c];
                    ortho = fmax(ortho, fabs(d - (i == j ? 1.0 : 0.0)));
                }
            const double det = R[k][0] * (R[k][4] * R[k][8] - R[k][5] * R[k][7]) - R[k][1] * (R[k][3] * R[k][8] - R[k][5] * R[k][6]) +
                               R[k][2] * (R[k][3] * R[k][7] - R[k][4] * R[k][6]);
            if (!(ortho < 1e-9) || !(det > 0.0)) ++bad;
            for (int p = 0; p < 3; ++p) {
                double y[3];
                for (int i = 0; i < 3; ++i) y[i] = R[k][3 * i] * X[p][0] + R[k][3 * i + 1] * X[p][1] + R[k][3 * i + 2] * X[p][2] + t[k][i];
                if (!(y[2] > 0.0)) { ++bad; continue; }
                const double r = fmax(fabs(y[0] / y[2] - h[p][0]), fabs(y[1] / y[2] - h[p][1]));
                worst = fmax(worst, r);
                if (!(r < 1e-3)) ++bad;
                if (!(r < 1e-9)) ++loose;
            }
            for (int i = 0; i < 9; ++i) dist = fmax(dist, fabs(R[k][i] - Rt[i]));
            for (int i = 0; i < 3; ++i) dist = fmax(dist, fabs(t[k][i] - tt[i]));
            planted = planted || dist < 1e-6;
        }
        found += planted ? 1 : 0;
    }
    printf("samples %d solutions %d histogram %d %d %d %d %d planted_found %d worst_residual %.3g\n", n, total, hist[0], hist[1],
           hist[2], hist[3], hist[4], found, worst);
    if (loose > 3 * total / 100) bad += loose;
    if (bad) printf("FAILED: %d checks\n", bad);
    return bad ? 1 : 0;
}
