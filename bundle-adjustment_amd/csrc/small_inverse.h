// small_inverse.h -- inverse of a d x d matrix, d <= 7 (the rank of a datum border), on the host: Gauss-Jordan with partial pivoting.
// One elimination; the two callers differ in the pivots they refuse.
#pragma once
#include <math.h>

#include <algorithm>
#include <cmath>

namespace jaicov {

// refuse(p): the pivot p of a column (its entry of largest magnitude) ends the inversion with `false`
template <typename Refuse>
inline bool gauss_jordan_inverse(int d, const double *S, double *Sinv, Refuse refuse) {
    double a[7][14];
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) { a[i][j] = S[i * d + j]; a[i][d + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < d; c++) {
        int piv = c;
        for (int r = c + 1; r < d; r++)
            if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
        if (refuse(a[piv][c])) return false;
        if (piv != c)
            for (int j = 0; j < 2 * d; j++) std::swap(a[c][j], a[piv][j]);
        const double inv = 1.0 / a[c][c];
        for (int j = 0; j < 2 * d; j++) a[c][j] *= inv;
        for (int r = 0; r < d; r++) {
            if (r == c) continue;
            const double f = a[r][c];
            if (f != 0.0)
                for (int j = 0; j < 2 * d; j++) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) Sinv[i * d + j] = a[i][d + j];
    return true;
}

// the solve's border algebra (engine_solve.hip): only an exactly zero pivot is refused
inline bool small_inverse(int d, const double *S, double *Sinv) {
    return gauss_jordan_inverse(d, S, Sinv, [](double p) { return p == 0.0; });
}

// the datum transformation (datum.hip): false when a pivot falls to 1e-12 of the largest entry (the datum rows do not fix the
// frame: collinear or coincident datum points), or when that entry is not finite and positive
inline bool datum_small_inverse(int d, const double *M, double *Minv) {
    double mx = 0.0;
    for (int i = 0; i < d * d; i++) mx = std::max(mx, fabs(M[i]));
    if (!(mx > 0.0) || !std::isfinite(mx)) return false;
    return gauss_jordan_inverse(d, M, Minv, [mx](double p) { return !(fabs(p) > 1e-12 * mx); });
}

}  // namespace jaicov
