// Internal constants and the per-image record of the forward intersection (intersect.hip, include/jaicov_intersect.h).
#pragma once

namespace jaicov {

constexpr int ISECT_CHUNK = 128;      // rays staged in LDS at a time; a point with at most this many rays keeps them resident

struct IsectImage {                   // written once per image by the prologue kernel, read by every ray of that image
    double r[9];                      // R(omega, phi, kappa) of PDF:125-135, row-major: r[3 i + j] = r_(i+1)(j+1)
    double X0[3];
    double x0, y0, c;
};

}  // namespace jaicov
