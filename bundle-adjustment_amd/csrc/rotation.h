// rotation.h -- R(omega, phi, kappa) = Rx(omega) Ry(phi) Rz(kappa) of the collinearity equations (PDF:125-135), the one place of the
// library's device code that writes its nine entries out.
// The header sets no floating-point contraction of its own: the entries are rounded the way the file that includes it rounds.
// wavealg.h includes it below its `fp contract(off)`, so the start-value kernels get every product and sum rounded on its own, as
// their restatements in tests/ round them; transform.hip includes it as it stands and keeps the compiler's fused products.
#pragma once
#include <hip/hip_runtime.h>

namespace jaicov {

// R (row-major) from the sines and cosines of omega, KAPPA and PHI, in that order: phi's pair comes last.
// What must hold: transform.hip, which leaves contraction on, fuses the second product of R[3] and of R[7] into the first, as the sums
// are written.  The compiler orders the two products of a sum by the rank of their factors, which for parameters is their position,
// before it fuses one; with phi's pair last both sums keep their order.  Whoever changes the parameter list compares the device
// assembly of transform.hip before and after.  The start-value kernels do not fuse, so the order means nothing to their results.
// Every call names its arguments so.., co.., sk.., ck.., sp.., cp..: tests/test_ownership_text.py holds the call sites to that.
__device__ inline void rotation_opk(double so, double co, double sk, double ck, double sp, double cp, double *R) {
    R[0] = cp * ck;                 R[1] = -cp * sk;                R[2] = sp;
    R[3] = co * sk + so * sp * ck;  R[4] = co * ck - so * sp * sk;  R[5] = -so * cp;
    R[6] = so * sk - co * sp * ck;  R[7] = so * ck + co * sp * sk;  R[8] = co * cp;
}

}  // namespace jaicov
