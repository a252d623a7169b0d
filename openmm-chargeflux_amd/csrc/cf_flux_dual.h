// cf_flux_dual.h -- the non-periodic branch of flux_term (cf_flux.h) restated over a number type T,
// and the (value, tangent) dual number the Hessian-vector products instantiate it with
// (cf_kernels_batch_hvp.hip; DESIGN.md §4.6, "batched, Hessian-vector products").  With T = Dual and
// the atoms' positions carrying a direction v as their tangents, every charge delta and every entry
// of the term's dq/dx block comes out with its directional derivative along v: forward-mode
// differentiation of the very expressions flux_term evaluates, so the three term kinds need no
// hand-written second derivatives.  cf_flux.h's bodies are not touched (the forward kernels keep
// their code objects); with T = double this is flux_term's arithmetic, operation for operation.
#pragma once

#include "cf_flux.h"

namespace cf {

struct Dual {
    double v, d;   // value, tangent
    __device__ __forceinline__ Dual() : v(0.0), d(0.0) {}
    __device__ __forceinline__ Dual(double v_) : v(v_), d(0.0) {}
    __device__ __forceinline__ Dual(double v_, double d_) : v(v_), d(d_) {}
};

__device__ __forceinline__ Dual operator-(Dual a) { return Dual(-a.v, -a.d); }
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return Dual(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return Dual(a.v - b.v, a.d - b.d); }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return Dual(a.v * b.v, a.d * b.v + a.v * b.d); }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
    const double q = a.v / b.v;
    return Dual(q, (a.d - q * b.d) / b.v);
}
// a plain double on either side: a constant (tangent 0), without the arithmetic on that zero
__device__ __forceinline__ Dual operator+(Dual a, double b) { return Dual(a.v + b, a.d); }
__device__ __forceinline__ Dual operator-(Dual a, double b) { return Dual(a.v - b, a.d); }
__device__ __forceinline__ Dual operator-(double a, Dual b) { return Dual(a - b.v, -b.d); }
__device__ __forceinline__ Dual operator*(Dual a, double b) { return Dual(a.v * b, a.d * b); }
__device__ __forceinline__ Dual operator*(double a, Dual b) { return Dual(a * b.v, a * b.d); }
__device__ __forceinline__ Dual operator/(Dual a, double b) { return Dual(a.v / b, a.d / b); }
__device__ __forceinline__ Dual operator/(double a, Dual b) {
    const double q = a / b.v;
    return Dual(q, -q * b.d / b.v);
}

// sqrt and acos under one name for both number types
__device__ __forceinline__ double num_sqrt(double a) { return sqrt(a); }
__device__ __forceinline__ double num_acos(double a) { return acos(a); }
__device__ __forceinline__ Dual num_sqrt(Dual a) {
    const double s = sqrt(a.v);
    return Dual(s, a.d / (2 * s));
}
__device__ __forceinline__ Dual num_acos(Dual a) { return Dual(acos(a.v), -a.d / sqrt(1 - a.v * a.v)); }

template <class T>
__device__ __forceinline__ T num_dot(const T a[3], const T b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// One flux term without a box: type 0 bond x1-x2, 1 angle x1-x2-x3 (x2 central), 2 water (O, H1, H2)
// = (x1, x2, x3), parameters p[0..5) as flux_term's.  dq[0..3): the charge deltas of the term's
// slots in slot order (a bond has two).  out(e, value): entry e of the term's dq/dx block, the
// reference's entry order (12 entries for a bond, 27 otherwise).
template <class T, class Out>
__device__ __forceinline__ void flux_term_nopbc(int type, const double* __restrict__ p, const T x1[3], const T x2[3],
                                                const T x3[3], T dq[3], Out&& out) {
    if (type == 0) {
        T d[3];
#pragma unroll
        for (int j = 0; j < 3; j++) d[j] = x2[j] - x1[j];
        const T r = num_sqrt(num_dot(d, d));
        const double k = p[0];
        const T q = k * (r - p[1]);
        dq[0] = q; dq[1] = -q; dq[2] = T(0.0);
        const T c = k / r;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const T v = c * d[j];
            out(j, -v); out(3 + j, v); out(6 + j, v); out(9 + j, -v);
        }
    } else if (type == 1) {
        T d21[3], d23[3], d13[3];
#pragma unroll
        for (int j = 0; j < 3; j++) { d21[j] = x1[j] - x2[j]; d23[j] = x3[j] - x2[j]; d13[j] = x3[j] - x1[j]; }
        const T r21_2 = num_dot(d21, d21), r23_2 = num_dot(d23, d23), r13_2 = num_dot(d13, d13);
        const T r21 = num_sqrt(r21_2), r23 = num_sqrt(r23_2);
        const T cost = (r23_2 + r21_2 - r13_2) / 2.0 / r21 / r23;
        const double k = p[0];
        const T q = k * (num_acos(cost) - p[1]);
        dq[0] = q; dq[1] = -2.0 * q; dq[2] = q;
        const T inv_s = 1.0 / num_sqrt(1.0 - cost * cost);
        const T c1 = k * (1.0 / r21 / r23) * inv_s;
        const T c21 = k * cost * inv_s / r21_2;
        const T c23 = k * cost * inv_s / r23_2;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const T v1 = -c1 * d23[j] + c21 * d21[j];
            const T v3 = -c1 * d21[j] + c23 * d23[j];
            const T v2 = -v1 - v3;
            out(j, v1); out(3 + j, v2); out(6 + j, v3);
            out(9 + j, -2.0 * v1); out(12 + j, -2.0 * v2); out(15 + j, -2.0 * v3);
            out(18 + j, v1); out(21 + j, v2); out(24 + j, v3);
        }
    } else {
        T d12[3], d13[3], d23[3];
#pragma unroll
        for (int j = 0; j < 3; j++) { d12[j] = x2[j] - x1[j]; d13[j] = x3[j] - x1[j]; d23[j] = x3[j] - x2[j]; }
        const T r12 = num_sqrt(num_dot(d12, d12)), r13 = num_sqrt(num_dot(d13, d13)), r23 = num_sqrt(num_dot(d23, d23));
        const double k1 = p[0], k2 = p[1], kub = p[2], b0 = p[3], ub0 = p[4];
        const T dq2 = k1 * (r12 - b0) + k2 * (r13 - b0) + kub * (r23 - ub0);
        const T dq3 = k1 * (r13 - b0) + k2 * (r12 - b0) + kub * (r23 - ub0);
        dq[0] = -dq2 - dq3; dq[1] = dq2; dq[2] = dq3;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const T n12 = d12[j] / r12, n13 = d13[j] / r13, n23 = d23[j] / r23;
            const T a12k1 = k1 * n12, a12k2 = k2 * n12, a13k1 = k1 * n13, a13k2 = k2 * n13, ub = kub * n23;
            out(0 + j, a12k1 + a12k2 + a13k1 + a13k2);
            out(3 + j, -a12k1 - a12k2 + 2.0 * ub);
            out(6 + j, -a13k2 - a13k1 - 2.0 * ub);
            out(9 + j, -a12k1 - a13k2);
            out(12 + j, a12k1 - ub);
            out(15 + j, a13k2 + ub);
            out(18 + j, -a12k2 - a13k1);
            out(21 + j, a12k2 - ub);
            out(24 + j, a13k1 + ub);
        }
    }
}

}  // namespace cf
