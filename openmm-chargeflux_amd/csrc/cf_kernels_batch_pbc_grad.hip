// cf_kernels_batch_pbc_grad.hip -- cf_compute_batch_periodic_vjp: the reverse-mode product of the
// periodic batch (cf_kernels_batch_pbc.hip) with respect to the base charges and the flux parameters
// ("batched, periodic, parameter gradients").  Per conformation and box, with
// cotangents e_bar (scalar), q_bar[N] and v = F_bar[N][3], the scalar
// L = e_bar E + sum q_bar_i q_i + sum v_i . F_i has
//     dL/d(base charge i) = a_i = e_bar g_i + q_bar_i - h_i
//     g_i = dE/dq_i = ke sum_j phi_ij q_j - 2 c_s q_i + sum_k 2 c_k Re[conj(e_i) S(k)]
//     h_i = D_v g_i = ke sum_j (phi_ij qdot_j + phi'_ij rdot_ij q_j) - 2 c_s qdot_i
//                     + sum_k 2 c_k Re[conj(e_i) (Sdot(k) - i kappa_i S(k))]
// with d_ij the minimum image of x_i - x_j, r = |d_ij|, rdot_ij = d_ij . (v_i - v_j) / r,
// c_s = ke alpha / sqrt(pi), qdot = D_v q, e_i = e^{i k.x_i}, kappa_i = k . v_i,
// S = sum_j q_j e_j, Sdot = sum_j (qdot_j + i q_j kappa_j) e_j, c_k = (4 pi ke / V) exp(-k^2 / 4 alpha^2) / k^2
// over the forward path's half-space k set (k from the box diagonals), and
//     excluded pair (any distance)     phi = -erf(alpha r) / r
//                                      phi' = erf(alpha r) / r^2 - (2 alpha / sqrt pi) e^{-alpha^2 r^2} / r
//     other pairs within the cutoff    phi = erfc(alpha r) / r
//                                      phi' = -erfc(alpha r) / r^2 - (2 alpha / sqrt pi) e^{-alpha^2 r^2} / r
// Every flux parameter's gradient is the non-periodic expression in a and g of its atoms
// (cf_kernels_batch_grad.hip), with the term geometry and its tangent from minimum-image vectors.
// A pass is k_bp_flux, k_b_charges, k_bp_tables (as they are), then k_bpg_tangent, k_bpg_sfac,
// k_bpg_pairs, k_bpg_recip, k_bpg_terms: at most eight launches whatever nconf.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N, the topology and kmax: a
// conformation's gradients are bitwise the same alone, in any batch and under any chunking.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms, khalf and the launch's own nconf: no device guard bits.
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

// ---------------------------------------------------------------------------------
// term geometry and its tangent along v: term_geometry of cf_kernels_batch_grad.hip with every
// difference vector the minimum image in the conformation's box (L, T) -- the delta_r calls
// flux_term makes with pbc = 1, in its order (delta_r(a, b) = b - a).  x[] holds the value each
// parameter group multiplies, xd[] its tangent (bond r; angle theta; water r12, r13, r23);
// vel == nullptr: xd = 0.  A definition of its own rather than a template shared with the
// non-periodic kernels: instantiated from a shared template, k_bg_tangent and k_bg_terms compiled to
// different code (other counts of v_add_f64 / v_fma_f64 / v_mul_f64), and their results are to stay
// as they are; left alone, cf_kernels_batch_grad.hip compiles to the object it was.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(double3 a, double3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double3 sub3(double3 a, double3 b) { return make_double3(a.x - b.x, a.y - b.y, a.z - b.z); }

__device__ __forceinline__ void term_geometry_pbc(int4 ti, const double* __restrict__ pos,
                                                  const double* __restrict__ vel, double3 L, double3 T, double x[3],
                                                  double xd[3]) {
    x[0] = x[1] = x[2] = 0.0;
    xd[0] = xd[1] = xd[2] = 0.0;
    if (ti.x == 0) {  // bond p1-p2
        const double3 d = delta_r(ld3(pos, ti.y), ld3(pos, ti.z), L, 1, T);
        const double r = sqrt(dot3(d, d));
        x[0] = r;
        if (vel) xd[0] = dot3(d, sub3(ld3(vel, ti.z), ld3(vel, ti.y))) / r;
    } else if (ti.x == 1) {  // angle p1-p2-p3, p2 central
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double3 d21 = delta_r(x2, x1, L, 1, T), d23 = delta_r(x2, x3, L, 1, T), d13 = delta_r(x1, x3, L, 1, T);
        const double r21_2 = dot3(d21, d21), r23_2 = dot3(d23, d23), r13_2 = dot3(d13, d13);
        const double r21 = sqrt(r21_2), r23 = sqrt(r23_2);
        const double cost = (r23_2 + r21_2 - r13_2) / 2 / r21 / r23;
        x[0] = acos(cost);
        if (vel) {
            const double3 v1 = ld3(vel, ti.y), v2 = ld3(vel, ti.z), v3 = ld3(vel, ti.w);
            const double s21 = dot3(d21, sub3(v1, v2)), s23 = dot3(d23, sub3(v3, v2)), s13 = dot3(d13, sub3(v3, v1));
            // c = u / (2 r21 r23), u = r23^2 + r21^2 - r13^2:  cdot = udot / (2 r21 r23) - c (r21dot / r21 + r23dot / r23)
            const double cdot = (s23 + s21 - s13) / r21 / r23 - cost * (s21 / r21_2 + s23 / r23_2);
            xd[0] = -cdot / sqrt(1 - cost * cost);
        }
    } else {  // water O,H1,H2
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double3 d12 = delta_r(x1, x2, L, 1, T), d13 = delta_r(x1, x3, L, 1, T), d23 = delta_r(x2, x3, L, 1, T);
        const double r12 = sqrt(dot3(d12, d12)), r13 = sqrt(dot3(d13, d13)), r23 = sqrt(dot3(d23, d23));
        x[0] = r12; x[1] = r13; x[2] = r23;
        if (vel) {
            const double3 v1 = ld3(vel, ti.y), v2 = ld3(vel, ti.z), v3 = ld3(vel, ti.w);
            xd[0] = dot3(d12, sub3(v2, v1)) / r12;
            xd[1] = dot3(d13, sub3(v3, v1)) / r13;
            xd[2] = dot3(d23, sub3(v3, v2)) / r23;
        }
    }
}

// ---------------------------------------------------------------------------------
// 3. charge tangents: k_bg_tangent with the conformation's box (term_geometry_pbc: the
//    minimum-image vectors of flux_term with pbc = 1).  One lane per (conformation, atom), the
//    atom's charge slots in qcsr slot order.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpg_tangent(int n, int nb, int na, const int4* __restrict__ tidx,
                                                     const double* __restrict__ tpar, const int* __restrict__ qs,
                                                     const int* __restrict__ qslot, const double* __restrict__ pos_all,
                                                     const double* __restrict__ boxes, const double* __restrict__ v_all,
                                                     double* __restrict__ qdot_all) {
    const size_t c = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* vel = v_all + c * 3 * (size_t)n;
    double3 L, T;
    load_box(boxes, c, L, T);
    double qd = 0;
    for (int k = qs[i]; k < qs[i + 1]; k++) {
        const int s = qslot[k];
        int t, role;
        if (s < 2 * nb) { t = s >> 1; role = s & 1; }
        else { const int u = s - 2 * nb; t = nb + u / 3; role = u % 3; }   // angles then waters: 3 slots each
        const int4 ti = tidx[t];
        const double* p = tpar + 5 * t;
        double x[3], xd[3];
        term_geometry_pbc(ti, pos, vel, L, T, x, xd);
        double d;
        if (ti.x == 0) {
            d = p[0] * xd[0];
            if (role) d = -d;
        } else if (ti.x == 1) {
            d = p[0] * xd[0];
            if (role == 1) d = -2 * d;
        } else {
            const double d2 = p[0] * xd[0] + p[1] * xd[1] + p[2] * xd[2];
            const double d3 = p[0] * xd[1] + p[1] * xd[0] + p[2] * xd[2];
            d = role == 0 ? -d2 - d3 : (role == 1 ? d2 : d3);
        }
        qd += d;
    }
    qdot_all[c * (size_t)n + i] = qd;
}

// ---------------------------------------------------------------------------------
// 5. structure factors: k_bp_sfac's shape, one lane per (conformation, k), the atoms in atom
//    order.  With a force cotangent S and Sdot are summed in the same sweep:
//    Sdot = sum_j (qdot_j + i q_j kappa_j) e_j, kappa_j = k . v_j.  Output per k: coef = 2 c_k S and
//    coefd = 2 c_k Sdot; no energy terms.
// ---------------------------------------------------------------------------------
template <bool HAS_V>
__global__ void __launch_bounds__(256) k_bpg_sfac(int n, int KX, int KY, int KZ, long khalf, double ke, double one_a2,
                                                  const double* __restrict__ boxes, const double* __restrict__ q_all,
                                                  const double* __restrict__ v_all, const double* __restrict__ qdot_all,
                                                  const double2* __restrict__ tab_all, double2* __restrict__ coef_all,
                                                  double2* __restrict__ coefd_all) {
    const size_t c = blockIdx.y;
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= khalf) return;
    int nx, ny, nz;
    half_space_k(k, KY, KZ, nx, ny, nz);
    double3 L, T;
    load_box(boxes, c, L, T);
    const double kx = nx * (2.0 * kPi / L.x), ky = ny * (2.0 * kPi / L.y), kz = nz * (2.0 * kPi / L.z);
    const int KS = KX + KY + KZ;
    const double2* row = tab_all + c * (size_t)n * KS;
    const double* q = q_all + c * (size_t)n;
    const double* vel = HAS_V ? v_all + c * 3 * (size_t)n : nullptr;
    const double* qdot = HAS_V ? qdot_all + c * (size_t)n : nullptr;
    double cs = 0, ss = 0, cd = 0, sd = 0;
    for (int i = 0; i < n; i++) {
        const double2 e = phase(row + (size_t)i * KS, 1, KX, KY, nx, ny, nz);
        const double qi = q[i];
        cs += qi * e.x;
        ss += qi * e.y;
        if (HAS_V) {
            const double qk = qi * (kx * vel[3 * i] + ky * vel[3 * i + 1] + kz * vel[3 * i + 2]);
            const double qd = qdot[i];
            cd += qd * e.x - qk * e.y;
            sd += qd * e.y + qk * e.x;
        }
    }
    const double k2 = kx * kx + ky * ky + kz * kz;
    const double eak = exp(-k2 * 0.25 * one_a2) / k2;
    const double cst = 4.0 / L.x / L.y / L.z * kPi * ke;   // RCK:517
    coef_all[c * (size_t)khalf + k] = make_double2(2.0 * cst * eak * cs, 2.0 * cst * eak * ss);
    if (HAS_V) coefd_all[c * (size_t)khalf + k] = make_double2(2.0 * cst * eak * cd, 2.0 * cst * eak * sd);
}

// ---------------------------------------------------------------------------------
// 6. direct space: the shape of k_bp_pairs / k_bg_pairs.  A block is kPgI = 64 i-atoms of one
//    conformation, one per lane, in each of its four waves; the j-atoms pass through LDS in tiles
//    of 256 -- (x, y, z, q) and, with a force cotangent, (v, qdot) -- and wave w takes entries
//    [64 w, 64 w + 64) of every tile.  Per pair: delta_r minimum image with the conformation's
//    box, then an excluded partner gets the erf pair of (phi, phi') at any distance, any other
//    partner within the cutoff the erfc pair (erfc_exp, the handle's erfcx table in LDS).  The
//    four waves' partial sums are added as (w0 + w1) + (w2 + w3), then the self terms; the pair
//    parts of g and h go to the workspace (k_bpg_recip finishes them).  No LJ work.
//    HAS_V = false (no force cotangent): h = 0, only g is summed (no v / qdot traffic or
//    arithmetic; the choice is an instantiation, not a branch in the j loop).
//    LDS: table 8256 B + two j tiles 16384 B + partial sums 3072 B = 27.1 KiB, below k_bp_pairs'
//    29.1 KiB: the forward pair kernel's occupancy.
// ---------------------------------------------------------------------------------
constexpr int kPgI = 64;
constexpr int kPgJ = 256;

template <bool HAS_V>
__global__ void __launch_bounds__(kPgJ) k_bpg_pairs(int n, double ke, double alpha, double rc2, double erfc_scale,
                                                    const double* __restrict__ erfc_tab,
                                                    const double* __restrict__ boxes,
                                                    const double* __restrict__ pos_all, const double* __restrict__ q_all,
                                                    const double* __restrict__ v_all, const double* __restrict__ qdot_all,
                                                    const int* __restrict__ ex_start, const int* __restrict__ ex_list,
                                                    double* __restrict__ g_all, double* __restrict__ h_all) {
    __shared__ double tab[kErfcMaxM * (kErfcDeg + 1)];
    __shared__ double4 sp[kPgJ];
    __shared__ double4 sv[HAS_V ? kPgJ : 1];
    __shared__ double red[3][2][kPgI];   // partial sums of waves 1..3
    for (int e = threadIdx.x; e < kErfcMaxM * (kErfcDeg + 1); e += kPgJ) tab[e] = erfc_tab[e];
    const size_t c = blockIdx.y;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    const double* vel = HAS_V ? v_all + c * 3 * (size_t)n : nullptr;
    const double* qdot = HAS_V ? qdot_all + c * (size_t)n : nullptr;
    double3 L, T;
    load_box(boxes, c, L, T);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kPgI + lane;
    const bool active = i < n;
    double3 xi = make_double3(0, 0, 0), vi = make_double3(0, 0, 0);
    double qi = 0, qdi = 0;
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        xi = ld3(pos, i);
        qi = q[i];
        if (HAS_V) { vi = ld3(vel, i); qdi = qdot[i]; }
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int k = 0; k < kMaxRegExcl; k++) reg[k] = k < exc ? ex_list[ex0 + k] : -1;
    const double two_over_sqrtpi = 1.1283791670955126;
    double g = 0, hs = 0;
    for (int base = 0; base < n; base += kPgJ) {
        const int j = base + threadIdx.x;
        __syncthreads();   // (first tile: the erfcx table is staged)
        if (j < n) {
            sp[threadIdx.x] = make_double4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], q[j]);
            if (HAS_V) sv[threadIdx.x] = make_double4(vel[3 * j], vel[3 * j + 1], vel[3 * j + 2], qdot[j]);
        }
        __syncthreads();
        const int t1 = min(64 * w + 64, n - base);
        if (!active) continue;
        for (int t = 64 * w; t < t1; t++) {
            const int jj = base + t;
            if (jj == i) continue;
            const double4 pj = sp[t];
            const double3 d = delta_r(make_double3(pj.x, pj.y, pj.z), xi, L, 1, T);   // x_i - x_j
            const double r2 = d.x * d.x + d.y * d.y + d.z * d.z;
            // p = phi r, dp = -phi' r^2: the pair adds ke (p / r) to g and ke / r (p qdot_j - dp q_j s / r^2) to h,
            // s = d . (v_i - v_j)
            double p, dp, inv_r;
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) {
                const double r = sqrt(r2);
                inv_r = 1.0 / r;
                const double ar = alpha * r;
                p = -erf(ar);
                dp = p + ar * exp(-ar * ar) * two_over_sqrtpi;
            } else {
                if (!(r2 <= rc2)) continue;
                inv_r = rsqrt_fp64(r2);
                const double ar = alpha * (r2 * inv_r);
                double e2;
                p = erfc_exp(ar, tab, erfc_scale, e2);
                dp = p + ar * e2 * two_over_sqrtpi;
            }
            const double kr = ke * inv_r;
            g += kr * pj.w * p;
            if (HAS_V) {
                const double4 vj = sv[t];
                const double s = d.x * (vi.x - vj.x) + d.y * (vi.y - vj.y) + d.z * (vi.z - vj.z);
                hs += kr * (p * vj.w - dp * pj.w * s * inv_r * inv_r);
            }
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = g;
        if (HAS_V) red[w - 1][1][lane] = hs;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    const double cself = ke * alpha / sqrt(kPi);   // RCK:507-510
    g = (g + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
    g_all[c * (size_t)n + i] = -2 * cself * qi + g;
    if (HAS_V) {
        hs = (hs + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
        h_all[c * (size_t)n + i] = -2 * cself * qdi + hs;
    }
}

// ---------------------------------------------------------------------------------
// 7. reciprocal part, k_bp_recip's shape: 64 atoms per block, one per lane, in each of the four
//    waves; the k-vectors pass through LDS in tiles of 256 (the coefficients 2 c_k S and, with a
//    force cotangent, 2 c_k Sdot, and the integer triple) and wave w takes entries
//    [64 w, 64 w + 64) of every tile; phases from the entry-major table.  Per k, with A = 2 c_k S,
//    B = 2 c_k Sdot, e = e_i:   g += Re[conj(e) A] = A.x e.x + A.y e.y
//                                h += Re[conj(e) B] + kappa_i Im[conj(e) A],  Im[conj(e) A] = A.y e.x - A.x e.y
//    The partial sums are added as (w0 + w1) + (w2 + w3) and then to the pair kernel's parts (this
//    lane's own atom).  Epilogue: g_i and a_i = e_bar g_i + q_bar_i - h_i to the workspace, a_i
//    also to grad[c][i].
// ---------------------------------------------------------------------------------
template <bool HAS_V>
__global__ void __launch_bounds__(256) k_bpg_recip(int n, long np, int KX, int KY, int KZ, long khalf,
                                                   const double* __restrict__ boxes, const double* __restrict__ v_all,
                                                   const double2* __restrict__ tab_t_all,
                                                   const double2* __restrict__ coef_all,
                                                   const double2* __restrict__ coefd_all,
                                                   const double* __restrict__ e_bar, const double* __restrict__ q_bar_all,
                                                   double* __restrict__ g_all, double* __restrict__ a_all,
                                                   double* __restrict__ grad_all) {
    __shared__ double2 sc[256];
    __shared__ double2 sd[HAS_V ? 256 : 1];
    __shared__ int4 sn[256];
    __shared__ double red[3][2][64];
    const size_t c = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const bool active = i < n;
    const int KS = KX + KY + KZ;
    const double2* row = tab_t_all + c * (size_t)n * KS + (active ? i : 0);   // entry m at row[m * n]
    const double2* coef = coef_all + c * (size_t)khalf;
    const double2* coefd = HAS_V ? coefd_all + c * (size_t)khalf : nullptr;
    double wx = 0, wy = 0, wz = 0;   // kappa_i = nx wx + ny wy + nz wz
    if (HAS_V && active) {
        double3 L, T;
        load_box(boxes, c, L, T);
        const double* vi = v_all + c * 3 * (size_t)n + 3 * (size_t)i;
        wx = vi[0] * (2.0 * kPi / L.x); wy = vi[1] * (2.0 * kPi / L.y); wz = vi[2] * (2.0 * kPi / L.z);
    }
    double t0 = 0, hk = 0;
    for (long base = 0; base < khalf; base += 256) {
        const long k = base + threadIdx.x;
        __syncthreads();
        if (k < khalf) {
            int nx, ny, nz;
            half_space_k(k, KY, KZ, nx, ny, nz);
            sc[threadIdx.x] = coef[k];
            if (HAS_V) sd[threadIdx.x] = coefd[k];
            sn[threadIdx.x] = make_int4(nx, ny, nz, 0);
        }
        __syncthreads();
        const int t1 = (int)min((long)(64 * w + 64), khalf - base);
        if (!active) continue;
        for (int t = 64 * w; t < t1; t++) {
            const double2 ab = sc[t];
            const int4 nn = sn[t];
            const double2 e = phase(row, (size_t)n, KX, KY, nn.x, nn.y, nn.z);
            t0 += ab.x * e.x + ab.y * e.y;
            if (HAS_V) {
                const double2 cd = sd[t];
                const double kap = nn.x * wx + nn.y * wy + nn.z * wz;
                hk += (cd.x * e.x + cd.y * e.y) + kap * (ab.y * e.x - ab.x * e.y);
            }
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = t0;
        if (HAS_V) red[w - 1][1][lane] = hk;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    t0 = (t0 + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
    const size_t at = c * (size_t)n + i;
    const double g = g_all[at] + t0;
    double a = (e_bar ? e_bar[c] : 0.0) * g + (q_bar_all ? q_bar_all[at] : 0.0);
    if (HAS_V) {
        hk = (hk + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
        a -= a_all[at] + hk;   // the pair kernel left its part of h here
    }
    g_all[at] = g;
    a_all[at] = a;
    grad_all[c * (size_t)np + i] = a;
}

// ---------------------------------------------------------------------------------
// 8. term gradients: k_bg_terms with the conformation's box (term_geometry_pbc).  One lane per
//    flattened (conformation, term), its 2 or 5 gradients into grad[c][N + ...] in the order of the
//    cf_params arrays: bonds (k, b), angles (k, theta0), waters (k1, k2, kub, b0, ub0).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpg_terms(int nconf, int n, int nterms, int nb, int na, long np,
                                                   const int4* __restrict__ tidx, const double* __restrict__ tpar,
                                                   const double* __restrict__ pos_all, const double* __restrict__ boxes,
                                                   const double* __restrict__ v_all, const double* __restrict__ g_all,
                                                   const double* __restrict__ a_all, double* __restrict__ grad_all) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long)nconf * nterms) return;
    const size_t c = (size_t)(gi / nterms);
    const int t = (int)(gi % nterms);
    const int4 ti = tidx[t];
    const double* p = tpar + 5 * t;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* vel = v_all ? v_all + c * 3 * (size_t)n : nullptr;
    const double* gw = g_all + c * (size_t)n;
    const double* aw = a_all + c * (size_t)n;
    double* out = grad_all + c * (size_t)np + n;
    double3 L, T;
    load_box(boxes, c, L, T);
    double x[3], xd[3];
    term_geometry_pbc(ti, pos, vel, L, T, x, xd);
    if (ti.x == 0) {
        const double da = aw[ti.y] - aw[ti.z], dg = gw[ti.y] - gw[ti.z];
        out += 2 * t;
        out[0] = da * (x[0] - p[1]) - dg * xd[0];
        out[1] = -p[0] * da;
    } else if (ti.x == 1) {
        const double wa = aw[ti.y] - 2 * aw[ti.z] + aw[ti.w], wg = gw[ti.y] - 2 * gw[ti.z] + gw[ti.w];
        out += 2 * nb + 2 * (t - nb);
        out[0] = wa * (x[0] - p[1]) - wg * xd[0];
        out[1] = -p[0] * wa;
    } else {
        const double a2 = aw[ti.z] - aw[ti.y], a3 = aw[ti.w] - aw[ti.y];
        const double g2 = gw[ti.z] - gw[ti.y], g3 = gw[ti.w] - gw[ti.y];
        const double b0 = p[3], ub0 = p[4];
        out += 2 * nb + 2 * na + 5 * (t - nb - na);
        out[0] = a2 * (x[0] - b0) + a3 * (x[1] - b0) - g2 * xd[0] - g3 * xd[1];
        out[1] = a2 * (x[1] - b0) + a3 * (x[0] - b0) - g2 * xd[1] - g3 * xd[0];
        out[2] = (a2 + a3) * (x[2] - ub0) - (g2 + g3) * xd[2];
        out[3] = -(p[0] + p[1]) * (a2 + a3);
        out[4] = -p[2] * (a2 + a3);
    }
}

// ---------------------------------------------------------------------------------
// launcher: one pass of nconf <= min(w.cap, gw.cap) conformations, at most eight launches
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

size_t batch_pbc_grad_doubles_per_conf(const Handle& h) {
    return 2 * (size_t)h.khalf + 3 * (size_t)h.n;   // coefd [khalf] x 2, qdot[N], g[N], a[N]
}

void batch_pbc_grad_carve(const Handle& h, double* base, int cap, BatchPbcGradWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n;
    w.base = base; w.cap = cap;
    w.coefd = reinterpret_cast<double2*>(base);
    w.qdot = reinterpret_cast<double*>(w.coefd + c * (size_t)h.khalf);
    w.g = w.qdot + c * n;
    w.a = w.g + c * n;
}

void launch_batch_pbc_vjp(Handle& h, const BatchPbcWs& w, const BatchPbcGradWs& gw, int nconf, const double* pos,
                          const double* boxes, const double* e_bar, const double* q_bar, const double* f_bar,
                          double* grad) {
    if (nconf <= 0 || nconf > w.cap || nconf > gw.cap || nconf > kBatchMaxPass)
        throw std::invalid_argument("launch_batch_pbc_vjp: pass size");
    const int n = h.n;
    const int KX = h.kmax[0], KY = h.kmax[1], KZ = h.kmax[2];
    const long khalf = (long)h.khalf;
    const long np = (long)n + 2L * h.nb + 2L * h.na + 5L * h.nw;
    const double one_a2 = 1.0 / (h.alpha * h.alpha), rc2 = h.cutoff * h.cutoff;
    launch_batch_pbc_flux_charges(h, w, nconf, pos, boxes, nullptr);
    if (f_bar)
        hipLaunchKernelGGL(k_bpg_tangent, dim3(nblk(n, 256), nconf), dim3(256), 0, h.stream, n, h.nb, h.na, h.term_idx,
                           h.term_par, h.qcsr_start, h.qcsr_slot, pos, boxes, f_bar, gw.qdot);
    launch_batch_pbc_tables(h, w, nconf, pos, boxes);
    const dim3 kgrid(nblk(khalf, 256), nconf), agrid(nblk(n, 64), nconf);
    if (f_bar) {
        hipLaunchKernelGGL(k_bpg_sfac<true>, kgrid, dim3(256), 0, h.stream, n, KX, KY, KZ, khalf, h.ke, one_a2, boxes,
                           w.q, f_bar, gw.qdot, w.tab, w.coef, gw.coefd);
        hipLaunchKernelGGL(k_bpg_pairs<true>, agrid, dim3(kPgJ), 0, h.stream, n, h.ke, h.alpha, rc2, h.erfc_scale,
                           h.erfc_tab, boxes, pos, w.q, f_bar, gw.qdot, h.ex_start, h.ex_list, gw.g, gw.a);
        hipLaunchKernelGGL(k_bpg_recip<true>, agrid, dim3(256), 0, h.stream, n, np, KX, KY, KZ, khalf, boxes, f_bar,
                           w.tab_t, w.coef, gw.coefd, e_bar, q_bar, gw.g, gw.a, grad);
    } else {
        hipLaunchKernelGGL(k_bpg_sfac<false>, kgrid, dim3(256), 0, h.stream, n, KX, KY, KZ, khalf, h.ke, one_a2, boxes,
                           w.q, nullptr, nullptr, w.tab, w.coef, nullptr);
        hipLaunchKernelGGL(k_bpg_pairs<false>, agrid, dim3(kPgJ), 0, h.stream, n, h.ke, h.alpha, rc2, h.erfc_scale,
                           h.erfc_tab, boxes, pos, w.q, nullptr, nullptr, h.ex_start, h.ex_list, gw.g, gw.a);
        hipLaunchKernelGGL(k_bpg_recip<false>, agrid, dim3(256), 0, h.stream, n, np, KX, KY, KZ, khalf, boxes, nullptr,
                           w.tab_t, w.coef, nullptr, e_bar, q_bar, gw.g, gw.a, grad);
    }
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bpg_terms, dim3(nblk((int64_t)nconf * h.nterms, 256)), dim3(256), 0, h.stream, nconf, n,
                           h.nterms, h.nb, h.na, np, h.term_idx, h.term_par, pos, boxes, f_bar, gw.g, gw.a, grad);
}

}  // namespace cf
