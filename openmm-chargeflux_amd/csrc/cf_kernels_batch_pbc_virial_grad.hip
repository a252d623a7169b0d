// cf_kernels_batch_pbc_virial_grad.hip -- cf_compute_batch_periodic_virial_vjp: the reverse-mode
// product of the virial tensors of the periodic batch (cf_kernels_batch_pbc_virial.hip) with respect
// to the base charges, the flux parameters and the LJ sigma / epsilon ("batched,
// periodic, virial parameter gradients").  Per conformation and ORTHORHOMBIC box, with cotangent
// W_bar (3 x 3), the scalar is L = W_bar : Xi, Xi = -dE/d eps.  Xi is symmetric, so only
// T = (W_bar + W_bar^T) / 2 enters, and L = -D_T E: the directional derivative along the strain
// x -> x (I + t T), h -> h (I + t T) at fixed pair set and images.  Under that strain
//   - a minimum-image vector d (a pair's, or one of a flux term's) has the tangent d T: the image
//     shift strains too, so the tangent is not a difference of atom tangents, and
//     rdot_ij = (d_ij T d_ij) / r;
//   - the phases k . x are invariant;
//   - c_k = (4 pi ke / V) exp(-k^2 / 4 alpha^2) / k^2 changes through V and k^2 (d k^2 = -2 k T k):
//     cdot_k = c_k [-tr T + 2 (k T k) (1 / k^2 + 1 / (4 alpha^2))].
// With qdot = D_T q, S = sum q_j e_j, Sq = sum qdot_j e_j, c_s = ke alpha / sqrt(pi):
//     g_i = dE/dq_i = ke sum_j phi_ij q_j - 2 c_s q_i + sum_k Re[conj(e_i) 2 c_k S(k)]
//     h_i = D_T g_i = ke sum_j (phi_ij qdot_j + phi'_ij rdot_ij q_j) - 2 c_s qdot_i
//                     + sum_k Re[conj(e_i) (2 c_k Sq(k) + 2 cdot_k S(k))]
//     dL/d(base charge i) = a_i = -h_i
//     flux term (k, ref), pieces q_a += c_a k (x - ref):   dL/dk   = sum_a c_a [a_a (x - ref) - g_a xd]
//                                                          dL/dref = -k sum_a c_a a_a
// phi and phi' as in cf_kernels_batch_pbc_grad.hip (erfc pair within the cutoff, -erf for an excluded
// pair at any distance); xd the tangent of the term's geometry from the d T tangents.  Only the LJ
// pair term depends on sigma and epsilon: L_LJ = -sum_pairs U'_ij rdot_ij, the sums of
// cf_kernels_batch_lj_grad.hip with e_bar = 0 and rdot_ij / r = d T d / r^2 (an atom with eps = 0: 0).
// A pass is k_bp_flux, k_b_charges, k_bp_tables (as they are), then k_bpvg_strain, k_bpvg_tangent,
// k_bpvg_sfac, k_bpvg_pairs, k_bpvg_recip, k_bpvg_terms: at most nine launches whatever nconf
// (the LJ gradients alone: k_bpvg_strain and k_bpvg_pairs).
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N, the topology and kmax: a
// conformation's rows are bitwise the same alone, in any batch, under any chunking and with or
// without the LJ output (the Coulomb and LJ sums of the pair kernel are explicit fma chains, the same
// in every instantiation).
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms, khalf and the launch's own nconf: no device guard bits.
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

// the symmetric strain direction of one conformation, (xx, xy, xz, yy, yz, zz)
struct Strain {
    double xx, xy, xz, yy, yz, zz;
};

__device__ __forceinline__ Strain load_strain(const double* __restrict__ t6, size_t c) {
    const double* t = t6 + 6 * c;
    return Strain{t[0], t[1], t[2], t[3], t[4], t[5]};
}

// d T d by six fmas (three products): dx (Txx dx + 2 Txy dy + 2 Txz dz) + dy (Tyy dy + 2 Tyz dz) + dz Tzz dz
__device__ __forceinline__ double strain_quad(const Strain& T, double dx, double dy, double dz) {
    const double a = fma(2 * T.xz, dz, fma(2 * T.xy, dy, T.xx * dx));
    const double b = fma(2 * T.yz, dz, T.yy * dy);
    return fma(dz, T.zz * dz, fma(dy, b, dx * a));
}
__device__ __forceinline__ double strain_quad(const Strain& T, double3 d) { return strain_quad(T, d.x, d.y, d.z); }

__device__ __forceinline__ double dot3s(double3 a, double3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// ---------------------------------------------------------------------------------
// 0. T = (W_bar + W_bar^T) / 2 of every conformation, once: six doubles.  An antisymmetric W_bar
//    gives exact zeros, W_bar and its transpose the same bits.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpvg_strain(int nconf, const double* __restrict__ vbar,
                                                     double* __restrict__ t6) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nconf) return;
    const double* w = vbar + 9 * (size_t)c;
    double* t = t6 + 6 * (size_t)c;
    t[0] = w[0];
    t[1] = 0.5 * (w[1] + w[3]);
    t[2] = 0.5 * (w[2] + w[6]);
    t[3] = w[4];
    t[4] = 0.5 * (w[5] + w[7]);
    t[5] = w[8];
}

// ---------------------------------------------------------------------------------
// term geometry and its tangent along the strain: term_geometry_pbc of cf_kernels_batch_pbc_grad.hip
// with the tangent of every minimum-image vector d equal to d T, so the tangent of |d| is
// (d T d) / |d|.  x[] holds the value each parameter group multiplies, xd[] its tangent (bond r;
// angle theta; water r12, r13, r23).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void term_geometry_strain(int4 ti, const double* __restrict__ pos, double3 L, double3 B,
                                                     const Strain& T, double x[3], double xd[3]) {
    x[0] = x[1] = x[2] = 0.0;
    xd[0] = xd[1] = xd[2] = 0.0;
    if (ti.x == 0) {  // bond p1-p2
        const double3 d = delta_r(ld3(pos, ti.y), ld3(pos, ti.z), L, 1, B);
        const double r = sqrt(dot3s(d, d));
        x[0] = r;
        xd[0] = strain_quad(T, d) / r;
    } else if (ti.x == 1) {  // angle p1-p2-p3, p2 central
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double3 d21 = delta_r(x2, x1, L, 1, B), d23 = delta_r(x2, x3, L, 1, B), d13 = delta_r(x1, x3, L, 1, B);
        const double r21_2 = dot3s(d21, d21), r23_2 = dot3s(d23, d23), r13_2 = dot3s(d13, d13);
        const double r21 = sqrt(r21_2), r23 = sqrt(r23_2);
        const double cost = (r23_2 + r21_2 - r13_2) / 2 / r21 / r23;
        x[0] = acos(cost);
        // s = d T d = r rdot of each vector; c = u / (2 r21 r23), u = r23^2 + r21^2 - r13^2:
        // cdot = udot / (2 r21 r23) - c (r21dot / r21 + r23dot / r23)
        const double s21 = strain_quad(T, d21), s23 = strain_quad(T, d23), s13 = strain_quad(T, d13);
        const double cdot = (s23 + s21 - s13) / r21 / r23 - cost * (s21 / r21_2 + s23 / r23_2);
        xd[0] = -cdot / sqrt(1 - cost * cost);
    } else {  // water O,H1,H2
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double3 d12 = delta_r(x1, x2, L, 1, B), d13 = delta_r(x1, x3, L, 1, B), d23 = delta_r(x2, x3, L, 1, B);
        const double r12 = sqrt(dot3s(d12, d12)), r13 = sqrt(dot3s(d13, d13)), r23 = sqrt(dot3s(d23, d23));
        x[0] = r12; x[1] = r13; x[2] = r23;
        xd[0] = strain_quad(T, d12) / r12;
        xd[1] = strain_quad(T, d13) / r13;
        xd[2] = strain_quad(T, d23) / r23;
    }
}

// ---------------------------------------------------------------------------------
// 1. strain charge tangents: one lane per (conformation, atom), qdot_i = D_T q_i summed over the
//    atom's charge slots in qcsr slot order (k_bpg_tangent's walk, the term tangents from d T).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpvg_tangent(int n, int nb, int na, const int4* __restrict__ tidx,
                                                      const double* __restrict__ tpar, const int* __restrict__ qs,
                                                      const int* __restrict__ qslot, const double* __restrict__ pos_all,
                                                      const double* __restrict__ boxes, const double* __restrict__ t6,
                                                      double* __restrict__ qdot_all) {
    const size_t c = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* pos = pos_all + c * 3 * (size_t)n;
    double3 L, B;
    load_box(boxes, c, L, B);
    const Strain T = load_strain(t6, c);
    double qd = 0;
    for (int k = qs[i]; k < qs[i + 1]; k++) {
        const int s = qslot[k];
        int t, role;
        if (s < 2 * nb) { t = s >> 1; role = s & 1; }
        else { const int u = s - 2 * nb; t = nb + u / 3; role = u % 3; }   // angles then waters: 3 slots each
        const int4 ti = tidx[t];
        const double* p = tpar + 5 * t;
        double x[3], xd[3];
        term_geometry_strain(ti, pos, L, B, T, x, xd);
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
// 2. structure factors: one lane per (conformation, k), the atoms in atom order; S = sum q_j e_j and
//    Sq = sum qdot_j e_j in one sweep over the atom-major phase table.  Output per k:
//    coef = 2 c_k S and coefd = 2 c_k Sq + 2 cdot_k S = 2 c_k (Sq + br S),
//    br = -tr T + 2 (k T k) (1 / k^2 + 1 / (4 alpha^2)): the strain of c_k is folded in here, so the
//    per-(atom, k) kernel reads two coefficients and no third.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpvg_sfac(int n, int KX, int KY, int KZ, long khalf, double ke, double one_a2,
                                                   const double* __restrict__ boxes, const double* __restrict__ t6,
                                                   const double* __restrict__ q_all, const double* __restrict__ qdot_all,
                                                   const double2* __restrict__ tab_all, double2* __restrict__ coef_all,
                                                   double2* __restrict__ coefd_all) {
    const size_t c = blockIdx.y;
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= khalf) return;
    int nx, ny, nz;
    half_space_k(k, KY, KZ, nx, ny, nz);
    double3 L, B;
    load_box(boxes, c, L, B);
    const Strain T = load_strain(t6, c);
    const double kx = nx * (2.0 * kPi / L.x), ky = ny * (2.0 * kPi / L.y), kz = nz * (2.0 * kPi / L.z);
    const int KS = KX + KY + KZ;
    const double2* row = tab_all + c * (size_t)n * KS;
    const double* q = q_all + c * (size_t)n;
    const double* qdot = qdot_all + c * (size_t)n;
    double cs = 0, ss = 0, cd = 0, sd = 0;
    for (int i = 0; i < n; i++) {
        const double2 e = phase(row + (size_t)i * KS, 1, KX, KY, nx, ny, nz);
        const double qi = q[i], qd = qdot[i];
        cs += qi * e.x;
        ss += qi * e.y;
        cd += qd * e.x;
        sd += qd * e.y;
    }
    const double k2 = kx * kx + ky * ky + kz * kz;
    const double eak = exp(-k2 * 0.25 * one_a2) / k2;
    const double cst = 4.0 / L.x / L.y / L.z * kPi * ke;   // RCK:517
    const double ck2 = 2.0 * cst * eak;
    const double br = 2.0 * strain_quad(T, kx, ky, kz) * (1.0 / k2 + 0.25 * one_a2) - (T.xx + T.yy + T.zz);
    coef_all[c * (size_t)khalf + k] = make_double2(ck2 * cs, ck2 * ss);
    coefd_all[c * (size_t)khalf + k] = make_double2(ck2 * (cd + br * cs), ck2 * (sd + br * ss));
}

// ---------------------------------------------------------------------------------
// 3. direct space.  A block is kVgI = 64 i-atoms of one conformation, one per lane, in each of its
//    four waves; the j-atoms pass through LDS in tiles of 256 -- (x, y, z, q), qdot and, with the LJ
//    gradients, (sigma_j / 2, 2 sqrt eps_j) -- and wave w takes entries [64 w, 64 w + 64) of every
//    tile.  Per pair, formed once and kept in registers: the minimum image d (delta_r with the
//    conformation's box), r^2, the exclusion and cutoff rule of k_bp_pairs (an excluded partner takes
//    the erf pair of (phi, phi') at any distance and no LJ, any other partner within the cutoff the
//    erfc pair from the handle's erfcx table in LDS), and u = d T d.  Accumulators per lane: the pair
//    parts of g_i and h_i and, with LJ, the two sums of k_blj_pairs with rdot / r = u / r^2.
//    MODE 0: Coulomb only; 1: Coulomb and LJ; 2: LJ only (no charges, no table).  The mode is an
//    instantiation, not a branch in the j loop, and the Coulomb and LJ sums are explicit fma chains:
//    g and h carry the same bits in modes 0 and 1, the LJ rows in modes 1 and 2.
//    The four waves' partial sums are added as (w0 + w1) + (w2 + w3) through LDS.  g and h go to
//    the workspace without the self terms (k_bpvg_recip adds them); the LJ rows are final:
//    lj_grad[c][i] = g_sigma / 2, lj_grad[c][N + i] = 2 T' / lj_i.y, exactly 0 for eps_i = 0.
//    LDS, mode 1: table 8256 B + (x, q) tile 8192 B + qdot tile 2048 B + LJ tile 4096 B + partial
//    sums 3 x 4 x 512 B = 28 736 B; mode 0: 21 568 B.
// ---------------------------------------------------------------------------------
constexpr int kVgI = 64;
constexpr int kVgJ = 256;

template <int MODE>
__global__ void __launch_bounds__(kVgJ) k_bpvg_pairs(int n, double ke, double alpha, double rc2, double erfc_scale,
                                                     const double* __restrict__ erfc_tab,
                                                     const double* __restrict__ boxes, const double* __restrict__ t6,
                                                     const double* __restrict__ pos_all, const double* __restrict__ q_all,
                                                     const double* __restrict__ qdot_all,
                                                     const double2* __restrict__ lj, const int* __restrict__ ex_start,
                                                     const int* __restrict__ ex_list, double* __restrict__ g_all,
                                                     double* __restrict__ h_all, double* __restrict__ lj_grad_all) {
    constexpr bool COUL = MODE != 2, LJ = MODE != 0;
    constexpr int NACC = (COUL ? 2 : 0) + (LJ ? 2 : 0), LJ0 = COUL ? 2 : 0;
    __shared__ double tab[COUL ? kErfcMaxM * (kErfcDeg + 1) : 1];
    __shared__ double4 sp[kVgJ];
    __shared__ double sq[COUL ? kVgJ : 1];
    __shared__ double2 sl[LJ ? kVgJ : 1];
    __shared__ double red[3][NACC][kVgI];   // partial sums of waves 1..3
    if (COUL)
        for (int e = threadIdx.x; e < kErfcMaxM * (kErfcDeg + 1); e += kVgJ) tab[e] = erfc_tab[e];
    const size_t c = blockIdx.y;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = COUL ? q_all + c * (size_t)n : nullptr;
    const double* qdot = COUL ? qdot_all + c * (size_t)n : nullptr;
    double3 L, B;
    load_box(boxes, c, L, B);
    const Strain T = load_strain(t6, c);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kVgI + lane;
    const bool active = i < n;
    double3 xi = make_double3(0, 0, 0);
    double2 li = make_double2(0, 0);
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        xi = ld3(pos, i);
        if (LJ) li = lj[i];
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int k = 0; k < kMaxRegExcl; k++) reg[k] = k < exc ? ex_list[ex0 + k] : -1;
    const bool ljwork = LJ && active && li.y != 0.0;   // eps_i = 0: no LJ interaction, both gradients exactly 0
    const bool work = COUL ? active : ljwork;
    const double two_over_sqrtpi = 1.1283791670955126;
    double g = 0, hs = 0, gs = 0, tp = 0;
    for (int base = 0; base < n; base += kVgJ) {
        const int j = base + threadIdx.x;
        __syncthreads();   // (first tile: the erfcx table is staged)
        if (j < n) {
            sp[threadIdx.x] = make_double4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], COUL ? q[j] : 0.0);
            if (COUL) sq[threadIdx.x] = qdot[j];
            if (LJ) sl[threadIdx.x] = lj[j];
        }
        __syncthreads();
        const int t1 = min(64 * w + 64, n - base);
        if (!work) continue;
        for (int t = 64 * w; t < t1; t++) {
            const int jj = base + t;
            if (jj == i) continue;
            if (!COUL && sl[t].y == 0.0) continue;   // wave-uniform: no LJ on this partner
            const double4 pj = sp[t];
            const double3 d = delta_r(make_double3(pj.x, pj.y, pj.z), xi, L, 1, B);   // x_i - x_j
            const double r2 = fma(d.z, d.z, fma(d.x, d.x, d.y * d.y));
            // p = phi r, dp = -phi' r^2: the pair adds ke (p / r) q_j to g and
            // ke / r (p qdot_j - dp q_j u / r^2) to h, u = d T d = r rdot
            double p, dp, inv_r;
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) {
                if (!COUL) continue;
                const double r = sqrt(r2);
                inv_r = 1.0 / r;
                const double ar = alpha * r;
                p = -erf(ar);
                dp = fma(ar * exp(-ar * ar), two_over_sqrtpi, p);
                const double u = strain_quad(T, d);
                const double kr = ke * inv_r, kq = kr * pj.w;
                g = fma(kq, p, g);
                hs = fma(kr * sq[t], p, hs);
                hs = fma(-kq, dp * (u * (inv_r * inv_r)), hs);
                continue;
            }
            if (!(r2 <= rc2)) continue;
            const double u = strain_quad(T, d);
            if (COUL) {
                inv_r = rsqrt_fp64(r2);
                const double ar = alpha * (r2 * inv_r);
                double e2;
                p = erfc_exp(ar, tab, erfc_scale, e2);
                dp = fma(ar * e2, two_over_sqrtpi, p);
                const double kr = ke * inv_r, kq = kr * pj.w;
                g = fma(kq, p, g);
                hs = fma(kr * sq[t], p, hs);
                hs = fma(-kq, dp * (u * (inv_r * inv_r)), hs);
            }
            if (LJ) {
                const double2 l = sl[t];
                if (!ljwork || l.y == 0.0) continue;
                const double ir2 = 1.0 / r2;
                const double A = li.x + l.x;
                const double A2 = A * A, ir6 = ir2 * ir2 * ir2;
                const double a5r6 = A2 * A2 * A * ir6;   // A^5 / r^6
                const double s6 = a5r6 * A;
                const double rr = u * ir2;               // rdot / r
                // explicit fmas, as the Coulomb sums: the same bits in modes 1 and 2
                gs = fma(li.y * l.y * a5r6, fma(144.0, s6, -36.0) * rr, gs);
                tp = fma(l.y, s6 * fma(12.0, s6, -6.0) * rr, tp);
            }
        }
    }
    if (w > 0) {
        if (COUL) { red[w - 1][0][lane] = g; red[w - 1][1][lane] = hs; }
        if (LJ) { red[w - 1][LJ0][lane] = gs; red[w - 1][LJ0 + 1][lane] = tp; }
    }
    __syncthreads();
    if (w > 0 || !active) return;
    auto tot = [&](double a, int m) { return (a + red[0][m][lane]) + (red[1][m][lane] + red[2][m][lane]); };
    if (COUL) {
        g_all[c * (size_t)n + i] = tot(g, 0);
        h_all[c * (size_t)n + i] = tot(hs, 1);
    }
    if (LJ) {
        gs = tot(gs, LJ0);
        tp = tot(tp, LJ0 + 1);
        double* out = lj_grad_all + c * 2 * (size_t)n;
        out[i] = ljwork ? 0.5 * gs : 0.0;
        out[(size_t)n + i] = ljwork ? 2.0 * tp / li.y : 0.0;
    }
}

// ---------------------------------------------------------------------------------
// 4. reciprocal part, k_bp_recip's shape: 64 atoms per block, one per lane, in each of the four
//    waves; the k-vectors pass through LDS in tiles of 256 (coef, coefd and the integer triple) and
//    wave w takes entries [64 w, 64 w + 64) of every tile; phases from the entry-major table.  Per k,
//    with e = e_i:  g += Re[conj(e) coef],  h += Re[conj(e) coefd]   (k . x is invariant: no kappa
//    term).  The partial sums are added as (w0 + w1) + (w2 + w3), then to the pair kernel's parts and
//    the self terms -2 c_s q_i and -2 c_s qdot_i.  Epilogue: g_i and a_i = -h_i to the workspace, a_i
//    also to grad[c][i].
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpvg_recip(int n, long np, int KX, int KY, int KZ, long khalf, double cself,
                                                    const double2* __restrict__ tab_t_all,
                                                    const double2* __restrict__ coef_all,
                                                    const double2* __restrict__ coefd_all,
                                                    const double* __restrict__ q_all, const double* __restrict__ qdot_all,
                                                    double* __restrict__ g_all, double* __restrict__ a_all,
                                                    double* __restrict__ grad_all) {
    __shared__ double2 sc[256];
    __shared__ double2 sd[256];
    __shared__ int4 sn[256];
    __shared__ double red[3][2][64];
    const size_t c = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const bool active = i < n;
    const int KS = KX + KY + KZ;
    const double2* row = tab_t_all + c * (size_t)n * KS + (active ? i : 0);   // entry m at row[m * n]
    const double2* coef = coef_all + c * (size_t)khalf;
    const double2* coefd = coefd_all + c * (size_t)khalf;
    double gk = 0, hk = 0;
    for (long base = 0; base < khalf; base += 256) {
        const long k = base + threadIdx.x;
        __syncthreads();
        if (k < khalf) {
            int nx, ny, nz;
            half_space_k(k, KY, KZ, nx, ny, nz);
            sc[threadIdx.x] = coef[k];
            sd[threadIdx.x] = coefd[k];
            sn[threadIdx.x] = make_int4(nx, ny, nz, 0);
        }
        __syncthreads();
        const int t1 = (int)min((long)(64 * w + 64), khalf - base);
        if (!active) continue;
        for (int t = 64 * w; t < t1; t++) {
            const double2 ab = sc[t], cd = sd[t];
            const int4 nn = sn[t];
            const double2 e = phase(row, (size_t)n, KX, KY, nn.x, nn.y, nn.z);
            gk += ab.x * e.x + ab.y * e.y;
            hk += cd.x * e.x + cd.y * e.y;
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = gk;
        red[w - 1][1][lane] = hk;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    gk = (gk + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
    hk = (hk + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
    const size_t at = c * (size_t)n + i;
    const double g = (-2 * cself * q_all[at] + g_all[at]) + gk;
    const double a = -((-2 * cself * qdot_all[at] + a_all[at]) + hk);   // the pair kernel left its part of h here
    g_all[at] = g;
    a_all[at] = a;
    grad_all[c * (size_t)np + i] = a;
}

// ---------------------------------------------------------------------------------
// 5. term gradients: one lane per flattened (conformation, term), its 2 or 5 gradients into
//    grad[c][N + ...] in the order of the cf_params arrays: bonds (k, b), angles (k, theta0), waters
//    (k1, k2, kub, b0, ub0); k_bpg_terms' expressions in a = -h and g, the geometry tangent xd from
//    the strain.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpvg_terms(int nconf, int n, int nterms, int nb, int na, long np,
                                                    const int4* __restrict__ tidx, const double* __restrict__ tpar,
                                                    const double* __restrict__ pos_all, const double* __restrict__ boxes,
                                                    const double* __restrict__ t6, const double* __restrict__ g_all,
                                                    const double* __restrict__ a_all, double* __restrict__ grad_all) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long)nconf * nterms) return;
    const size_t c = (size_t)(gi / nterms);
    const int t = (int)(gi % nterms);
    const int4 ti = tidx[t];
    const double* p = tpar + 5 * t;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* gw = g_all + c * (size_t)n;
    const double* aw = a_all + c * (size_t)n;
    double* out = grad_all + c * (size_t)np + n;
    double3 L, B;
    load_box(boxes, c, L, B);
    const Strain T = load_strain(t6, c);
    double x[3], xd[3];
    term_geometry_strain(ti, pos, L, B, T, x, xd);
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
// launcher: one pass of nconf <= min(w.cap, vw.cap) conformations, at most nine launches
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

size_t batch_pbc_virial_grad_doubles_per_conf(const Handle& h) {
    return 2 * (size_t)h.khalf + 3 * (size_t)h.n + 6;   // coefd [khalf] x 2, qdot[N], g[N], a[N], T[6]
}

void batch_pbc_virial_grad_carve(const Handle& h, double* base, int cap, BatchPbcVirialGradWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n;
    w.base = base; w.cap = cap;
    w.coefd = reinterpret_cast<double2*>(base);
    w.qdot = reinterpret_cast<double*>(w.coefd + c * (size_t)h.khalf);
    w.g = w.qdot + c * n;
    w.a = w.g + c * n;
    w.t6 = w.a + c * n;
}

void launch_batch_pbc_virial_vjp(Handle& h, const BatchPbcWs& w, const BatchPbcVirialGradWs& vw, int nconf,
                                 const double* pos, const double* boxes, const double* virial_bar, double* grad,
                                 double* lj_grad) {
    if (nconf <= 0 || nconf > w.cap || nconf > vw.cap || nconf > kBatchMaxPass)
        throw std::invalid_argument("launch_batch_pbc_virial_vjp: pass size");
    if (!virial_bar || (!grad && !lj_grad)) throw std::invalid_argument("launch_batch_pbc_virial_vjp: nothing to do");
    const int n = h.n;
    const int KX = h.kmax[0], KY = h.kmax[1], KZ = h.kmax[2];
    const long khalf = (long)h.khalf;
    const long np = (long)n + 2L * h.nb + 2L * h.na + 5L * h.nw;
    const double one_a2 = 1.0 / (h.alpha * h.alpha), rc2 = h.cutoff * h.cutoff;
    const dim3 kgrid(nblk(khalf, 256), nconf), agrid(nblk(n, kVgI), nconf);
#define CF_VG_PAIRS(MODE)                                                                                          \
    hipLaunchKernelGGL(k_bpvg_pairs<MODE>, agrid, dim3(kVgJ), 0, h.stream, n, h.ke, h.alpha, rc2, h.erfc_scale,    \
                       h.erfc_tab, boxes, vw.t6, pos, w.q, vw.qdot, h.lj, h.ex_start, h.ex_list, vw.g, vw.a, lj_grad)
    hipLaunchKernelGGL(k_bpvg_strain, dim3(nblk(nconf, 256)), dim3(256), 0, h.stream, nconf, virial_bar, vw.t6);
    if (!grad) {   // sigma and epsilon alone: the charges do not enter
        CF_VG_PAIRS(2);
        return;
    }
    launch_batch_pbc_flux_charges(h, w, nconf, pos, boxes, nullptr);
    hipLaunchKernelGGL(k_bpvg_tangent, dim3(nblk(n, 256), nconf), dim3(256), 0, h.stream, n, h.nb, h.na, h.term_idx,
                       h.term_par, h.qcsr_start, h.qcsr_slot, pos, boxes, vw.t6, vw.qdot);
    launch_batch_pbc_tables(h, w, nconf, pos, boxes);
    hipLaunchKernelGGL(k_bpvg_sfac, kgrid, dim3(256), 0, h.stream, n, KX, KY, KZ, khalf, h.ke, one_a2, boxes, vw.t6, w.q,
                       vw.qdot, w.tab, w.coef, vw.coefd);
    if (lj_grad) CF_VG_PAIRS(1);
    else CF_VG_PAIRS(0);
#undef CF_VG_PAIRS
    hipLaunchKernelGGL(k_bpvg_recip, agrid, dim3(256), 0, h.stream, n, np, KX, KY, KZ, khalf,
                       h.ke * h.alpha / sqrt(kPi), w.tab_t, w.coef, vw.coefd, w.q, vw.qdot, vw.g, vw.a, grad);
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bpvg_terms, dim3(nblk((int64_t)nconf * h.nterms, 256)), dim3(256), 0, h.stream, nconf, n,
                           h.nterms, h.nb, h.na, np, h.term_idx, h.term_par, pos, boxes, vw.t6, vw.g, vw.a, grad);
}

}  // namespace cf
