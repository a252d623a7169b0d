// cf_kernels_batch_pbc_hvp_grad.hip -- cf_compute_batch_periodic_hvp_vjp: the reverse-mode product of
// the Hessian-vector products of the periodic batch (cf_kernels_batch_pbc_hvp.hip) with respect to the
// base charges and the flux parameters ("batched, periodic, Hessian-vector parameter
// gradients").  Per conformation x with its box, directions v_k and cotangents u_k, the scalar is
//     L = sum_k u_k . H(x; box) v_k = sum_k D_u D_v E        (fixed box, pair set and image of every pair).
// E = E_LJ + q^T M(x) q / 2 with M the pair, self and reciprocal parts, g = M q; the assembly is the
// one of cf_kernels_batch_hvp_grad.hip:
//     dL/d(base charge i) = sum_k g^uv_i
//     dL/dk   += sum_k sum_a c_a [ g^uv_a (gamma - ref) + g^u_a gamma^v + g^v_a gamma^u + g_a gamma^uv ]
//     dL/dref += -k sum_k sum_a c_a g^uv_a
// with gamma from the term's MINIMUM-IMAGE geometry on hyper-dual numbers (term_gammas_pbc).
// d = minimum image of x_i - x_j, r = |d|, w^u = u_i - u_j, c = 2 / sqrt(pi), c_s = ke alpha / sqrt(pi),
// P = erfc(alpha r) for a non-excluded pair within the cutoff and -erf(alpha r) for an excluded pair at
// any distance, Q = P + c (alpha r) e^{-alpha^2 r^2}, T = c (alpha r)^3 e^{-alpha^2 r^2}:
//     g_i    = ke sum_j q_j P / r                                                             - 2 c_s q_i
//     g^u_i  = ke sum_j [ q^u_j P / r - q_j Q (d.w^u) / r^3 ]                                 - 2 c_s q^u_i
//     g^uv_i = ke sum_j [ q^uv_j P / r - Q (q^u_j (d.w^v) + q^v_j (d.w^u) + q_j (w^u.w^v)) / r^3
//                         + q_j (3 Q + 2 T) (d.w^u)(d.w^v) / r^5 ]                            - 2 c_s q^uv_i
// plus the reciprocal part over the forward path's half-space k set (k from the box diagonals), with
// e_i = e^{i k.x_i}, kappa^u_i = k.u_i and A = 2 c_k S:
//     S^u  = sum_j (q^u_j + i q_j kappa^u_j) e_j
//     S^uv = sum_j (q^uv_j + i (q^u_j kappa^v_j + q^v_j kappa^u_j) - q_j kappa^u_j kappa^v_j) e_j
//     g_i    += sum_k Re[conj(e_i) A]
//     g^u_i  += sum_k Re[conj(e_i) (A^u - i kappa^u_i A)]
//     g^uv_i += sum_k Re[conj(e_i) (A^uv - i kappa^u_i A^v - i kappa^v_i A^u - kappa^u_i kappa^v_i A)]
// LJ does not enter and neither does dq/dx.  Nothing divides by a parameter: k = 0 is legal.
//
// What does not depend on the direction -- minimum image, the excluded and cutoff tests, the erfc
// lookup, exp, the phase products -- is done once for a CHUNK of kPhgKC direction rows of a
// conformation: blockIdx.y of k_bphg_sfac, k_bphg_pairs and k_bphg_recip is (conformation, chunk).
// A pass: k_bp_flux, k_b_charges, k_bp_tables (as they are, once per conformation), then k_bphg_geom,
// k_bhg_qtan (cf_kernels_batch_hvp_grad.hip's, as it is), k_bphg_sfac, k_bphg_pairs, k_bphg_recip,
// k_bphg_rows: at most nine launches.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N, the topology, kmax and the order of
// the directions; a row the tail chunk lacks is zeros.  A conformation's gradient row is bitwise the
// same alone, at any position of any batch, in any chunk slot and however its directions are split
// into passes.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms, khalf, kv and the launch's own counts: no device guard bits.
#include <stdexcept>

#include "cf_flux_dual.h"

namespace cf {

constexpr int kPhgKC = 4;   // direction rows per chunk

// ---------------------------------------------------------------------------------
// 1. geometry tangents: k_bhg_geom with the conformation's box.  One lane per flattened (row, term);
//    the term's atoms carry (x, u, v, 0) as hyper-duals; the u, v and mixed parts of its
//    minimum-image geometries go to gam[row][0..3)[G].
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bphg_geom(int nrows, int kv, int n, int nterms, int nb, int na, int ngeo,
                                                   const int4* __restrict__ tidx, const double* __restrict__ pos_all,
                                                   const double* __restrict__ boxes, const double* __restrict__ vec_all,
                                                   const double* __restrict__ ubar_all, long vstride,
                                                   double* __restrict__ gam_all) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)nrows * nterms) return;
    const size_t row = (size_t)(g / nterms);
    const int t = (int)(g % nterms);
    const size_t c = row / (size_t)kv, k = row % (size_t)kv;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const size_t at = c * (size_t)vstride + k * 3 * (size_t)n;
    const double* u = ubar_all + at;
    const double* v = vec_all + at;
    double3 L, T;
    load_box(boxes, c, L, T);
    const int4 ti = tidx[t];
    const int a3 = ti.x == 0 ? ti.z : ti.w;   // a bond has no third atom: its second again, unused
    HDual x1[3], x2[3], x3[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        x1[j] = HDual(pos[3 * ti.y + j], u[3 * ti.y + j], v[3 * ti.y + j], 0.0);
        x2[j] = HDual(pos[3 * ti.z + j], u[3 * ti.z + j], v[3 * ti.z + j], 0.0);
        x3[j] = HDual(pos[3 * a3 + j], u[3 * a3 + j], v[3 * a3 + j], 0.0);
    }
    HDual gam[3];
    term_gammas_pbc<HDual>(ti.x, x1, x2, x3, L, T, gam);
    double* o = gam_all + row * 3 * (size_t)ngeo + geom_start(t, nb, na);
    o[0] = gam[0].u; o[ngeo] = gam[0].w; o[2 * ngeo] = gam[0].uw;
    if (ti.x == 2) {   // straight-line stores, as k_bhg_geom
        o[1] = gam[1].u; o[ngeo + 1] = gam[1].w; o[2 * ngeo + 1] = gam[1].uw;
        o[2] = gam[2].u; o[ngeo + 2] = gam[2].w; o[2 * ngeo + 2] = gam[2].uw;
    }
}

// ---------------------------------------------------------------------------------
// 3. structure factors: one lane per (conformation, chunk, k), the atoms in atom order.  An atom's
//    phase is formed once from the atom-major table and feeds S and the chunk's S^u, S^v, S^uv, held in
//    registers.  Output per k: coeft[row][0..3) = 2 c_k (S^u, S^v, S^uv) of every row of the chunk and,
//    from the conformation's chunk 0, coef = 2 c_k S.
// ---------------------------------------------------------------------------------
struct SfacRow {
    double ur, ui, vr, vi, wr, wi;   // S^u, S^v, S^uv
};

__global__ void __launch_bounds__(256) k_bphg_sfac(int n, int kv, int nchunks, int KX, int KY, int KZ, long khalf,
                                                   double ke, double one_a2, const double* __restrict__ boxes,
                                                   const double* __restrict__ q_all, const double* __restrict__ vec_all,
                                                   const double* __restrict__ ubar_all, long vstride,
                                                   const double* __restrict__ qt_all,
                                                   const double2* __restrict__ tab_all, double2* __restrict__ coef_all,
                                                   double2* __restrict__ coeft_all) {
    const size_t c = blockIdx.y / (unsigned)nchunks;
    const int k0 = (int)(blockIdx.y % (unsigned)nchunks) * kPhgKC;
    const int kc = min(kPhgKC, kv - k0);   // rows this chunk has
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
    const size_t row0 = c * (size_t)kv + k0;
    const size_t at0 = c * (size_t)vstride + (size_t)k0 * 3 * (size_t)n;
    SfacRow a[kPhgKC];
#pragma unroll
    for (int s = 0; s < kPhgKC; s++) a[s] = SfacRow{0, 0, 0, 0, 0, 0};
    double cs = 0, ss = 0;
    for (int i = 0; i < n; i++) {
        const double2 e = phase(row + (size_t)i * KS, 1, KX, KY, nx, ny, nz);
        const double qi = q[i];
        cs += qi * e.x;
        ss += qi * e.y;
#pragma unroll
        for (int s = 0; s < kPhgKC; s++) {
            if (s < kc) {
                const size_t at = at0 + (size_t)s * 3 * (size_t)n + 3 * (size_t)i;
                const double* qt = qt_all + (row0 + s) * 3 * (size_t)n + i;
                const double ku = kx * ubar_all[at] + ky * ubar_all[at + 1] + kz * ubar_all[at + 2];
                const double kw = kx * vec_all[at] + ky * vec_all[at + 1] + kz * vec_all[at + 2];
                const double qu = qt[0], qv = qt[n], quv = qt[2 * (size_t)n];
                const double bu = qi * ku, bv = qi * kw;            // S^u: (qu + i bu) e
                const double ar = quv - bu * kw, ai = qu * kw + qv * ku;   // S^uv: (ar + i ai) e
                a[s].ur += qu * e.x - bu * e.y; a[s].ui += qu * e.y + bu * e.x;
                a[s].vr += qv * e.x - bv * e.y; a[s].vi += qv * e.y + bv * e.x;
                a[s].wr += ar * e.x - ai * e.y; a[s].wi += ar * e.y + ai * e.x;
            }
        }
    }
    const double k2 = kx * kx + ky * ky + kz * kz;
    const double eak = exp(-k2 * 0.25 * one_a2) / k2;
    const double cst = 4.0 / L.x / L.y / L.z * kPi * ke;
    const double f = 2.0 * cst * eak;
    if (k0 == 0) coef_all[c * (size_t)khalf + k] = make_double2(f * cs, f * ss);
#pragma unroll
    for (int s = 0; s < kPhgKC; s++) {
        if (s < kc) {
            double2* o = coeft_all + (row0 + s) * 3 * (size_t)khalf + k;
            o[0] = make_double2(f * a[s].ur, f * a[s].ui);
            o[khalf] = make_double2(f * a[s].vr, f * a[s].vi);
            o[2 * (size_t)khalf] = make_double2(f * a[s].wr, f * a[s].wi);
        }
    }
}

// ---------------------------------------------------------------------------------
// 4. direct space, the first hot kernel.  The block shape of the periodic pair kernels: kPhgI = 64
//    i-atoms of one conformation, one per lane in each of the four waves, TIMES a chunk of kPhgKC = 4
//    direction rows: blockIdx.y = conformation * nchunks + chunk.  The j-atoms pass through LDS in
//    tiles of kPhgJ = 128 entries -- (x, y, z, q) once and, per row of the chunk, (u, q^u), (v, q^v)
//    and q^uv, 9 doubles -- and wave w takes entries [32 w, 32 w + 32) of every tile as LDS
//    broadcasts.  Per pair, ONCE: the minimum image, the excluded test, the erf pair at any distance
//    or the erfc pair (erfc_exp, the handle's erfcx table in LDS) within the cutoff, and from them
//    gp = ke P / r, g3 = ke Q / r^3 and g5 = ke (3 Q + 2 T) / r^5.  Per direction row: d.w^u, d.w^v,
//    w^u.w^v and the three accumulators.  The waves' partial sums are added as (w0 + w1) + (w2 + w3)
//    through the LDS the row tiles no longer need.  A row the tail chunk lacks is zeros in LDS and
//    registers, never a global address.  Writes the pair parts of g^u, g^v, g^uv per row and, from
//    the conformation's chunk 0, of g (every chunk sums it).
//    LDS: table 8256 B + atoms 4096 B + row tiles 8 x 4096 B + q^uv 4 x 1024 B = 49216 B (48.1 KiB):
//    three blocks fit a CU's 160 KiB.
// ---------------------------------------------------------------------------------
constexpr int kPhgI = 64;
constexpr int kPhgJ = 128;
constexpr int kPhgSums = 3 * kPhgKC + 1;
static_assert(3 * kPhgSums * kPhgI * sizeof(double) <= 2 * kPhgKC * kPhgJ * sizeof(double4),
              "the reduction reuses the row tiles");

__global__ void __launch_bounds__(256) k_bphg_pairs(int n, int kv, int nchunks, double ke, double alpha, double rc2,
                                                    double erfc_scale, const double* __restrict__ erfc_tab,
                                                    const double* __restrict__ boxes,
                                                    const double* __restrict__ pos_all, const double* __restrict__ q_all,
                                                    const double* __restrict__ vec_all,
                                                    const double* __restrict__ ubar_all, long vstride,
                                                    const double* __restrict__ qt_all, const int* __restrict__ ex_start,
                                                    const int* __restrict__ ex_list, double* __restrict__ g_all,
                                                    double* __restrict__ gt_all) {
    __shared__ double tab[kErfcMaxM * (kErfcDeg + 1)];
    __shared__ double4 sp[kPhgJ];                 // (x, y, z, q)
    __shared__ double4 srow[2 * kPhgKC][kPhgJ];   // row k: [k] = (u, q^u), [kPhgKC + k] = (v, q^v)
    __shared__ double sq[kPhgKC][kPhgJ];          // q^uv
    for (int e = threadIdx.x; e < kErfcMaxM * (kErfcDeg + 1); e += 256) tab[e] = erfc_tab[e];
    const size_t c = blockIdx.y / (unsigned)nchunks;
    const int k0 = (int)(blockIdx.y % (unsigned)nchunks) * kPhgKC;
    const int kc = min(kPhgKC, kv - k0);          // rows this chunk has
    const size_t row0 = c * (size_t)kv + k0;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    const size_t at0 = c * (size_t)vstride + (size_t)k0 * 3 * (size_t)n;
    double3 L, T;
    load_box(boxes, c, L, T);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kPhgI + lane;
    const bool active = i < n;
    double3 xi = make_double3(0, 0, 0);
    double ui[kPhgKC][3], vi[kPhgKC][3];
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        xi = ld3(pos, i);
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int k = 0; k < kPhgKC; k++) {
        const bool have = active && k < kc;
        const size_t at = at0 + (size_t)k * 3 * (size_t)n + 3 * (size_t)i;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            ui[k][j] = have ? ubar_all[at + j] : 0.0;
            vi[k][j] = have ? vec_all[at + j] : 0.0;
        }
    }
#pragma unroll
    for (int m = 0; m < kMaxRegExcl; m++) reg[m] = m < exc ? ex_list[ex0 + m] : -1;
    const double two_over_sqrtpi = 1.1283791670955126;
    double g = 0, gu[kPhgKC], gv[kPhgKC], guv[kPhgKC];
#pragma unroll
    for (int k = 0; k < kPhgKC; k++) gu[k] = gv[k] = guv[k] = 0;
    for (int base = 0; base < n; base += kPhgJ) {
        __syncthreads();   // (first tile: the erfcx table is staged)
        // the tile: item = slot * kPhgJ + entry, slot 0 the atoms, slot 1 + k row k of the chunk
        for (int item = threadIdx.x; item < (1 + kPhgKC) * kPhgJ; item += 256) {
            const int e = item % kPhgJ, slot = item / kPhgJ;
            const int j = base + e;
            if (j >= n) continue;
            if (slot == 0) {
                sp[e] = make_double4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], q[j]);
                continue;
            }
            const int k = slot - 1;
            double4 uj = make_double4(0, 0, 0, 0), vj = make_double4(0, 0, 0, 0);
            double quv = 0;
            if (k < kc) {
                const size_t at = at0 + (size_t)k * 3 * (size_t)n + 3 * (size_t)j;
                const double* qt = qt_all + (row0 + k) * 3 * (size_t)n + j;
                uj = make_double4(ubar_all[at], ubar_all[at + 1], ubar_all[at + 2], qt[0]);
                vj = make_double4(vec_all[at], vec_all[at + 1], vec_all[at + 2], qt[n]);
                quv = qt[2 * (size_t)n];
            }
            srow[k][e] = uj; srow[kPhgKC + k][e] = vj; sq[k][e] = quv;
        }
        __syncthreads();
        const int t1 = min(32 * w + 32, n - base);
        if (!active) continue;
        for (int t = 32 * w; t < t1; t++) {
            const int jj = base + t;
            if (jj == i) continue;
            const double4 pj = sp[t];
            const double3 d = delta_r(make_double3(pj.x, pj.y, pj.z), xi, L, 1, T);   // x_i - x_j
            const double r2 = d.x * d.x + d.y * d.y + d.z * d.z;
            // p = P, dp = Q, x3 = 2 T
            double p, dp, x3, inv_r;
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) {
                const double r = sqrt(r2);
                inv_r = 1.0 / r;
                const double ar = alpha * r;
                const double ee = ar * exp(-ar * ar) * two_over_sqrtpi;
                p = -erf(ar);
                dp = p + ee;
                x3 = 2 * (ar * ar) * ee;
            } else {
                if (!(r2 <= rc2)) continue;
                inv_r = rsqrt_fp64(r2);
                const double ar = alpha * (r2 * inv_r);
                double e2;
                p = erfc_exp(ar, tab, erfc_scale, e2);
                const double ee = ar * e2 * two_over_sqrtpi;
                dp = p + ee;
                x3 = 2 * (ar * ar) * ee;
            }
            const double inv_r2 = inv_r * inv_r;
            const double kr = ke * inv_r;
            const double gp = kr * p;                         // ke P / r
            const double g3 = kr * dp * inv_r2;               // ke Q / r^3
            const double g5 = kr * (3 * dp + x3) * inv_r2 * inv_r2 * pj.w;   // ke q_j (3 Q + 2 T) / r^5
            const double g3q = g3 * pj.w;
            g += gp * pj.w;
#pragma unroll
            for (int k = 0; k < kPhgKC; k++) {
                const double4 uj = srow[k][t], vj = srow[kPhgKC + k][t];
                const double wux = ui[k][0] - uj.x, wuy = ui[k][1] - uj.y, wuz = ui[k][2] - uj.z;
                const double wvx = vi[k][0] - vj.x, wvy = vi[k][1] - vj.y, wvz = vi[k][2] - vj.z;
                const double du = d.x * wux + d.y * wuy + d.z * wuz;
                const double dv = d.x * wvx + d.y * wvy + d.z * wvz;
                const double uv = wux * wvx + wuy * wvy + wuz * wvz;
                gu[k] += gp * uj.w - g3q * du;
                gv[k] += gp * vj.w - g3q * dv;
                guv[k] += gp * sq[k][t] - g3 * (uj.w * dv + vj.w * du + pj.w * uv) + g5 * du * dv;
            }
        }
    }
    __syncthreads();   // every wave is done with the tiles: their LDS takes the partial sums of waves 1..3
    double (*red)[kPhgSums][kPhgI] = reinterpret_cast<double (*)[kPhgSums][kPhgI]>(&srow[0][0]);
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < kPhgKC; k++) {
            red[w - 1][3 * k][lane] = gu[k]; red[w - 1][3 * k + 1][lane] = gv[k]; red[w - 1][3 * k + 2][lane] = guv[k];
        }
        red[w - 1][3 * kPhgKC][lane] = g;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    auto tot = [&](double a, int m) { return (a + red[0][m][lane]) + (red[1][m][lane] + red[2][m][lane]); };
#pragma unroll
    for (int k = 0; k < kPhgKC; k++) {
        if (k < kc) {
            double* o = gt_all + (row0 + k) * 3 * (size_t)n + i;
            o[0] = tot(gu[k], 3 * k);
            o[n] = tot(gv[k], 3 * k + 1);
            o[2 * (size_t)n] = tot(guv[k], 3 * k + 2);
        }
    }
    if (k0 == 0) g_all[c * (size_t)n + i] = tot(g, 3 * kPhgKC);
}

// ---------------------------------------------------------------------------------
// 5. reciprocal part, the second hot kernel.  k_bph_recip's shape: 64 atoms of one conformation per
//    block, one per lane in each of the four waves, times a chunk of kPhgKC rows; the k-vectors pass
//    through LDS in tiles of kPhgK = 128 entries -- A = 2 c_k S, per row of the chunk A^u, A^v and
//    A^uv (26 doubles) and the integer triple -- and wave w takes entries [32 w, 32 w + 32) of every
//    tile.  The phase from the entry-major table, ONCE per (atom, k), with R = Re[conj(e) A] and
//    G = -Im[conj(e) A]; g += R once.  Per row, with kappa^u_i and kappa^v_i from the lane's own u_i,
//    v_i and the triple, and R^x, G^x the same of A^x:
//        g^u  += R^u - kappa^u G,    g^v += R^v - kappa^v G,
//        g^uv += R^uv - kappa^u G^v - kappa^v G^u - kappa^u kappa^v R.
//    The partial sums are added as (w0 + w1) + (w2 + w3) through the LDS the tiles no longer need.
//    Epilogue, this lane's own atom: the conformation's chunk 0 completes g, every row completes g^u,
//    g^v, g^uv: (pair part + reciprocal part) - 2 c_s (q, q^u, q^v, q^uv).
//    LDS: 128 x (26 doubles + 16 B) = 28672 B (28 KiB); the partial sums (3 x 13 x 512 B) reuse it.
// ---------------------------------------------------------------------------------
constexpr int kPhgK = 128;
static_assert(3 * kPhgSums * 64 * sizeof(double) <= 3 * kPhgKC * kPhgK * sizeof(double2),
              "the reduction reuses the coefficient tiles");

__global__ void __launch_bounds__(256) k_bphg_recip(int n, int kv, int nchunks, int KX, int KY, int KZ, long khalf,
                                                    double cself, const double* __restrict__ boxes,
                                                    const double* __restrict__ q_all, const double* __restrict__ vec_all,
                                                    const double* __restrict__ ubar_all, long vstride,
                                                    const double* __restrict__ qt_all,
                                                    const double2* __restrict__ tab_t_all,
                                                    const double2* __restrict__ coef_all,
                                                    const double2* __restrict__ coeft_all, double* __restrict__ g_all,
                                                    double* __restrict__ gt_all) {
    __shared__ double2 sa[kPhgK];                  // A
    __shared__ double2 st[3 * kPhgKC][kPhgK];      // row k: [3 k] = A^u, [3 k + 1] = A^v, [3 k + 2] = A^uv
    __shared__ int4 sn[kPhgK];
    const size_t c = blockIdx.y / (unsigned)nchunks;
    const int k0 = (int)(blockIdx.y % (unsigned)nchunks) * kPhgKC;
    const int kc = min(kPhgKC, kv - k0);
    const size_t row0 = c * (size_t)kv + k0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const bool active = i < n;
    const int KS = KX + KY + KZ;
    const double2* row = tab_t_all + c * (size_t)n * KS + (active ? i : 0);   // entry m at row[m * n]
    const double2* coef = coef_all + c * (size_t)khalf;
    double3 L, T;
    load_box(boxes, c, L, T);
    const double fx = 2.0 * kPi / L.x, fy = 2.0 * kPi / L.y, fz = 2.0 * kPi / L.z;
    double wu[kPhgKC][3], wv[kPhgKC][3];   // u_i, v_i times 2 pi / L: kappa_i = n . w
#pragma unroll
    for (int k = 0; k < kPhgKC; k++) {
        const bool have = active && k < kc;
        const size_t at = c * (size_t)vstride + (size_t)(k0 + k) * 3 * (size_t)n + 3 * (size_t)i;
        wu[k][0] = have ? ubar_all[at] * fx : 0.0; wu[k][1] = have ? ubar_all[at + 1] * fy : 0.0;
        wu[k][2] = have ? ubar_all[at + 2] * fz : 0.0;
        wv[k][0] = have ? vec_all[at] * fx : 0.0; wv[k][1] = have ? vec_all[at + 1] * fy : 0.0;
        wv[k][2] = have ? vec_all[at + 2] * fz : 0.0;
    }
    double g = 0, gu[kPhgKC], gv[kPhgKC], guv[kPhgKC];
#pragma unroll
    for (int k = 0; k < kPhgKC; k++) gu[k] = gv[k] = guv[k] = 0;
    for (long base = 0; base < khalf; base += kPhgK) {
        __syncthreads();
        // the tile: item = slot * kPhgK + entry, slot 0 A and the triple, slot 1 + m tangent m of the chunk
        for (int item = threadIdx.x; item < (1 + 3 * kPhgKC) * kPhgK; item += 256) {
            const int e = item % kPhgK, slot = item / kPhgK;
            const long k = base + e;
            if (k >= khalf) continue;
            if (slot == 0) {
                int nx, ny, nz;
                half_space_k(k, KY, KZ, nx, ny, nz);
                sa[e] = coef[k];
                sn[e] = make_int4(nx, ny, nz, 0);
                continue;
            }
            const int m = slot - 1;   // row m / 3 of the chunk, tangent m % 3
            st[m][e] = m / 3 < kc ? coeft_all[((row0 + m / 3) * 3 + m % 3) * (size_t)khalf + k] : make_double2(0, 0);
        }
        __syncthreads();
        const int t1 = (int)min((long)(32 * w + 32), khalf - base);
        if (!active) continue;
        for (int t = 32 * w; t < t1; t++) {
            const double2 ab = sa[t];
            const int4 nn = sn[t];
            const double2 e = phase(row, (size_t)n, KX, KY, nn.x, nn.y, nn.z);
            const double R = ab.x * e.x + ab.y * e.y;
            const double G = ab.x * e.y - ab.y * e.x;
            g += R;
#pragma unroll
            for (int k = 0; k < kPhgKC; k++) {
                const double2 au = st[3 * k][t], av = st[3 * k + 1][t], aw = st[3 * k + 2][t];
                const double ku = nn.x * wu[k][0] + nn.y * wu[k][1] + nn.z * wu[k][2];
                const double kw = nn.x * wv[k][0] + nn.y * wv[k][1] + nn.z * wv[k][2];
                const double Ru = au.x * e.x + au.y * e.y, Gu = au.x * e.y - au.y * e.x;
                const double Rv = av.x * e.x + av.y * e.y, Gv = av.x * e.y - av.y * e.x;
                const double Rw = aw.x * e.x + aw.y * e.y;
                gu[k] += Ru - ku * G;
                gv[k] += Rv - kw * G;
                guv[k] += Rw - ku * Gv - kw * Gu - ku * kw * R;
            }
        }
    }
    __syncthreads();   // every wave is done with the tiles: their LDS takes the partial sums of waves 1..3
    double (*red)[kPhgSums][64] = reinterpret_cast<double (*)[kPhgSums][64]>(&st[0][0]);
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < kPhgKC; k++) {
            red[w - 1][3 * k][lane] = gu[k]; red[w - 1][3 * k + 1][lane] = gv[k]; red[w - 1][3 * k + 2][lane] = guv[k];
        }
        red[w - 1][3 * kPhgKC][lane] = g;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    auto tot = [&](double a, int m) { return (a + red[0][m][lane]) + (red[1][m][lane] + red[2][m][lane]); };
    const size_t at = c * (size_t)n + i;
    if (k0 == 0) g_all[at] = (g_all[at] + tot(g, 3 * kPhgKC)) - 2 * cself * q_all[at];   // no other chunk touches g
#pragma unroll
    for (int k = 0; k < kPhgKC; k++) {
        if (k < kc) {
            double* o = gt_all + (row0 + k) * 3 * (size_t)n + i;
            const double* qt = qt_all + (row0 + k) * 3 * (size_t)n + i;
            o[0] = (o[0] + tot(gu[k], 3 * k)) - 2 * cself * qt[0];
            o[n] = (o[n] + tot(gv[k], 3 * k + 1)) - 2 * cself * qt[n];
            o[2 * (size_t)n] = (o[2 * (size_t)n] + tot(guv[k], 3 * k + 2)) - 2 * cself * qt[2 * (size_t)n];
        }
    }
}

// ---------------------------------------------------------------------------------
// 6. the gradient rows, k_bhg_rows's scheme: one lane per flattened (conformation, owner), the owners
//    of a conformation being its N atoms and then its terms.  An atom: the running sum (zero, or what
//    an earlier pass of this conformation's directions left in grad) + g^uv_i of the pass's rows in
//    ascending k.  A term: its own geometry from minimum-image vectors in plain doubles, g of its
//    atoms, then its rows in ascending k added to running sums that start as an atom's does.
//    grad[c][N + ...] in the order of the cf_params arrays: bonds (k, b), angles (k, theta0), waters
//    (k1, k2, kub, b0, ub0).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bphg_rows(int nconf, int kv, int n, int nterms, int nb, int na, int ngeo,
                                                   long np, int first, const int4* __restrict__ tidx,
                                                   const double* __restrict__ tpar, const double* __restrict__ pos_all,
                                                   const double* __restrict__ boxes, const double* __restrict__ g_all,
                                                   const double* __restrict__ gt_all,
                                                   const double* __restrict__ gam_all, double* __restrict__ grad_all) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    const long owners = (long)n + nterms;
    if (gi >= (long)nconf * owners) return;
    const size_t c = (size_t)(gi / owners);
    const int t = (int)(gi % owners) - n;
    if (t < 0) {
        const int i = t + n;
        double* o = grad_all + c * (size_t)np + i;
        double s = first ? 0.0 : *o;
        const double* guv = gt_all + (c * (size_t)kv * 3 + 2) * (size_t)n + i;
        for (int k = 0; k < kv; k++) s += guv[(size_t)k * 3 * (size_t)n];
        *o = s;
        return;
    }
    const int4 ti = tidx[t];
    const double* p = tpar + 5 * t;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* gw = g_all + c * (size_t)n;
    double3 L, T;
    load_box(boxes, c, L, T);
    const int a1 = ti.y, a2 = ti.z, a3 = ti.x == 0 ? ti.z : ti.w;
    double x1[3], x2[3], x3[3], gam[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 3; j++) { x1[j] = pos[3 * a1 + j]; x2[j] = pos[3 * a2 + j]; x3[j] = pos[3 * a3 + j]; }
    term_gammas_pbc<double>(ti.x, x1, x2, x3, L, T, gam);
    const int geo0 = geom_start(t, nb, na);
    const size_t sn = (size_t)n, sg = (size_t)ngeo;
    if (ti.x != 2) {
        // bond: c = (1, -1) over (p1, p2); angle: c = (1, -2, 1) over (p1, p2, p3)
        const double c2 = ti.x == 0 ? -1.0 : -2.0, c3 = ti.x == 0 ? 0.0 : 1.0;
        double* out = grad_all + c * (size_t)np + n + 2 * t;
        const double cg = gw[a1] + c2 * gw[a2] + c3 * gw[a3];
        const double dev = gam[0] - p[1];
        double sk = first ? 0.0 : out[0], sr = first ? 0.0 : out[1];
        for (int k = 0; k < kv; k++) {
            const size_t row = c * (size_t)kv + k;
            const double* gu = gt_all + row * 3 * sn;
            const double* mu = gam_all + row * 3 * sg + geo0;
            const double cu = gu[a1] + c2 * gu[a2] + c3 * gu[a3];
            const double cv = gu[sn + a1] + c2 * gu[sn + a2] + c3 * gu[sn + a3];
            const double cuv = gu[2 * sn + a1] + c2 * gu[2 * sn + a2] + c3 * gu[2 * sn + a3];
            sk += cuv * dev + cu * mu[sg] + cv * mu[0] + cg * mu[2 * sg];
            sr += -p[0] * cuv;
        }
        out[0] = sk; out[1] = sr;
    } else {
        // water (O, H1, H2): k1 (r12 - b0) into H1 and k1 (r13 - b0) into H2, k2 crosswise, kub (r23 - ub0)
        // into both, the oxygen minus what the hydrogens get
        double* out = grad_all + c * (size_t)np + n + 2 * nb + 2 * na + 5 * (t - nb - na);
        const double g2 = gw[a2] - gw[a1], g3 = gw[a3] - gw[a1];
        const double e12 = gam[0] - p[3], e13 = gam[1] - p[3], e23 = gam[2] - p[4];
        double s[5];
#pragma unroll
        for (int m = 0; m < 5; m++) s[m] = first ? 0.0 : out[m];
        for (int k = 0; k < kv; k++) {
            const size_t row = c * (size_t)kv + k;
            const double* gu = gt_all + row * 3 * sn;
            const double* mu = gam_all + row * 3 * sg + geo0;
            const double* mv = mu + sg;
            const double* muv = mu + 2 * sg;
            const double u2 = gu[a2] - gu[a1], u3 = gu[a3] - gu[a1];
            const double v2 = gu[sn + a2] - gu[sn + a1], v3 = gu[sn + a3] - gu[sn + a1];
            const double w2 = gu[2 * sn + a2] - gu[2 * sn + a1], w3 = gu[2 * sn + a3] - gu[2 * sn + a1];
            // piece(c, m) = c^uv (gamma_m - ref) + c^u gamma_m^v + c^v gamma_m^u + c^g gamma_m^uv
            const double p2_12 = w2 * e12 + u2 * mv[0] + v2 * mu[0] + g2 * muv[0];
            const double p3_13 = w3 * e13 + u3 * mv[1] + v3 * mu[1] + g3 * muv[1];
            const double p2_13 = w2 * e13 + u2 * mv[1] + v2 * mu[1] + g2 * muv[1];
            const double p3_12 = w3 * e12 + u3 * mv[0] + v3 * mu[0] + g3 * muv[0];
            s[0] += p2_12 + p3_13;
            s[1] += p2_13 + p3_12;
            s[2] += (w2 + w3) * e23 + (u2 + u3) * mv[2] + (v2 + v3) * mu[2] + (g2 + g3) * muv[2];
            s[3] += -(p[0] + p[1]) * (w2 + w3);
            s[4] += -p[2] * (w2 + w3);
        }
#pragma unroll
        for (int m = 0; m < 5; m++) out[m] = s[m];
    }
}

// ---------------------------------------------------------------------------------
// launcher: one pass of nconf <= w.cap conformations x kv directions, nconf * kv <= gw.cap rows, at
// most nine launches
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }
static inline size_t ngeom(const Handle& h) { return (size_t)h.nb + (size_t)h.na + 3 * (size_t)h.nw; }

size_t batch_pbc_hvp_grad_doubles_per_row(const Handle& h) {
    // coeft [3][khalf] x 2, the geometries' three tangents, (q^u, q^v, q^uv)[N], (g^u, g^v, g^uv)[N], g[N]
    return 6 * (size_t)h.khalf + 3 * ngeom(h) + 7 * (size_t)h.n;
}

void batch_pbc_hvp_grad_carve(const Handle& h, double* base, int cap, BatchPbcHvpGradWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n;
    w.base = base; w.cap = cap;
    w.coeft = reinterpret_cast<double2*>(base);
    w.gam = reinterpret_cast<double*>(w.coeft + c * 3 * (size_t)h.khalf);
    w.qt = w.gam + c * 3 * ngeom(h);
    w.gt = w.qt + c * 3 * n;
    w.g = w.gt + c * 3 * n;
}

void launch_batch_pbc_hvp_vjp(Handle& h, const BatchPbcWs& w, const BatchPbcHvpGradWs& gw, int nconf, int kv,
                              const double* pos, const double* boxes, const double* vec, const double* out_bar,
                              long vstride, bool first, double* grad) {
    const int64_t rows64 = (int64_t)nconf * kv;
    if (nconf <= 0 || kv <= 0 || nconf > w.cap || rows64 > gw.cap || rows64 > kBatchMaxPass)
        throw std::invalid_argument("launch_batch_pbc_hvp_vjp: pass size");
    const int n = h.n, rows = (int)rows64, ngeo = (int)ngeom(h);
    const long np = (long)n + 2L * h.nb + 2L * h.na + 5L * h.nw;
    const int nchunks = nblk(kv, kPhgKC);
    const int KX = h.kmax[0], KY = h.kmax[1], KZ = h.kmax[2];
    const long khalf = (long)h.khalf;
    launch_batch_pbc_flux_charges(h, w, nconf, pos, boxes, nullptr);
    launch_batch_pbc_tables(h, w, nconf, pos, boxes);
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bphg_geom, dim3(nblk((int64_t)rows * h.nterms, 256)), dim3(256), 0, h.stream, rows, kv, n,
                           h.nterms, h.nb, h.na, ngeo, h.term_idx, pos, boxes, vec, out_bar, vstride, gw.gam);
    launch_batch_hvp_qtan(h, rows, gw.gam, gw.qt);
    const dim3 kgrid(nblk(khalf, 256), nconf * nchunks), agrid(nblk(n, kPhgI), nconf * nchunks);
    hipLaunchKernelGGL(k_bphg_sfac, kgrid, dim3(256), 0, h.stream, n, kv, nchunks, KX, KY, KZ, khalf, h.ke,
                       1.0 / (h.alpha * h.alpha), boxes, w.q, vec, out_bar, vstride, gw.qt, w.tab, w.coef, gw.coeft);
    hipLaunchKernelGGL(k_bphg_pairs, agrid, dim3(256), 0, h.stream, n, kv, nchunks, h.ke, h.alpha, h.cutoff * h.cutoff,
                       h.erfc_scale, h.erfc_tab, boxes, pos, w.q, vec, out_bar, vstride, gw.qt, h.ex_start, h.ex_list,
                       gw.g, gw.gt);
    hipLaunchKernelGGL(k_bphg_recip, agrid, dim3(256), 0, h.stream, n, kv, nchunks, KX, KY, KZ, khalf,
                       h.ke * h.alpha / sqrt(kPi), boxes, w.q, vec, out_bar, vstride, gw.qt, w.tab_t, w.coef, gw.coeft,
                       gw.g, gw.gt);
    hipLaunchKernelGGL(k_bphg_rows, dim3(nblk((int64_t)nconf * (n + h.nterms), 256)), dim3(256), 0, h.stream, nconf, kv,
                       n, h.nterms, h.nb, h.na, ngeo, np, first ? 1 : 0, h.term_idx, h.term_par, pos, boxes, gw.g, gw.gt,
                       gw.gam, grad);
}

}  // namespace cf
