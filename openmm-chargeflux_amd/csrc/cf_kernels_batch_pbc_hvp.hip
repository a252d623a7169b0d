// cf_kernels_batch_pbc_hvp.hip -- cf_compute_batch_periodic_hvp: Hessian-vector products of the
// periodic batch (cf_kernels_batch_pbc.hip) with respect to the positions ("batched,
// periodic, Hessian-vector products").  Per conformation x, box and direction v, with F the forces
// of cf_compute_batch_periodic, H v = -D_v F at fixed box, pair set and image of every pair:
//     (H v)_i = -D_v F_i^pair - D_v F_i^recip + sum_a (gdot_a D_ai + g_a Ddot_ai)
// d = minimum image of x_i - x_j, r = |d|, w = v_i - v_j, qdot = D_v q, D = dq/dx (k_bp_flux's blocks),
// Ddot = D_v D (the flux terms on dual numbers, flux_term_pbc of cf_flux_dual.h), c = 2 / sqrt(pi).
// Pair part (phi the erfc function within the cutoff, the erf function for an excluded pair at any
// distance; P = phi r, Q = -phi' r^2 = P + c (alpha r) e^{-alpha^2 r^2}, Q' = -2 c alpha (alpha r)^2 e^{..}):
//     F_i^pair = sum_j s d,   s = (A + C Q) / r^2,  A = e4 s6 (12 s6 - 6) (0 if excluded),  C = ke q_i q_j / r
//     D_v F_i^pair = sum_j (sdot d + s w)
//     sdot = [e4 s6 (48 - 168 s6) - C (3 Q + 2 c (alpha r)^3 e^{..})] (d.w) / r^4 + ke Q (qdot_i q_j + q_i qdot_j) / r^3
//     g_i    = ke sum_j q_j P / r - 2 c_s q_i + sum_k Re[conj(e_i) A_k]
//     gdot_i = ke sum_j (P qdot_j - Q q_j (d.w) / r^2) / r - 2 c_s qdot_i
//              + sum_k (Re[conj(e_i) B_k] + kappa_i Im[conj(e_i) A_k])
// (g and gdot: g_i and h_i of cf_kernels_batch_pbc_grad.hip with v in F_bar's place), c_s = ke alpha / sqrt(pi).
// Reciprocal part, k_bp_recip's signs: A_k = 2 c_k S, B_k = 2 c_k Sdot, e_i = e^{i k.x_i}, kappa_i = k.v_i,
//     F_i^recip = q_i sum_k k G,   G = A.x e.y - A.y e.x = -Im[conj(e_i) A]
//     D_v F_i^recip = qdot_i sum_k k G + q_i sum_k k (B.x e.y - B.y e.x + kappa_i Re[conj(e_i) A])
// over the forward path's half-space k set, k from the box diagonals.  Nothing divides by a
// parameter: k = 0 is legal.
//
// The per-pair and per-(atom, k) work that does not depend on the direction -- minimum image, rsqrt,
// the erfc lookup, exp, in_excl, the phase products -- is done once for a CHUNK of kBphKD directions
// of a conformation: blockIdx.y of k_bph_sfac, k_bph_pairs and k_bph_recip is (conformation, chunk).
// A conformation's tail chunk runs the same code with its unused slots zero-filled and not written.
// A pass: k_bp_flux, k_b_charges, k_bp_tables (as they are, once per conformation), then k_bph_terms,
// k_bph_qdot, k_bph_sfac, k_bph_pairs, k_bph_recip, k_bph_chain: at most nine launches.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N, the topology and kmax, and every
// direction runs the same per-slot function whatever its slot: the row of a (conformation, direction)
// is bitwise the same alone, at any position of any batch, for any nvec and under any pass size.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms, khalf, kv and the launch's own counts: no device guard bits.
#include <stdexcept>

#include "cf_flux_dual.h"

#ifndef CF_BPH_KD
#define CF_BPH_KD 4
#endif

namespace cf {

constexpr int kBphKD = CF_BPH_KD;   // directions per chunk (a build-time switch: the probe also builds 1)
static_assert(kBphKD >= 1 && kBphKD <= 8, "directions per chunk");

// ---------------------------------------------------------------------------------
// 1. term tangents: k_bh_terms with the conformation's box.  One lane per flattened (row, term),
//    g = cv * nterms + t, cv = c * kv + k; the lane's Ddot block goes to LDS and the block's run is
//    written coalesced; the tangents of the term's charge slots go to dslot[cv][S].
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bph_terms(int nrows, int kv, int n, int nterms, int nb, int na, int nslots,
                                                   long nd3, const int4* __restrict__ tidx,
                                                   const double* __restrict__ tpar, const double* __restrict__ pos_all,
                                                   const double* __restrict__ boxes, const double* __restrict__ vec_all,
                                                   long vstride, double* __restrict__ dslot_all,
                                                   double* __restrict__ ddot_all) {
    __shared__ double st[256 * 27];
    const long total = (long)nrows * nterms;
    const long g0 = (long)blockIdx.x * 256;
    const long g = g0 + threadIdx.x;
    const long base = batch_dqdx_at(g0, nterms, nb, na, nd3);
    if (g < total) {
        const size_t cv = (size_t)(g / nterms);
        const int t = (int)(g % nterms);
        const size_t c = cv / (size_t)kv, k = cv % (size_t)kv;
        const double* pos = pos_all + c * 3 * (size_t)n;
        const double* vec = vec_all + c * (size_t)vstride + k * 3 * (size_t)n;
        double3 L, T;
        load_box(boxes, c, L, T);
        const int4 ti = tidx[t];
        const int a3 = ti.x == 0 ? ti.z : ti.w;   // a bond has no third atom: its second again, unused
        Dual x1[3], x2[3], x3[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            x1[j] = Dual(pos[3 * ti.y + j], vec[3 * ti.y + j]);
            x2[j] = Dual(pos[3 * ti.z + j], vec[3 * ti.z + j]);
            x3[j] = Dual(pos[3 * a3 + j], vec[3 * a3 + j]);
        }
        double* o = st + (batch_dqdx_at(g, nterms, nb, na, nd3) - base);
        Dual dq[3];
        flux_term_pbc<Dual>(ti.x, tpar + 5 * t, x1, x2, x3, L, T, dq, [o](int e, Dual val) { o[e] = val.d; });
        double* ds = dslot_all + cv * (size_t)nslots;
        if (ti.x == 0) {
            ds[2 * t] = dq[0].d; ds[2 * t + 1] = dq[1].d;
        } else {   // angles then waters: 3 slots each
            const int s = 2 * nb + 3 * (t - nb);
            ds[s] = dq[0].d; ds[s + 1] = dq[1].d; ds[s + 2] = dq[2].d;
        }
    }
    __syncthreads();
    const int len = (int)(batch_dqdx_at(min(g0 + 256, total), nterms, nb, na, nd3) - base);
    for (int e = threadIdx.x; e < len; e += 256) ddot_all[base + e] = st[e];
}

// ---------------------------------------------------------------------------------
// 2. charge tangents: one lane per (row, atom), the atom's slot tangents added in qcsr slot order
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bph_qdot(int n, int nslots, const int* __restrict__ qs,
                                                  const int* __restrict__ qslot, const double* __restrict__ dslot_all,
                                                  double* __restrict__ qdot_all) {
    const size_t cv = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* ds = dslot_all + cv * (size_t)nslots;
    double qd = 0;
    for (int s = qs[i]; s < qs[i + 1]; s++) qd += ds[qslot[s]];
    qdot_all[cv * (size_t)n + i] = qd;
}

// ---------------------------------------------------------------------------------
// 3. structure factors: one lane per (conformation, chunk, k), the atoms in atom order.  An atom's
//    phase is formed once and feeds S and the Sdot of the chunk's directions, held in registers:
//    Sdot = sum_j (qdot_j + i q_j kappa_j) e_j, kappa_j = k . v_j.  Output per k: coefd[cv] =
//    2 c_k Sdot of every direction of the chunk and, from the conformation's chunk 0, coef = 2 c_k S.
// ---------------------------------------------------------------------------------
struct SfacSlot {
    const double* vel;    // the direction [N][3]; null: an unused slot of a tail chunk
    const double* qdot;   // its charge tangents [N]
    double cd, sd;
};

__device__ __forceinline__ void sfac_slot(SfacSlot& s, int i, double qi, double2 e, double kx, double ky, double kz) {
    const double qk = qi * (kx * s.vel[3 * i] + ky * s.vel[3 * i + 1] + kz * s.vel[3 * i + 2]);
    const double qd = s.qdot[i];
    s.cd += qd * e.x - qk * e.y;
    s.sd += qd * e.y + qk * e.x;
}

__global__ void __launch_bounds__(256) k_bph_sfac(int n, int kv, int nchunk, int KX, int KY, int KZ, long khalf,
                                                  double ke, double one_a2, const double* __restrict__ boxes,
                                                  const double* __restrict__ q_all, const double* __restrict__ vec_all,
                                                  long vstride, const double* __restrict__ qdot_all,
                                                  const double2* __restrict__ tab_all, double2* __restrict__ coef_all,
                                                  double2* __restrict__ coefd_all) {
    const size_t c = blockIdx.y / (unsigned)nchunk;
    const int k0 = (int)(blockIdx.y % (unsigned)nchunk) * kBphKD;   // the chunk's first direction
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
    SfacSlot sl[kBphKD];
#pragma unroll
    for (int s = 0; s < kBphKD; s++) {
        const bool on = k0 + s < kv;
        sl[s].vel = on ? vec_all + c * (size_t)vstride + (size_t)(k0 + s) * 3 * (size_t)n : nullptr;
        sl[s].qdot = on ? qdot_all + (c * (size_t)kv + (size_t)(k0 + s)) * (size_t)n : nullptr;
        sl[s].cd = 0; sl[s].sd = 0;
    }
    double cs = 0, ss = 0;
    for (int i = 0; i < n; i++) {
        const double2 e = phase(row + (size_t)i * KS, 1, KX, KY, nx, ny, nz);
        const double qi = q[i];
        cs += qi * e.x;
        ss += qi * e.y;
#pragma unroll
        for (int s = 0; s < kBphKD; s++)
            if (sl[s].vel) sfac_slot(sl[s], i, qi, e, kx, ky, kz);
    }
    const double k2 = kx * kx + ky * ky + kz * kz;
    const double eak = exp(-k2 * 0.25 * one_a2) / k2;
    const double cst = 4.0 / L.x / L.y / L.z * kPi * ke;   // RCK:517
    if (k0 == 0) coef_all[c * (size_t)khalf + k] = make_double2(2.0 * cst * eak * cs, 2.0 * cst * eak * ss);
#pragma unroll
    for (int s = 0; s < kBphKD; s++)
        if (sl[s].vel)
            coefd_all[(c * (size_t)kv + (size_t)(k0 + s)) * (size_t)khalf + k] =
                make_double2(2.0 * cst * eak * sl[s].cd, 2.0 * cst * eak * sl[s].sd);
}

// ---------------------------------------------------------------------------------
// 4. direct space, the block shape of k_bp_pairs: kBphI = 64 i-atoms of one conformation, one per
//    lane, in each of the four waves; the j-atoms pass through LDS in tiles of 256 -- (x, y, z, q),
//    the LJ pair and, per direction of the chunk, (v, qdot) -- and wave w takes entries
//    [64 w, 64 w + 64) of every tile.  Per pair, ONCE: delta_r minimum image, the excluded test, the
//    erf pair at any distance or the erfc pair (erfc_exp, the handle's erfcx table in LDS) within
//    the cutoff, the LJ term, and from them s and the three coefficients of sdot.  Then per direction
//    (pair_slot): d.w, sdot, and its sums of D_v F^pair and gdot.  The four waves' partial sums are
//    added as (w0 + w1) + (w2 + w3), then the self terms.  Writes -D_v F^pair to out (overwriting it)
//    and the pair part of gdot per direction, the pair part of g from the conformation's chunk 0.
//    LDS: table 8256 B + (x, q) tile 8192 B + LJ tile 4096 B + kBphKD (v, qdot) tiles of 8192 B =
//    52.1 KiB with 4 directions; the partial sums of waves 1..3 (3 x 17 x 512 B) reuse the direction
//    tiles after the j loop.  k_bp_pairs holds 29.1 KiB: by LDS 3 blocks of this kernel fit a CU's
//    160 KiB where 5 of the forward kernel do (12 waves against 20) -- the price of 4 directions per
//    block; the block carries ~50 fp64 values per lane and is bound by registers before that.
// ---------------------------------------------------------------------------------
constexpr int kBphI = 64;
constexpr int kBphJ = 256;

struct PairSlot {
    double vx, vy, vz, qd;      // atom i's direction and charge tangent
    double hx, hy, hz, gd;      // sums: D_v F^pair, gdot
};

// one pair for one direction: d the minimum image, s the pair's force factor, c1 (d.w) + c2 qdot_i +
// c3 qdot_j its tangent, gp = ke P / r, gq = ke Q q_j / r^3
__device__ __forceinline__ void pair_slot(PairSlot& a, double4 vj, double3 d, double s, double c1, double c2, double c3,
                                          double gp, double gq) {
    const double wx = a.vx - vj.x, wy = a.vy - vj.y, wz = a.vz - vj.z;
    const double dw = d.x * wx + d.y * wy + d.z * wz;
    const double sd = c1 * dw + (c2 * a.qd + c3 * vj.w);
    a.hx += sd * d.x + s * wx;
    a.hy += sd * d.y + s * wy;
    a.hz += sd * d.z + s * wz;
    a.gd += gp * vj.w - gq * dw;
}

__global__ void __launch_bounds__(kBphJ) k_bph_pairs(int n, int kv, int nchunk, double ke, double alpha, double rc2,
                                                     double erfc_scale, const double* __restrict__ erfc_tab,
                                                     const double* __restrict__ boxes,
                                                     const double* __restrict__ pos_all, const double* __restrict__ q_all,
                                                     const double* __restrict__ vec_all, long vstride,
                                                     const double* __restrict__ qdot_all, const double2* __restrict__ lj,
                                                     const int* __restrict__ ex_start, const int* __restrict__ ex_list,
                                                     double* __restrict__ g_all, double* __restrict__ gdot_all,
                                                     double* __restrict__ out_all) {
    constexpr int kAcc = 1 + 4 * kBphKD;   // g, then (hx, hy, hz, gd) per direction
    __shared__ double tab[kErfcMaxM * (kErfcDeg + 1)];
    __shared__ double4 sp[kBphJ];
    __shared__ double2 sl[kBphJ];
    __shared__ double4 sv[kBphKD][kBphJ];
    static_assert(sizeof(double4) * kBphKD * kBphJ >= sizeof(double) * 3 * kAcc * kBphI,
                  "the partial sums reuse the direction tiles");
    for (int e = threadIdx.x; e < kErfcMaxM * (kErfcDeg + 1); e += kBphJ) tab[e] = erfc_tab[e];
    const size_t c = blockIdx.y / (unsigned)nchunk;
    const int k0 = (int)(blockIdx.y % (unsigned)nchunk) * kBphKD;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    const double* vel[kBphKD];
    const double* qdot[kBphKD];
#pragma unroll
    for (int s = 0; s < kBphKD; s++) {
        const bool on = k0 + s < kv;
        vel[s] = on ? vec_all + c * (size_t)vstride + (size_t)(k0 + s) * 3 * (size_t)n : nullptr;
        qdot[s] = on ? qdot_all + (c * (size_t)kv + (size_t)(k0 + s)) * (size_t)n : nullptr;
    }
    double3 L, T;
    load_box(boxes, c, L, T);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kBphI + lane;
    const bool active = i < n;
    double3 xi = make_double3(0, 0, 0);
    double qi = 0;
    double2 li = make_double2(0, 0);
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    PairSlot acc[kBphKD];
#pragma unroll
    for (int s = 0; s < kBphKD; s++) acc[s] = PairSlot{0, 0, 0, 0, 0, 0, 0, 0};
    if (active) {
        xi = ld3(pos, i);
        qi = q[i];
        li = lj[i];
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
#pragma unroll
        for (int s = 0; s < kBphKD; s++)
            if (vel[s]) { acc[s].vx = vel[s][3 * i]; acc[s].vy = vel[s][3 * i + 1]; acc[s].vz = vel[s][3 * i + 2]; acc[s].qd = qdot[s][i]; }
    }
#pragma unroll
    for (int m = 0; m < kMaxRegExcl; m++) reg[m] = m < exc ? ex_list[ex0 + m] : -1;
    const double two_over_sqrtpi = 1.1283791670955126;
    double g = 0;
    for (int base = 0; base < n; base += kBphJ) {
        const int j = base + threadIdx.x;
        __syncthreads();   // (first tile: the erfcx table is staged)
        if (j < n) {
            sp[threadIdx.x] = make_double4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], q[j]);
            sl[threadIdx.x] = lj[j];
#pragma unroll
            for (int s = 0; s < kBphKD; s++)
                sv[s][threadIdx.x] = vel[s] ? make_double4(vel[s][3 * j], vel[s][3 * j + 1], vel[s][3 * j + 2], qdot[s][j])
                                            : make_double4(0, 0, 0, 0);
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
            // p = P, dp = Q, x3 = 2 c (alpha r)^3 e^{-alpha^2 r^2}; lja = A, ljd = e4 s6 (48 - 168 s6)
            double p, dp, x3, inv_r, lja = 0, ljd = 0;
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
                const double2 lj2 = sl[t];
                const double sig = li.x + lj2.x;
                double s2 = inv_r * sig; s2 *= s2;
                const double sig6 = s2 * s2 * s2;
                const double es6 = sig6 * li.y * lj2.y;
                lja = es6 * (12 * sig6 - 6);
                ljd = es6 * (48 - 168 * sig6);
            }
            const double inv_r2 = inv_r * inv_r;
            const double kr = ke * inv_r;
            const double cq = kr * qi * pj.w;                        // C
            const double s = (lja + cq * dp) * inv_r2;
            const double c1 = (ljd - cq * (3 * dp + x3)) * inv_r2 * inv_r2;
            const double kq = kr * dp * inv_r2;
            const double c2 = kq * pj.w, c3 = kq * qi;
            const double gp = kr * p, gq = kr * dp * pj.w * inv_r2;
            g += gp * pj.w;
#pragma unroll
            for (int sI = 0; sI < kBphKD; sI++) pair_slot(acc[sI], sv[sI][t], d, s, c1, c2, c3, gp, gq);
        }
    }
    __syncthreads();   // every wave is done with the direction tiles: the partial sums take their place
    double* red = reinterpret_cast<double*>(&sv[0][0]);   // [3][kAcc][64]
    if (w > 0) {
        double* r = red + (size_t)(w - 1) * kAcc * kBphI + lane;
        r[0] = g;
#pragma unroll
        for (int s = 0; s < kBphKD; s++) {
            r[(1 + 4 * s) * kBphI] = acc[s].hx; r[(2 + 4 * s) * kBphI] = acc[s].hy;
            r[(3 + 4 * s) * kBphI] = acc[s].hz; r[(4 + 4 * s) * kBphI] = acc[s].gd;
        }
    }
    __syncthreads();
    if (w > 0 || !active) return;
    const double* r0 = red + lane;
    const double* r1 = r0 + kAcc * kBphI;
    const double* r2 = r1 + kAcc * kBphI;
    auto tot = [&](double a, int m) { return (a + r0[m * kBphI]) + (r1[m * kBphI] + r2[m * kBphI]); };
    const double cself = ke * alpha / sqrt(kPi);   // RCK:507-510
    if (k0 == 0) g_all[c * (size_t)n + i] = -2 * cself * qi + tot(g, 0);
#pragma unroll
    for (int s = 0; s < kBphKD; s++) {
        if (!vel[s]) continue;
        const size_t cv = c * (size_t)kv + (size_t)(k0 + s);
        gdot_all[cv * (size_t)n + i] = -2 * cself * acc[s].qd + tot(acc[s].gd, 4 + 4 * s);
        double* o = out_all + c * (size_t)vstride + (size_t)(k0 + s) * 3 * (size_t)n + 3 * (size_t)i;
        o[0] = -tot(acc[s].hx, 1 + 4 * s);
        o[1] = -tot(acc[s].hy, 2 + 4 * s);
        o[2] = -tot(acc[s].hz, 3 + 4 * s);
    }
}

// ---------------------------------------------------------------------------------
// 5. reciprocal part, the shape of k_bpg_recip: 64 atoms per block, one per lane, in each of the
//    four waves; the k-vectors pass through LDS in tiles of 256 (A = 2 c_k S, the chunk's
//    B = 2 c_k Sdot per direction, the integer triple) and wave w takes entries [64 w, 64 w + 64) of
//    every tile; the phase from the entry-major table, ONCE per (atom, k), with
//    G = A.x e.y - A.y e.x and R = A.x e.x + A.y e.y.  g += R and sum_k n G once; per direction
//    (recip_slot): gdot += Re[conj(e) B] - kappa G and sum_k n (B.x e.y - B.y e.x + kappa R).
//    The partial sums are added as (w0 + w1) + (w2 + w3).  Epilogue, this lane's own atom: the
//    conformation's chunk 0 completes g; every direction completes gdot and subtracts
//    D_v F^recip = (2 pi / L) (qdot_i sum n G + q_i sum n (...)) from out.
//    LDS: A 4 KiB + B 4 KiB per direction + triples 4 KiB + partial sums 3 x (4 + 4 kBphKD) x 512 B
//    = 54 KiB with 4 directions.
// ---------------------------------------------------------------------------------
struct RecipSlot {
    double wx, wy, wz;          // v_i (2 pi / L): kappa_i = n . w
    double gd, dx, dy, dz;      // sums
};

__device__ __forceinline__ void recip_slot(RecipSlot& a, double2 cd, double2 e, int4 nn, double G, double R) {
    const double kap = nn.x * a.wx + nn.y * a.wy + nn.z * a.wz;
    a.gd += (cd.x * e.x + cd.y * e.y) - kap * G;
    const double dg = (cd.x * e.y - cd.y * e.x) + kap * R;
    a.dx += dg * nn.x; a.dy += dg * nn.y; a.dz += dg * nn.z;
}

__global__ void __launch_bounds__(256) k_bph_recip(int n, int kv, int nchunk, int KX, int KY, int KZ, long khalf,
                                                   const double* __restrict__ boxes, const double* __restrict__ q_all,
                                                   const double* __restrict__ vec_all, long vstride,
                                                   const double* __restrict__ qdot_all,
                                                   const double2* __restrict__ tab_t_all,
                                                   const double2* __restrict__ coef_all,
                                                   const double2* __restrict__ coefd_all, double* __restrict__ g_all,
                                                   double* __restrict__ gdot_all, double* __restrict__ out_all) {
    constexpr int kAcc = 4 + 4 * kBphKD;   // g, sum n G (3), then (gd, dx, dy, dz) per direction
    __shared__ double2 sc[256];
    __shared__ double2 sd[kBphKD][256];
    __shared__ int4 sn[256];
    __shared__ double red[3][kAcc][64];
    const size_t c = blockIdx.y / (unsigned)nchunk;
    const int k0 = (int)(blockIdx.y % (unsigned)nchunk) * kBphKD;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const bool active = i < n;
    const int KS = KX + KY + KZ;
    const double2* row = tab_t_all + c * (size_t)n * KS + (active ? i : 0);   // entry m at row[m * n]
    const double2* coef = coef_all + c * (size_t)khalf;
    const double2* coefd[kBphKD];
    double3 L, T;
    load_box(boxes, c, L, T);
    const double fx = 2.0 * kPi / L.x, fy = 2.0 * kPi / L.y, fz = 2.0 * kPi / L.z;
    RecipSlot acc[kBphKD];
#pragma unroll
    for (int s = 0; s < kBphKD; s++) {
        const bool on = k0 + s < kv;
        coefd[s] = on ? coefd_all + (c * (size_t)kv + (size_t)(k0 + s)) * (size_t)khalf : nullptr;
        acc[s] = RecipSlot{0, 0, 0, 0, 0, 0, 0};
        if (on && active) {
            const double* vi = vec_all + c * (size_t)vstride + (size_t)(k0 + s) * 3 * (size_t)n + 3 * (size_t)i;
            acc[s].wx = vi[0] * fx; acc[s].wy = vi[1] * fy; acc[s].wz = vi[2] * fz;
        }
    }
    double t0 = 0, gx = 0, gy = 0, gz = 0;
    for (long base = 0; base < khalf; base += 256) {
        const long k = base + threadIdx.x;
        __syncthreads();
        if (k < khalf) {
            int nx, ny, nz;
            half_space_k(k, KY, KZ, nx, ny, nz);
            sc[threadIdx.x] = coef[k];
#pragma unroll
            for (int s = 0; s < kBphKD; s++) sd[s][threadIdx.x] = coefd[s] ? coefd[s][k] : make_double2(0, 0);
            sn[threadIdx.x] = make_int4(nx, ny, nz, 0);
        }
        __syncthreads();
        const int t1 = (int)min((long)(64 * w + 64), khalf - base);
        if (!active) continue;
        for (int t = 64 * w; t < t1; t++) {
            const double2 ab = sc[t];
            const int4 nn = sn[t];
            const double2 e = phase(row, (size_t)n, KX, KY, nn.x, nn.y, nn.z);
            const double R = ab.x * e.x + ab.y * e.y;
            const double G = ab.x * e.y - ab.y * e.x;
            t0 += R;
            gx += G * nn.x; gy += G * nn.y; gz += G * nn.z;
#pragma unroll
            for (int s = 0; s < kBphKD; s++) recip_slot(acc[s], sd[s][t], e, nn, G, R);
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = t0; red[w - 1][1][lane] = gx; red[w - 1][2][lane] = gy; red[w - 1][3][lane] = gz;
#pragma unroll
        for (int s = 0; s < kBphKD; s++) {
            red[w - 1][4 + 4 * s][lane] = acc[s].gd; red[w - 1][5 + 4 * s][lane] = acc[s].dx;
            red[w - 1][6 + 4 * s][lane] = acc[s].dy; red[w - 1][7 + 4 * s][lane] = acc[s].dz;
        }
    }
    __syncthreads();
    if (w > 0 || !active) return;
    auto tot = [&](double a, int m) { return (a + red[0][m][lane]) + (red[1][m][lane] + red[2][m][lane]); };
    const size_t at = c * (size_t)n + i;
    if (k0 == 0) g_all[at] += tot(t0, 0);   // no other chunk reads or writes g here
    gx = tot(gx, 1); gy = tot(gy, 2); gz = tot(gz, 3);
    const double qi = q_all[at];
#pragma unroll
    for (int s = 0; s < kBphKD; s++) {
        if (!coefd[s]) continue;
        const size_t cv = c * (size_t)kv + (size_t)(k0 + s);
        const double qd = qdot_all[cv * (size_t)n + i];
        gdot_all[cv * (size_t)n + i] += tot(acc[s].gd, 4 + 4 * s);
        double* o = out_all + c * (size_t)vstride + (size_t)(k0 + s) * 3 * (size_t)n + 3 * (size_t)i;
        o[0] -= (qd * gx + qi * tot(acc[s].dx, 5 + 4 * s)) * fx;
        o[1] -= (qd * gy + qi * tot(acc[s].dy, 6 + 4 * s)) * fy;
        o[2] -= (qd * gz + qi * tot(acc[s].dz, 7 + 4 * s)) * fz;
    }
}

// ---------------------------------------------------------------------------------
// 6. chain rule: k_bh_chain with the periodic D and Ddot and the conformation's g.  One lane per
//    (row, atom b): out_b += sum_e (gdot[a_e] D_e + g[a_e] Ddot_e) over the ccsr entries of b in entry
//    order, batches of 4 entries in flight.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bph_chain(int n, int kv, long nd3, const int* __restrict__ cs,
                                                   const int2* __restrict__ ce, const double* __restrict__ g_all,
                                                   const double* __restrict__ gdot_all,
                                                   const double* __restrict__ dqdx_all,
                                                   const double* __restrict__ ddot_all, long vstride,
                                                   double* __restrict__ out_all) {
    const size_t cv = blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const size_t c = cv / (size_t)kv, k = cv % (size_t)kv;
    const double* gw = g_all + c * (size_t)n;
    const double* gdw = gdot_all + cv * (size_t)n;
    const double* dqdx = dqdx_all + c * (size_t)nd3;
    const double* ddot = ddot_all + cv * (size_t)nd3;
    double* o = out_all + c * (size_t)vstride + k * 3 * (size_t)n + 3 * (size_t)b;
    double hx = o[0], hy = o[1], hz = o[2];
    const int k1 = cs[b + 1];
    for (int k0 = cs[b]; k0 < k1; k0 += 4) {
        int2 en[4];
#pragma unroll
        for (int u = 0; u < 4; u++) en[u] = ce[min(k0 + u, k1 - 1)];
        double g[4], gd[4], d[4][3], dd[4][3];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            g[u] = gw[en[u].y]; gd[u] = gdw[en[u].y];
#pragma unroll
            for (int j = 0; j < 3; j++) { d[u][j] = dqdx[3 * en[u].x + j]; dd[u][j] = ddot[3 * en[u].x + j]; }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (k0 + u < k1) {
                hx += gd[u] * d[u][0] + g[u] * dd[u][0];
                hy += gd[u] * d[u][1] + g[u] * dd[u][1];
                hz += gd[u] * d[u][2] + g[u] * dd[u][2];
            }
        }
    }
    o[0] = hx; o[1] = hy; o[2] = hz;
}

// ---------------------------------------------------------------------------------
// launcher: one pass of nconf <= w.cap conformations x kv directions, nconf * kv <= hw.cap rows, at
// most nine launches
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

int batch_pbc_hvp_chunk() { return kBphKD; }

size_t batch_pbc_hvp_doubles_per_row(const Handle& h) {
    // coefd [khalf] x 2, slot tangents, Ddot, qdot[N], gdot[N], and g[N] (used per conformation: a pass
    // has no more conformations than rows)
    return 2 * (size_t)h.khalf + (size_t)h.nslots_dq + 3 * (size_t)h.nd + 3 * (size_t)h.n;
}

void batch_pbc_hvp_carve(const Handle& h, double* base, int cap, BatchPbcHvpWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n;
    w.base = base; w.cap = cap;
    w.coefd = reinterpret_cast<double2*>(base);
    w.dslot = reinterpret_cast<double*>(w.coefd + c * (size_t)h.khalf);
    w.ddot = w.dslot + c * (size_t)h.nslots_dq;
    w.qdot = w.ddot + c * 3 * (size_t)h.nd;
    w.gdot = w.qdot + c * n;
    w.g = w.gdot + c * n;
}

void launch_batch_pbc_hvp(Handle& h, const BatchPbcWs& w, const BatchPbcHvpWs& hw, int nconf, int kv, const double* pos,
                          const double* boxes, const double* vec, long vstride, double* out) {
    const int64_t rows64 = (int64_t)nconf * kv;
    if (nconf <= 0 || kv <= 0 || nconf > w.cap || rows64 > hw.cap || rows64 > kBatchMaxPass)
        throw std::invalid_argument("launch_batch_pbc_hvp: pass size");
    const int n = h.n, rows = (int)rows64;
    const int nchunk = (kv + kBphKD - 1) / kBphKD;
    const int KX = h.kmax[0], KY = h.kmax[1], KZ = h.kmax[2];
    const long khalf = (long)h.khalf, nd3 = 3L * h.nd;
    launch_batch_pbc_flux_charges(h, w, nconf, pos, boxes, nullptr);
    launch_batch_pbc_tables(h, w, nconf, pos, boxes);
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bph_terms, dim3(nblk((int64_t)rows * h.nterms, 256)), dim3(256), 0, h.stream, rows, kv, n,
                           h.nterms, h.nb, h.na, h.nslots_dq, nd3, h.term_idx, h.term_par, pos, boxes, vec, vstride,
                           hw.dslot, hw.ddot);
    hipLaunchKernelGGL(k_bph_qdot, dim3(nblk(n, 256), rows), dim3(256), 0, h.stream, n, h.nslots_dq, h.qcsr_start,
                       h.qcsr_slot, hw.dslot, hw.qdot);
    const dim3 kgrid(nblk(khalf, 256), nconf * nchunk), agrid(nblk(n, kBphI), nconf * nchunk);
    hipLaunchKernelGGL(k_bph_sfac, kgrid, dim3(256), 0, h.stream, n, kv, nchunk, KX, KY, KZ, khalf, h.ke,
                       1.0 / (h.alpha * h.alpha), boxes, w.q, vec, vstride, hw.qdot, w.tab, w.coef, hw.coefd);
    hipLaunchKernelGGL(k_bph_pairs, agrid, dim3(kBphJ), 0, h.stream, n, kv, nchunk, h.ke, h.alpha, h.cutoff * h.cutoff,
                       h.erfc_scale, h.erfc_tab, boxes, pos, w.q, vec, vstride, hw.qdot, h.lj, h.ex_start, h.ex_list,
                       hw.g, hw.gdot, out);
    hipLaunchKernelGGL(k_bph_recip, agrid, dim3(256), 0, h.stream, n, kv, nchunk, KX, KY, KZ, khalf, boxes, w.q, vec,
                       vstride, hw.qdot, w.tab_t, w.coef, hw.coefd, hw.g, hw.gdot, out);
    hipLaunchKernelGGL(k_bph_chain, dim3(nblk(n, 256), rows), dim3(256), 0, h.stream, n, kv, nd3, h.ccsr_start,
                       h.ccsr_ent, hw.g, hw.gdot, w.dqdx, hw.ddot, vstride, out);
}

}  // namespace cf
