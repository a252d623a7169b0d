// cf_kernels_batch_pbc_virial.hip -- cf_compute_batch_periodic_virial: the virial tensor of every
// frame of the periodic batch (cf_kernels_batch_pbc.hip) beside its energies, forces and charges
// ("batched, periodic, virial").  Per conformation x and ORTHORHOMBIC box h, with E
// the energy of cf_compute_batch_periodic and the strain x -> x (I + eps), h -> h (I + eps) at fixed
// alpha, kmax, cutoff, pair set and image of every pair:
//     Xi = -dE/d eps = Xi^pair + Xi^recip + Xi^flux
//     Xi^pair  = 1/2 sum_i sum_{j != i} s_ij d (x) d        d = minimum image of x_i - x_j, F_i = sum_j s_ij d
//     Xi^recip = sum_k ek_k [1 - 2 k (x) k (1 / k^2 + 1 / (4 alpha^2))]   (k . x is invariant, V -> V (1 + tr eps),
//                                                           d k^2 / d eps_ab = -2 k_a k_b; ek: k_bp_sfac's)
//     Xi^flux  = -sum_terms sum_b r_b (x) w_b,  w_b = sum_a g_a dq_a/dx_b   (g = the complete dE/dq, r_b the term's
//                                                           minimum image of x_b - x_anchor, dq_a/dx_b: k_bp_flux's)
// The self term depends on the strain through the charges only (g).  Each part is symmetric: six sums
// (xx, xy, xz, yy, yz, zz) are carried and mirrored into the 3 x 3 output.
//
// A pass: k_bp_flux, k_b_charges, k_bp_tables, k_bp_sfac (as they are), k_bpv_pairs (k_bp_pairs with
// the six sums in the same sweep), k_bp_recip, k_bp_assemble (as they are), k_bpv_flux, k_bpv_close:
// at most nine launches.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N, the topology and kmax: a frame's
// tensor is bitwise the same alone, at any position of any batch and under any pass size.  Every
// index is topological (validated by cf_create) or derived from blockIdx / threadIdx against n,
// nterms, khalf and the launch's own counts: no device guard bits.
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

struct VirAcc {
    double xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
};

// v += s d (x) d (upper triangle).  The products s d are formed on their own and every sum is an
// explicit fma, so the pair's force sums beside it keep k_bp_pairs' operations
__device__ __forceinline__ void vir_pair(VirAcc& v, double s, double3 d) {
    const double sx = s * d.x, sy = s * d.y, sz = s * d.z;
    v.xx = fma(sx, d.x, v.xx); v.xy = fma(sx, d.y, v.xy); v.xz = fma(sx, d.z, v.xz);
    v.yy = fma(sy, d.y, v.yy); v.yz = fma(sy, d.z, v.yz);
    v.zz = fma(sz, d.z, v.zz);
}

// v -= r (x) w (upper triangle)
__device__ __forceinline__ void vir_flux(VirAcc& v, double3 r, double3 w) {
    v.xx -= r.x * w.x; v.xy -= r.x * w.y; v.xz -= r.x * w.z;
    v.yy -= r.y * w.y; v.yz -= r.y * w.z;
    v.zz -= r.z * w.z;
}

// the six sums over the 64 lanes of a wave: a butterfly, the same order in every lane
__device__ __forceinline__ void vir_wave_sum(double (&v)[6]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] += __shfl_xor(v[k], m);
    }
}

// the six sums over the 256 threads of a block: the butterfly, then the waves as (w0 + w1) + (w2 + w3);
// threads 0..5 return component threadIdx.x.  red: 24 doubles of LDS
__device__ __forceinline__ double vir_block_sum(const VirAcc& a, double (*red)[6]) {
    double v[6] = {a.xx, a.xy, a.xz, a.yy, a.yz, a.zz};
    vir_wave_sum(v);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    const int k = threadIdx.x < 6 ? threadIdx.x : 0;
    return (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// ---------------------------------------------------------------------------------
// 1. direct space: k_bp_pairs' block -- kPbvI = 64 i-atoms of one conformation, one per lane, in each
//    of the four waves; the j-atoms through LDS in tiles of 256, wave w takes entries [64 w, 64 w + 64)
//    of every tile.  Per pair the force scalar s (ewald_pair's dEdR within the cutoff, -g of
//    CF_EXCL_PAIR for an excluded partner at any distance) also feeds the lane's six tensor sums: one
//    sweep over the pairs.  F, dE/dq and the per-atom energy are k_bp_pairs' to the bit: the same
//    statements in the same blocks, the force sums as the fma the contraction makes of them there.
//    include_forces stays a kernel argument (always 1 here), not a constant: without the branches the
//    compiler contracts sig6 - 1 of the energy term with the product that forms sig6, and the
//    energies lose k_bp_pairs' bits.  The four waves' sums are added as (w0 + w1) + (w2 + w3); then
//    wave 0 adds the tensor sums of its 64 lanes by the butterfly and lane 0 writes half of them (every
//    pair is seen from both atoms): one 6-vector per (conformation, i-block).
//    LDS: table 8256 B + (x, q) tile 8192 B + LJ tile 4096 B + partial sums of waves 1..3
//    3 x 12 x 512 B = 18 432 B.
// ---------------------------------------------------------------------------------
constexpr int kPbvI = 64;
constexpr int kPbvJ = 256;

// ewald_pair (cf_pair.h) statement for statement, the pair's force scalar also into the tensor sums
__device__ __forceinline__ void ewald_pair_v(PairAcc& acc, VirAcc& vir, double ke, double alpha, double erfc_scale,
                                             int include_forces, const double* __restrict__ tab, double qi, double2 li,
                                             double qj_, double2 lj2, double dx, double dy, double dz, double r2) {
    const double two_over_sqrtpi = 1.1283791670955126;
    double inv_r = rsqrt_fp64(r2);
    double r = r2 * inv_r;
    double ar = alpha * r;
    double e2;
    double ec = erfc_exp(ar, tab, erfc_scale, e2);
    const double qj = ke * qj_ * inv_r;
    const double qq = qi * qj;
    double sig = li.x + lj2.x;
    double s2 = inv_r * sig; s2 *= s2;
    const double sig6 = s2 * s2 * s2;
    const double es6 = sig6 * li.y * lj2.y;
    if (include_forces) {
        const double dEdR = fma(qq, ec + ar * e2 * two_over_sqrtpi, es6 * (12 * sig6 - 6)) * (inv_r * inv_r);
        acc.fx = fma(dEdR, dx, acc.fx); acc.fy = fma(dEdR, dy, acc.fy); acc.fz = fma(dEdR, dz, acc.fz);
        acc.dq += qj * ec;
        vir_pair(vir, dEdR, make_double3(dx, dy, dz));
    }
    acc.e += qq * ec + es6 * (sig6 - 1);
}

__global__ void __launch_bounds__(kPbvJ) k_bpv_pairs(int n, int include_forces, double ke, double alpha, double rc2,
                                                     double erfc_scale, const double* __restrict__ erfc_tab,
                                                     const double* __restrict__ boxes,
                                                     const double* __restrict__ pos_all, const double* __restrict__ q_all,
                                                     const double2* __restrict__ lj, const int* __restrict__ ex_start,
                                                     const int* __restrict__ ex_list, double* __restrict__ dedq_all,
                                                     double* __restrict__ f_part_all, double* __restrict__ e_atom_all,
                                                     double* __restrict__ vpart_all) {
    __shared__ double tab[kErfcMaxM * (kErfcDeg + 1)];
    __shared__ double4 sp[kPbvJ];
    __shared__ double2 sl[kPbvJ];
    __shared__ double red[3][12][kPbvI];   // partial sums of waves 1..3
    for (int e = threadIdx.x; e < kErfcMaxM * (kErfcDeg + 1); e += kPbvJ) tab[e] = erfc_tab[e];
    const size_t c = blockIdx.y;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    double3 L, T;
    load_box(boxes, c, L, T);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kPbvI + lane;
    const bool active = i < n;
    double3 xi = make_double3(0, 0, 0);
    double qi = 0;
    double2 li = make_double2(0, 0);
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        xi = ld3(pos, i);
        qi = q[i];
        li = lj[i];
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int k = 0; k < kMaxRegExcl; k++) reg[k] = k < exc ? ex_list[ex0 + k] : -1;
    PairAcc acc;
    VirAcc vir;
    double ex_e = 0;
    for (int base = 0; base < n; base += kPbvJ) {
        const int j = base + threadIdx.x;
        __syncthreads();   // (first tile: the erfcx table is staged)
        if (j < n) {
            sp[threadIdx.x] = make_double4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], q[j]);
            sl[threadIdx.x] = lj[j];
        }
        __syncthreads();
        const int t1 = min(64 * w + 64, n - base);
        if (!active) continue;
        for (int t = 64 * w; t < t1; t++) {
            const int jj = base + t;
            if (jj == i) continue;
            const double4 pj = sp[t];
            const double3 d = delta_r(make_double3(pj.x, pj.y, pj.z), xi, L, 1, T);   // x_i - x_j
            // d.x * d.x + d.y * d.y + d.z * d.z as k_bp_pairs' build contracts it (written out: beside the
            // tensor sums the compiler orders the two inner products the other way, one ulp apart)
            const double r2 = fma(d.z, d.z, fma(d.x, d.x, d.y * d.y));
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) {   // CF_EXCL_PAIR with forces, its g kept
                const double two_over_sqrtpi = 1.1283791670955126;
                double r = sqrt(r2);
                double inv_r = 1.0 / r, ar = alpha * r;
                double ef = erf(ar);
                double qj = pj.w;
                if (include_forces) {
                    double g = ke * qi * qj * inv_r * inv_r * inv_r * (ef - ar * exp(-ar * ar) * two_over_sqrtpi);
                    acc.fx = fma(-g, d.x, acc.fx); acc.fy = fma(-g, d.y, acc.fy); acc.fz = fma(-g, d.z, acc.fz);
                    acc.dq -= ke * qj * inv_r * ef;
                    vir_pair(vir, -g, d);
                }
                ex_e -= 0.5 * ke * qi * qj * inv_r * ef;
                continue;
            }
            if (r2 <= rc2)
                ewald_pair_v(acc, vir, ke, alpha, erfc_scale, include_forces, tab, qi, li, pj.w, sl[t], d.x, d.y, d.z, r2);
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = acc.fx; red[w - 1][1][lane] = acc.fy; red[w - 1][2][lane] = acc.fz;
        red[w - 1][3][lane] = acc.dq; red[w - 1][4][lane] = acc.e; red[w - 1][5][lane] = ex_e;
        red[w - 1][6][lane] = vir.xx; red[w - 1][7][lane] = vir.xy; red[w - 1][8][lane] = vir.xz;
        red[w - 1][9][lane] = vir.yy; red[w - 1][10][lane] = vir.yz; red[w - 1][11][lane] = vir.zz;
    }
    __syncthreads();
    if (w > 0) return;
    auto tot = [&](double a, int m) { return (a + red[0][m][lane]) + (red[1][m][lane] + red[2][m][lane]); };
    if (active) {
        const double cself = ke * alpha / sqrt(kPi);   // RCK:507-510
        const double e = tot(acc.e, 4);
        ex_e = tot(ex_e, 5);
        e_atom_all[c * (size_t)n + i] = (-cself * qi * qi + 0.5 * e) + ex_e;
        if (include_forces) {
            const double fx = tot(acc.fx, 0), fy = tot(acc.fy, 1), fz = tot(acc.fz, 2);
            const double dq = tot(acc.dq, 3);
            dedq_all[c * (size_t)n + i] = -2 * cself * qi + dq;
            double* f = f_part_all + c * 3 * (size_t)n + 3 * (size_t)i;
            f[0] = fx; f[1] = fy; f[2] = fz;
        }
    }
    // an inactive lane's sums are zero in all four waves
    double v[6] = {tot(vir.xx, 6), tot(vir.xy, 7), tot(vir.xz, 8), tot(vir.yy, 9), tot(vir.yz, 10), tot(vir.zz, 11)};
    vir_wave_sum(v);
    if (lane == 0) {
        double* o = vpart_all + (c * (size_t)gridDim.x + blockIdx.x) * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = 0.5 * v[k];
    }
}

// ---------------------------------------------------------------------------------
// 2. charge response, after dE/dq is complete (k_bp_recip): one lane per (conformation, term).  The
//    term's atoms b other than its anchor -- a bond's first atom, an angle's central atom, a water's
//    oxygen -- contribute -r_b (x) w_b: r_b = delta_r from the anchor, the minimum-image vector
//    flux_term itself forms (d of a bond, d21 and d23 of an angle, d12 and d13 of a water), and
//    w_b = sum_a g_a dq_a/dx_b over the term's charges a, entry (a, b) of its dq/dx block at
//    o[3 (A a + b)], A the term's atom count.  (The anchor's own row drops out: the block sums to zero
//    over b.)  The block's 256 lanes are added by vir_block_sum: one 6-vector per (conformation, block).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpv_flux(int n, int nterms, int nb, int na, long nd3,
                                                  const int4* __restrict__ tidx, const double* __restrict__ pos_all,
                                                  const double* __restrict__ boxes,
                                                  const double* __restrict__ dedq_all,
                                                  const double* __restrict__ dqdx_all, double* __restrict__ vpart_all) {
    __shared__ double red[4][6];
    const size_t c = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    VirAcc vir;
    if (t < nterms) {
        const double* pos = pos_all + c * 3 * (size_t)n;
        const double* g = dedq_all + c * (size_t)n;
        const double* o = dqdx_all + c * (size_t)nd3 + dqdx_start(t, nb, na);
        double3 L, T;
        load_box(boxes, c, L, T);
        const int4 ti = tidx[t];
        if (ti.x == 0) {   // bond p1-p2: anchor p1
            const double3 d = delta_r(ld3(pos, ti.y), ld3(pos, ti.z), L, 1, T);
            const double g1 = g[ti.y], g2 = g[ti.z];
            vir_flux(vir, d, make_double3(g1 * o[3] + g2 * o[9], g1 * o[4] + g2 * o[10], g1 * o[5] + g2 * o[11]));
        } else {           // angle p1-p2-p3: anchor p2, others 0 and 2; water O,H1,H2: anchor O, others 1 and 2
            const int anchor = ti.x == 1 ? ti.z : ti.y;
            const int b0 = ti.x == 1 ? 0 : 1;
            const int other = ti.x == 1 ? ti.y : ti.z;
            const double3 xa = ld3(pos, anchor);
            const double3 r0 = delta_r(xa, ld3(pos, other), L, 1, T), r2 = delta_r(xa, ld3(pos, ti.w), L, 1, T);
            const double g1 = g[ti.y], g2 = g[ti.z], g3 = g[ti.w];
            const double* o0 = o + 3 * b0;
            vir_flux(vir, r0, make_double3(g1 * o0[0] + g2 * o0[9] + g3 * o0[18], g1 * o0[1] + g2 * o0[10] + g3 * o0[19],
                                           g1 * o0[2] + g2 * o0[11] + g3 * o0[20]));
            vir_flux(vir, r2, make_double3(g1 * o[6] + g2 * o[15] + g3 * o[24], g1 * o[7] + g2 * o[16] + g3 * o[25],
                                           g1 * o[8] + g2 * o[17] + g3 * o[26]));
        }
    }
    const double s = vir_block_sum(vir, red);
    if (threadIdx.x < 6) vpart_all[(c * (size_t)gridDim.x + blockIdx.x) * 6 + threadIdx.x] = s;
}

// ---------------------------------------------------------------------------------
// 3. closing reduction: one block per conformation.  Thread t adds the reciprocal terms
//    ek_k [delta - 2 k (x) k (1 / k^2 + 1 / (4 alpha^2))] of k-vectors t, t + 256, ... of the half-space set
//    (half_space_k's order, k = 2 pi n / L from the box diagonals), then vir_block_sum; threads 0..5
//    each close one component: the pair kernel's block partials in block order, then the flux
//    kernel's, then the reciprocal sum; written as nine doubles with the mirror.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bpv_close(int nib, int nfb, int KY, int KZ, long khalf, double one_a2,
                                                   const double* __restrict__ boxes, const double* __restrict__ ek_all,
                                                   const double* __restrict__ vpair_all,
                                                   const double* __restrict__ vflux_all, double* __restrict__ virial) {
    __shared__ double red[4][6];
    __shared__ double fin[6];
    const size_t c = blockIdx.x;
    double3 L, T;
    load_box(boxes, c, L, T);
    const double ux = 2.0 * kPi / L.x, uy = 2.0 * kPi / L.y, uz = 2.0 * kPi / L.z;
    const double* ek = ek_all + c * (size_t)khalf;
    VirAcc vir;
    for (long k = threadIdx.x; k < khalf; k += 256) {
        int nx, ny, nz;
        half_space_k(k, KY, KZ, nx, ny, nz);
        const double kx = nx * ux, ky = ny * uy, kz = nz * uz;
        const double k2 = kx * kx + ky * ky + kz * kz;
        const double e = ek[k];
        const double f = -2.0 * e * (1.0 / k2 + 0.25 * one_a2);
        const double fx = f * kx, fy = f * ky, fz = f * kz;
        vir.xx += fma(fx, kx, e); vir.xy += fx * ky; vir.xz += fx * kz;
        vir.yy += fma(fy, ky, e); vir.yz += fy * kz;
        vir.zz += fma(fz, kz, e);
    }
    const double recip = vir_block_sum(vir, red);
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        const double* vp = vpair_all + c * (size_t)nib * 6 + k;
        const double* vf = vflux_all + c * (size_t)nfb * 6 + k;
        double a = 0;
        for (int b = 0; b < nib; b++) a += vp[6 * (size_t)b];
        for (int b = 0; b < nfb; b++) a += vf[6 * (size_t)b];
        fin[k] = a + recip;
    }
    __syncthreads();
    if (threadIdx.x < 9) {   // (xx, xy, xz, yy, yz, zz) -> row-major 3 x 3
        const int row = threadIdx.x / 3, col = threadIdx.x % 3;
        const int a = min(row, col), b = max(row, col);
        virial[c * 9 + threadIdx.x] = fin[a == 0 ? b : (a == 1 ? 2 + b : 5)];
    }
}

// ---------------------------------------------------------------------------------
// launcher: one pass of nconf <= min(w.cap, vw.cap) conformations, at most nine launches
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

size_t batch_pbc_virial_doubles_per_conf(const Handle& h) {
    return 6 * ((size_t)nblk(h.n, kPbvI) + (size_t)nblk(h.nterms, 256));
}

void batch_pbc_virial_carve(const Handle& h, double* base, int cap, BatchPbcVirialWs& w) {
    w.base = base; w.cap = cap;
    w.pair = base;
    w.flux = w.pair + (size_t)cap * 6 * (size_t)nblk(h.n, kPbvI);
}

void launch_batch_pbc_virial(Handle& h, const BatchPbcWs& w, const BatchPbcVirialWs& vw, int nconf, const double* pos,
                             const double* boxes, int flags, double* forces, double* energy, double* charges,
                             double* virial) {
    if (nconf <= 0 || nconf > w.cap || nconf > vw.cap || nconf > kBatchMaxPass)
        throw std::invalid_argument("launch_batch_pbc_virial: pass size");
    const int n = h.n;
    const int nib = nblk(n, kPbvI), nfb = nblk(h.nterms, 256);
    const bool do_f = (flags & CF_INCLUDE_FORCES) && forces;
    const bool do_er = (flags & CF_INCLUDE_ENERGY) && energy;
    // every stage runs whatever the flags (the tensor needs the complete dE/dq and ek); the flags
    // decide what k_bp_assemble writes, as in launch_batch_pbc
    launch_batch_pbc_flux_charges(h, w, nconf, pos, boxes, charges);
    launch_batch_pbc_tables(h, w, nconf, pos, boxes);
    launch_batch_pbc_sfac(h, w, nconf, boxes);
    hipLaunchKernelGGL(k_bpv_pairs, dim3(nib, nconf), dim3(kPbvJ), 0, h.stream, n, 1, h.ke, h.alpha, h.cutoff * h.cutoff,
                       h.erfc_scale, h.erfc_tab, boxes, pos, w.q, h.lj, h.ex_start, h.ex_list, w.dedq, w.f_part, w.e_atom,
                       vw.pair);
    launch_batch_pbc_recip(h, w, nconf, boxes);
    if (do_f || energy) launch_batch_pbc_assemble(h, w, nconf, do_f ? forces : nullptr, energy, do_er ? 1 : 0);
    if (nfb > 0)
        hipLaunchKernelGGL(k_bpv_flux, dim3(nfb, nconf), dim3(256), 0, h.stream, n, h.nterms, h.nb, h.na, 3L * h.nd,
                           h.term_idx, pos, boxes, w.dedq, w.dqdx, vw.flux);
    hipLaunchKernelGGL(k_bpv_close, dim3(nconf), dim3(256), 0, h.stream, nib, nfb, h.kmax[1], h.kmax[2], (long)h.khalf,
                       1.0 / (h.alpha * h.alpha), boxes, w.ek, vw.pair, vw.flux, virial);
}

}  // namespace cf
