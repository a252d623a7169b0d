// cf_flux.h -- the charge-flux term bodies, shared by the single-evaluation kernel k_flux_terms
// (cf_kernels_core.hip) and the batched ones k_b_flux (cf_kernels_batch.hip) and k_bp_flux
// (cf_kernels_batch_pbc.hip), with the other bodies the batched kernels share (the periodic ones and
// their parameter gradients, cf_kernels_batch_pbc_grad.hip: load_box, phase): one definition of the
// reference's formulas (ReferenceCoulKernels.cpp, RCK: bonds :42-80, angles :81-162, waters
// :163-227), so the two paths cannot drift apart.
#pragma once

#include "cf_pair.h"

namespace cf {

// first dq/dx double of term t: bonds (12 doubles each), then angles (27), then waters (27) --
// the terms of a block write one contiguous range
__device__ __forceinline__ long dqdx_start(int t, int nb, int na) {
    const int b = min(t, nb), an = max(0, min(t, nb + na) - nb), w = max(0, t - nb - na);
    return 3L * (4L * b + 9L * an + 9L * w);
}

// term t = (ti.x type; ti.y, ti.z, ti.w atoms) with parameters p[0..5): its charge deltas into
// dq_slot (the term's 2 or 3 slots) and its dq/dx block (12 or 27 doubles, the reference's entry
// order) into o
__device__ __forceinline__ void flux_term(int t, int4 ti, const double* __restrict__ p, int nb, int na,
                                          const double* __restrict__ pos, double3 L, double3 T, int pbc,
                                          double* __restrict__ dq_slot, double* o) {
    if (ti.x == 0) {  // bond p1-p2
        double3 d = delta_r(ld3(pos, ti.y), ld3(pos, ti.z), L, pbc, T);
        double r = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
        double k = p[0], dq = k * (r - p[1]);
        dq_slot[2 * t] = dq;
        dq_slot[2 * t + 1] = -dq;
        double c = k / r;
        double v[3] = {c * d.x, c * d.y, c * d.z};
#pragma unroll
        for (int j = 0; j < 3; j++) { o[j] = -v[j]; o[3 + j] = v[j]; o[6 + j] = v[j]; o[9 + j] = -v[j]; }
    } else if (ti.x == 1) {  // angle p1-p2-p3, p2 central
        int a = t - nb;
        double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        double3 d21 = delta_r(x2, x1, L, pbc, T), d23 = delta_r(x2, x3, L, pbc, T), d13 = delta_r(x1, x3, L, pbc, T);
        double r21_2 = d21.x * d21.x + d21.y * d21.y + d21.z * d21.z;
        double r23_2 = d23.x * d23.x + d23.y * d23.y + d23.z * d23.z;
        double r13_2 = d13.x * d13.x + d13.y * d13.y + d13.z * d13.z;
        double r21 = sqrt(r21_2), r23 = sqrt(r23_2);
        double cost = (r23_2 + r21_2 - r13_2) / 2 / r21 / r23;
        double k = p[0];
        double dq = k * (acos(cost) - p[1]);
        int s = 2 * nb + 3 * a;
        dq_slot[s] = dq; dq_slot[s + 1] = -2 * dq; dq_slot[s + 2] = dq;
        double inv_s = 1 / sqrt(1 - cost * cost);
        double c1 = k * (1.0 / r21 / r23) * inv_s;
        double c21 = k * cost * inv_s / r21_2;
        double c23 = k * cost * inv_s / r23_2;
        double a21[3] = {d21.x, d21.y, d21.z}, a23[3] = {d23.x, d23.y, d23.z};
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double v1 = -c1 * a23[j] + c21 * a21[j];
            double v3 = -c1 * a21[j] + c23 * a23[j];
            double v2 = -v1 - v3;
            o[j] = v1; o[3 + j] = v2; o[6 + j] = v3;
            o[9 + j] = -2 * v1; o[12 + j] = -2 * v2; o[15 + j] = -2 * v3;
            o[18 + j] = v1; o[21 + j] = v2; o[24 + j] = v3;
        }
    } else {  // water O,H1,H2
        int w = t - nb - na;
        double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        double3 d12 = delta_r(x1, x2, L, pbc, T), d13 = delta_r(x1, x3, L, pbc, T), d23 = delta_r(x2, x3, L, pbc, T);
        double r12 = sqrt(d12.x * d12.x + d12.y * d12.y + d12.z * d12.z);
        double r13 = sqrt(d13.x * d13.x + d13.y * d13.y + d13.z * d13.z);
        double r23 = sqrt(d23.x * d23.x + d23.y * d23.y + d23.z * d23.z);
        double k1 = p[0], k2 = p[1], kub = p[2], b0 = p[3], ub0 = p[4];
        double dq2 = k1 * (r12 - b0) + k2 * (r13 - b0) + kub * (r23 - ub0);
        double dq3 = k1 * (r13 - b0) + k2 * (r12 - b0) + kub * (r23 - ub0);
        int s = 2 * nb + 3 * na + 3 * w;
        dq_slot[s] = -dq2 - dq3; dq_slot[s + 1] = dq2; dq_slot[s + 2] = dq3;
        double e12[3] = {d12.x, d12.y, d12.z}, e13[3] = {d13.x, d13.y, d13.z}, e23[3] = {d23.x, d23.y, d23.z};
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double n12 = e12[j] / r12, n13 = e13[j] / r13, n23 = e23[j] / r23;
            double a12k1 = k1 * n12, a12k2 = k2 * n12, a13k1 = k1 * n13, a13k2 = k2 * n13, ub = kub * n23;
            o[0 + j] = a12k1 + a12k2 + a13k1 + a13k2;
            o[3 + j] = -a12k1 - a12k2 + 2 * ub;
            o[6 + j] = -a13k2 - a13k1 - 2 * ub;
            o[9 + j] = -a12k1 - a13k2;
            o[12 + j] = a12k1 - ub;
            o[15 + j] = a13k2 + ub;
            o[18 + j] = -a12k2 - a13k1;
            o[21 + j] = a12k2 - ub;
            o[24 + j] = a13k1 + ub;
        }
    }
}

// ---- bodies shared by the batched kernels (cf_kernels_batch.hip, cf_kernels_batch_pbc.hip) -------
// The (conformation, term) pairs of a batch are flattened, g = c * nterms + t; dq/dx is
// [conformation][D * 3], so a block's output is one contiguous run across conformations.
__device__ __forceinline__ long batch_dqdx_at(long g, int nterms, int nb, int na, long nd3) {
    return (g / nterms) * nd3 + dqdx_start((int)(g % nterms), nb, na);
}

// one block of 256 flattened (conformation, term) pairs: the lane's term into st (LDS, 256 * 27
// doubles), then the block's dq/dx run written coalesced.  PBC: the conformation's box from boxes
// ([conformation][8]: Lx, Ly, Lz, bx, cx, cy, -, -), box-vector minimum image; else no box.
template <bool PBC>
__device__ __forceinline__ void batch_flux_block(int nconf, int n, int nterms, int nb, int na, int nslots, long nd3,
                                                 const int4* __restrict__ tidx, const double* __restrict__ tpar,
                                                 const double* __restrict__ pos_all, const double* __restrict__ boxes,
                                                 int pbc, double* __restrict__ dq_slot_all,
                                                 double* __restrict__ dqdx_all, double* st) {
    const long total = (long)nconf * nterms;
    const long g0 = (long)blockIdx.x * 256;
    const long g = g0 + threadIdx.x;
    const long base = batch_dqdx_at(g0, nterms, nb, na, nd3);
    if (g < total) {
        const size_t c = (size_t)(g / nterms);
        const int t = (int)(g % nterms);
        double3 L = make_double3(0.0, 0.0, 0.0), T = make_double3(0.0, 0.0, 0.0);
        if (PBC) {
            const double* b = boxes + 8 * c;
            L = make_double3(b[0], b[1], b[2]);
            T = make_double3(b[3], b[4], b[5]);
        }
        flux_term(t, tidx[t], tpar + 5 * t, nb, na, pos_all + c * 3 * (size_t)n, L, T, PBC ? pbc : 0,
                  dq_slot_all + c * (size_t)nslots, st + (batch_dqdx_at(g, nterms, nb, na, nd3) - base));
    }
    __syncthreads();
    const int len = (int)(batch_dqdx_at(min(g0 + 256, total), nterms, nb, na, nd3) - base);
    for (int e = threadIdx.x; e < len; e += 256) dqdx_all[base + e] = st[e];
}

// the box of conformation c of a periodic batch: diagonal L and off-diagonals T = (bx, cx, cy)
__device__ __forceinline__ void load_box(const double* __restrict__ boxes, size_t c, double3& L, double3& T) {
    const double* b = boxes + 8 * c;
    L = make_double3(b[0], b[1], b[2]);
    T = make_double3(b[3], b[4], b[5]);
}

// e^{i k.r} of one atom from its table entries row[m * stride] (stride 1: the atom-major table,
// stride N: the entry-major one): X[nx] Y[|ny|]^(sign) Z[|nz|]^(sign) (nx >= 0)
__device__ __forceinline__ double2 phase(const double2* __restrict__ row, size_t stride, int KX, int KY, int nx,
                                         int ny, int nz) {
    const double2 X = row[nx * stride];
    double2 Y = row[(KX + abs(ny)) * stride];
    double2 Z = row[(KX + KY + abs(nz)) * stride];
    if (ny < 0) Y.y = -Y.y;
    if (nz < 0) Z.y = -Z.y;
    const double ar = X.x * Y.x - X.y * Y.y, ai = X.x * Y.y + X.y * Y.x;
    return make_double2(ar * Z.x - ai * Z.y, ar * Z.y + ai * Z.x);
}

// chain rule of atom b: (fx, fy, fz) -= sum_e dE/dq[a_e] dq_{a_e}/dx_b over the ccsr entries of b
// in entry order (k_assemble_energy's gather), batches of 4 entries in flight
__device__ __forceinline__ void chain_rule_atom(int b, const int* __restrict__ cs, const int2* __restrict__ ce,
                                                const double* __restrict__ dedq, const double* __restrict__ dqdx,
                                                double& fx, double& fy, double& fz) {
    const int k1 = cs[b + 1];
    for (int k0 = cs[b]; k0 < k1; k0 += 4) {   // batches of 4 entries in flight, summed in entry order
        int2 en[4];
#pragma unroll
        for (int u = 0; u < 4; u++) en[u] = ce[min(k0 + u, k1 - 1)];
        double g[4], d[4][3];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            g[u] = dedq[en[u].y];
            d[u][0] = dqdx[3 * en[u].x]; d[u][1] = dqdx[3 * en[u].x + 1]; d[u][2] = dqdx[3 * en[u].x + 2];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (k0 + u < k1) {
                fx -= g[u] * d[u][0];
                fy -= g[u] * d[u][1];
                fz -= g[u] * d[u][2];
            }
        }
    }
}

// sum of a over the 256 threads of a block, in a fixed order: a butterfly within each wave, then
// the four waves as (w0 + w1) + (w2 + w3), stored to *out by thread 0.  red: 4 doubles of LDS.
__device__ __forceinline__ void block_sum_256_store(double a, double* red, double* out) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

// true if j is one of the cnt exclusion partners ex_list[ex0, ex0 + cnt), the first kMaxRegExcl of
// which the caller holds in reg
__device__ __forceinline__ bool in_excl(int j, const int* reg, int cnt, const int* ex_list, int ex0) {
    int m = cnt < kMaxRegExcl ? cnt : kMaxRegExcl;
#pragma unroll
    for (int k = 0; k < kMaxRegExcl; k++)
        if (k < m && reg[k] == j) return true;
    for (int k = kMaxRegExcl; k < cnt; k++)
        if (ex_list[ex0 + k] == j) return true;
    return false;
}

// one non-periodic pair (RCK:436-491) seen from atom i: d = x_j - x_i (getDeltaR(i, j)), charges
// qi, qj, LJ (sigma/2, 2 sqrt eps) li, lj.  Adds half the pair energy to e, and with forces the
// force on i to (fx, fy, fz) and ke q_j / r to dq (dE/dq_i).
__device__ __forceinline__ void nopbc_pair(double dx, double dy, double dz, double qi, double qj, double2 li, double2 lj,
                                           double ke, int include_forces, int include_energy, double& fx, double& fy,
                                           double& fz, double& dq, double& e) {
    double inv_r = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
    double sig = li.x + lj.x;
    double s2 = inv_r * sig; s2 *= s2;
    double sig6 = s2 * s2 * s2;
    double es6 = sig6 * li.y * lj.y;
    double qq = ke * qi * qj * inv_r;
    if (include_energy) e += 0.5 * (qq + es6 * (sig6 - 1));
    if (include_forces) {
        double dEdR = (es6 * (12 * sig6 - 6) + qq) * inv_r * inv_r;
        fx -= dEdR * dx; fy -= dEdR * dy; fz -= dEdR * dz;
        dq += ke * qj * inv_r;
    }
}

}  // namespace cf
