// cf_kernels_batch_dipole.hip -- cf_compute_batch_dipole and cf_compute_batch_dipole_vjp: dipoles and
// atomic polar tensors (APT) of the conformations of a non-periodic batch, and their reverse-mode
// product with respect to the base charges and the flux parameters ("batched,
// dipoles and polar tensors").  Per conformation, with q the charges after flux (k_b_charges: the
// bits of cf_compute_batch),
//     mu_al        = sum_a q_a x_a,al                                          (e nm, about the origin)
//     P[b][al][be] = d mu_al / d x_b,be = q_b delta_al,be + sum_a x_a,al dq_a/dx_b,be       (e)
// the sum over atom b's entries of the chain-rule CSR, in entry order: chain_rule_atom's gather with
// x_a in the place of dE/dq_a.  A forward pass is k_b_flux, k_b_charges (as they are), then k_bd_apt.
//
// The VJP differentiates L = mu_bar . mu + sum_b P_bar_b : P_b.  Every flux term is a sum of pieces
// q_a += c_a k (g(x) - ref) over the term's atoms; with a_i = mu_bar . x_i + tr P_bar_i and
// w = sum_a c_a x_a,
//     dL/d(base charge i) = a_i
//     dL/dk   += (sum_a c_a a_a) (g - ref) + sum_b w^T P_bar_b grad_b g
//     dL/dref += -k sum_a c_a a_a
// Nothing divides by a parameter (k = 0 is legal), there is no pair sum and no workspace: k_bd_base
// and k_bd_terms, both from the positions alone.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N and the topology: a
// conformation's results are bitwise the same alone, in any batch and under any chunking.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms and the launch's own nconf: no device guard bits.
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

// ---------------------------------------------------------------------------------
// 1. polar tensors and dipoles: one lane per (conformation, atom b).  The lane's 9 doubles go to
//    LDS at 9 * lane (18 dwords apart: the 16 lanes a 64-bit LDS store is served in cover the 32
//    store banks once, no conflict; the read-back is consecutive doubles), then the block's
//    contiguous run of 9 * min(256, n - b0) doubles is written coalesced, as batch_flux_block writes
//    dq/dx -- a lane storing its own tensor would write 8 bytes at a stride of 72.  Block 0 of every conformation also sums the three dipole
//    components in k_b_assemble's order: thread t adds atoms t, t + 256, ..., then
//    block_sum_256_store per component, each with its own four doubles of LDS.
//    LDS: 256 * 9 * 8 = 18432 B + 96 B.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bd_apt(int n, long nd3, const int* __restrict__ cs,
                                                const int2* __restrict__ ce, const double* __restrict__ pos_all,
                                                const double* __restrict__ q_all,
                                                const double* __restrict__ dqdx_all, double* __restrict__ dipole_out,
                                                double* __restrict__ apt_out) {
    __shared__ double st[256 * 9];
    __shared__ double red[3][4];
    const size_t c = blockIdx.y;
    const int b0 = blockIdx.x * 256;
    const int b = b0 + threadIdx.x;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    if (apt_out) {   // block-uniform
        if (b < n) {
            const double* dqdx = dqdx_all + c * (size_t)nd3;
            const double qb = q[b];
            double p[9] = {qb, 0, 0, 0, qb, 0, 0, 0, qb};
            const int k1 = cs[b + 1];
            for (int k0 = cs[b]; k0 < k1; k0 += 4) {   // batches of 4 entries in flight, summed in entry order
                int2 en[4];
#pragma unroll
                for (int u = 0; u < 4; u++) en[u] = ce[min(k0 + u, k1 - 1)];
                double x[4][3], d[4][3];
#pragma unroll
                for (int u = 0; u < 4; u++) {
#pragma unroll
                    for (int j = 0; j < 3; j++) { x[u][j] = pos[3 * en[u].y + j]; d[u][j] = dqdx[3 * en[u].x + j]; }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (k0 + u < k1) {
#pragma unroll
                        for (int al = 0; al < 3; al++)
#pragma unroll
                            for (int be = 0; be < 3; be++) p[3 * al + be] += x[u][al] * d[u][be];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 9; j++) st[9 * threadIdx.x + j] = p[j];
        }
        __syncthreads();
        const int len = 9 * min(256, n - b0);
        double* out = apt_out + 9 * (c * (size_t)n + (size_t)b0);
        for (int e = threadIdx.x; e < len; e += 256) out[e] = st[e];
    }
    if (blockIdx.x != 0 || !dipole_out) return;   // block-uniform
    double mx = 0, my = 0, mz = 0;
    for (int k = threadIdx.x; k < n; k += 256) {
        const double qk = q[k];
        mx += qk * pos[3 * k];
        my += qk * pos[3 * k + 1];
        mz += qk * pos[3 * k + 2];
    }
    block_sum_256_store(mx, red[0], dipole_out + 3 * c);
    block_sum_256_store(my, red[1], dipole_out + 3 * c + 1);
    block_sum_256_store(mz, red[2], dipole_out + 3 * c + 2);
}

// ---------------------------------------------------------------------------------
// the VJP's bodies.  mu_bar: the conformation's 3 doubles or null (= zero); pb: its [N][3][3] or
// null (= zero).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double3 dsub(double3 a, double3 b) { return make_double3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ double ddot(double3 a, double3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// a_i = mu_bar . x_i + tr P_bar_i
__device__ __forceinline__ double adjoint_weight(int i, double3 xi, const double* __restrict__ mu_bar,
                                                 const double* __restrict__ pb) {
    double a = 0;
    if (mu_bar) a = mu_bar[0] * xi.x + mu_bar[1] * xi.y + mu_bar[2] * xi.z;
    if (pb) a += pb[9 * (size_t)i] + pb[9 * (size_t)i + 4] + pb[9 * (size_t)i + 8];
    return a;
}

// w^T P_bar_b u
__device__ __forceinline__ double bilinear(const double* __restrict__ pb, int b, double3 w, double3 u) {
    const double* m = pb + 9 * (size_t)b;
    return w.x * (m[0] * u.x + m[1] * u.y + m[2] * u.z) + w.y * (m[3] * u.x + m[4] * u.y + m[5] * u.z) +
           w.z * (m[6] * u.x + m[7] * u.y + m[8] * u.z);
}

// a distance r_ij and sum_b w^T P_bar_b grad_b r_ij = w^T (P_bar_j - P_bar_i) u, u = (x_j - x_i) / r_ij
__device__ __forceinline__ double distance_piece(const double* __restrict__ pb, int i, int j, double3 xi, double3 xj,
                                                 double3 w, double& r) {
    const double3 d = dsub(xj, xi);
    r = sqrt(ddot(d, d));
    if (!pb) return 0.0;
    const double3 u = make_double3(d.x / r, d.y / r, d.z / r);
    return bilinear(pb, j, w, u) - bilinear(pb, i, w, u);
}

// ---------------------------------------------------------------------------------
// 2. base charges: one lane per (conformation, atom), a_i to grad[c][i]
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bd_base(int n, long np, const double* __restrict__ pos_all,
                                                 const double* __restrict__ mu_bar_all,
                                                 const double* __restrict__ pb_all, double* __restrict__ grad_all) {
    const size_t c = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* pos = pos_all + c * 3 * (size_t)n;
    grad_all[c * (size_t)np + i] = adjoint_weight(i, ld3(pos, i), mu_bar_all ? mu_bar_all + 3 * c : nullptr,
                                                  pb_all ? pb_all + c * 9 * (size_t)n : nullptr);
}

// ---------------------------------------------------------------------------------
// 3. term gradients: one lane per flattened (conformation, term), g = c * nterms + t.  a of the
//    term's two or three atoms again, the term's geometry and its gradients (flux_term's dq/dx
//    block with unit slopes) from the positions, its 2 or 5 gradients into grad[c][N + ...] in the
//    order of the cf_params arrays: bonds (k, b), angles (k, theta0), waters (k1, k2, kub, b0, ub0).
//      bond   c = (1, -1)      g = r12
//      angle  c = (1, -2, 1)   g = theta
//      water  k1: (r12 - b0) with c = (-1, 1, 0) and (r13 - b0) with c = (-1, 0, 1); k2: the two
//             distances exchanged; kub: (r23 - ub0) with c = (-2, 1, 1)
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bd_terms(int nconf, int n, int nterms, int nb, int na, long np,
                                                  const int4* __restrict__ tidx, const double* __restrict__ tpar,
                                                  const double* __restrict__ pos_all,
                                                  const double* __restrict__ mu_bar_all,
                                                  const double* __restrict__ pb_all, double* __restrict__ grad_all) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long)nconf * nterms) return;
    const size_t c = (size_t)(gi / nterms);
    const int t = (int)(gi % nterms);
    const int4 ti = tidx[t];
    const double* p = tpar + 5 * t;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* mu_bar = mu_bar_all ? mu_bar_all + 3 * c : nullptr;
    const double* pb = pb_all ? pb_all + c * 9 * (size_t)n : nullptr;
    double* out = grad_all + c * (size_t)np + n;
    if (ti.x == 0) {  // bond p1-p2
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z);
        const double da = adjoint_weight(ti.y, x1, mu_bar, pb) - adjoint_weight(ti.z, x2, mu_bar, pb);
        double r;
        const double gk = distance_piece(pb, ti.y, ti.z, x1, x2, dsub(x1, x2), r);
        out += 2 * t;
        out[0] = da * (r - p[1]) + gk;
        out[1] = -p[0] * da;
    } else if (ti.x == 1) {  // angle p1-p2-p3, p2 central
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double wa = adjoint_weight(ti.y, x1, mu_bar, pb) - 2 * adjoint_weight(ti.z, x2, mu_bar, pb) +
                          adjoint_weight(ti.w, x3, mu_bar, pb);
        const double3 d21 = dsub(x1, x2), d23 = dsub(x3, x2), d13 = dsub(x3, x1);
        const double r21_2 = ddot(d21, d21), r23_2 = ddot(d23, d23), r13_2 = ddot(d13, d13);
        const double r21 = sqrt(r21_2), r23 = sqrt(r23_2);
        const double cost = (r23_2 + r21_2 - r13_2) / 2 / r21 / r23;   // flux_term's law-of-cosines cosine
        const double theta = acos(cost);
        double gk = 0;
        if (pb) {
            const double inv_s = 1 / sqrt(1 - cost * cost);
            const double c1 = (1.0 / r21 / r23) * inv_s, c21 = cost * inv_s / r21_2, c23 = cost * inv_s / r23_2;
            const double3 v1 = make_double3(-c1 * d23.x + c21 * d21.x, -c1 * d23.y + c21 * d21.y, -c1 * d23.z + c21 * d21.z);
            const double3 v3 = make_double3(-c1 * d21.x + c23 * d23.x, -c1 * d21.y + c23 * d23.y, -c1 * d21.z + c23 * d23.z);
            const double3 v2 = make_double3(-v1.x - v3.x, -v1.y - v3.y, -v1.z - v3.z);
            const double3 w = make_double3(x1.x - 2 * x2.x + x3.x, x1.y - 2 * x2.y + x3.y, x1.z - 2 * x2.z + x3.z);
            gk = bilinear(pb, ti.y, w, v1) + bilinear(pb, ti.z, w, v2) + bilinear(pb, ti.w, w, v3);
        }
        out += 2 * nb + 2 * (t - nb);
        out[0] = wa * (theta - p[1]) + gk;
        out[1] = -p[0] * wa;
    } else {  // water O,H1,H2
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double a1 = adjoint_weight(ti.y, x1, mu_bar, pb);
        const double a2 = adjoint_weight(ti.z, x2, mu_bar, pb) - a1, a3 = adjoint_weight(ti.w, x3, mu_bar, pb) - a1;
        const double3 w2 = dsub(x2, x1), w3 = dsub(x3, x1);
        const double3 w23 = make_double3(w2.x + w3.x, w2.y + w3.y, w2.z + w3.z);
        double r12, r13, r23;
        const double g12_2 = distance_piece(pb, ti.y, ti.z, x1, x2, w2, r12);   // r12 with c = (-1, 1, 0)
        const double g12_3 = distance_piece(pb, ti.y, ti.z, x1, x2, w3, r12);   // r12 with c = (-1, 0, 1)
        const double g13_2 = distance_piece(pb, ti.y, ti.w, x1, x3, w2, r13);
        const double g13_3 = distance_piece(pb, ti.y, ti.w, x1, x3, w3, r13);
        const double g23 = distance_piece(pb, ti.z, ti.w, x2, x3, w23, r23);
        const double b0 = p[3], ub0 = p[4];
        out += 2 * nb + 2 * na + 5 * (t - nb - na);
        out[0] = a2 * (r12 - b0) + a3 * (r13 - b0) + g12_2 + g13_3;
        out[1] = a2 * (r13 - b0) + a3 * (r12 - b0) + g13_2 + g12_3;
        out[2] = (a2 + a3) * (r23 - ub0) + g23;
        out[3] = -(p[0] + p[1]) * (a2 + a3);
        out[4] = -p[2] * (a2 + a3);
    }
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

// one pass of nconf <= w.cap conformations: at most three launches
void launch_batch_dipole(Handle& h, const BatchWs& w, int nconf, const double* pos, double* dipole, double* apt,
                         double* charges) {
    if (nconf <= 0 || nconf > w.cap || nconf > kBatchMaxPass) throw std::invalid_argument("launch_batch_dipole: pass size");
    launch_batch_flux_charges(h, w, nconf, pos, charges);
    if (dipole || apt)
        hipLaunchKernelGGL(k_bd_apt, dim3(nblk(h.n, 256), nconf), dim3(256), 0, h.stream, h.n, 3L * h.nd, h.ccsr_start,
                           h.ccsr_ent, pos, w.q, w.dqdx, dipole, apt);
}

// one pass of nconf <= kBatchMaxPass conformations: at most two launches, no workspace
void launch_batch_dipole_vjp(Handle& h, int nconf, const double* pos, const double* dipole_bar, const double* apt_bar,
                             double* grad) {
    if (nconf <= 0 || nconf > kBatchMaxPass) throw std::invalid_argument("launch_batch_dipole_vjp: pass size");
    const int n = h.n;
    const long np = (long)n + 2L * h.nb + 2L * h.na + 5L * h.nw;
    hipLaunchKernelGGL(k_bd_base, dim3(nblk(n, 256), nconf), dim3(256), 0, h.stream, n, np, pos, dipole_bar, apt_bar,
                       grad);
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bd_terms, dim3(nblk((int64_t)nconf * h.nterms, 256)), dim3(256), 0, h.stream, nconf, n,
                           h.nterms, h.nb, h.na, np, h.term_idx, h.term_par, pos, dipole_bar, apt_bar, grad);
}

}  // namespace cf
