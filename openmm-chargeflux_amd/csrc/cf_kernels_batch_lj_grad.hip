// cf_kernels_batch_lj_grad.hip -- cf_compute_batch_lj_vjp: the reverse-mode product of the batches
// (cf_kernels_batch.hip, cf_kernels_batch_pbc.hip) with respect to the Lennard-Jones sigma and
// epsilon of every atom ("batched, LJ parameter gradients").  The handle stores
// lj_i = (sigma_i / 2, 2 sqrt(eps_i)); a pair carries, with A = lj_i.x + lj_j.x, e4 = lj_i.y lj_j.y
// and s6 = (A / r)^6,
//     U_ij = e4 s6 (s6 - 1)
// over every non-excluded pair (periodic: minimum image within the cutoff, the pair set of
// k_bp_pairs).  Neither the pair set nor the charges depend on sigma or epsilon, so the Coulomb part
// does not enter: no flux, charge or k-space stage.  Per conformation, with cotangents e_bar (scalar)
// and v = F_bar[N][3], the scalar L = e_bar E + sum v_i . F_i has v . F_LJ = sum_pairs W_ij,
// W_ij = e4 (12 s6^2 - 6 s6) rdot_ij / r, rdot_ij = d_ij . (v_i - v_j) / r, and
//     dL/dsigma_i = 1/2 sum_j e4 (A^5 / r^6) [e_bar (12 s6 - 6) + (144 s6 - 36) rdot_ij / r]
//     T'_i        =     sum_j lj_j.y [e_bar s6 (s6 - 1) + (12 s6^2 - 6 s6) rdot_ij / r]
//     dL/deps_i   = 2 T'_i / lj_i.y
// A^5 / r^6 is computed as such: nothing divides by sigma or A (sigma_i = sigma_j = 0 gives 0).
// Convention: an atom with eps_i = 0 receives exactly 0 for both gradients (it has no LJ
// interaction; the derivative of sqrt(eps_i eps_j) is singular there).
// A pass is one launch, without a workspace.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N and the topology: a
// conformation's gradients are bitwise the same alone, in any batch and under any chunking.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n and the launch's own nconf: no device guard bits.
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

// ---------------------------------------------------------------------------------
// the shape of k_bg_pairs / k_bpg_pairs.  A block is kLjI = 64 i-atoms of one conformation, one
// per lane, in each of its four waves; the j-atoms pass through LDS in tiles of 256 --
// (x, y, z, sigma_j / 2) and, with a force cotangent, (v_j, 2 sqrt eps_j), else 2 sqrt eps_j
// alone -- and wave w takes entries [64 w, 64 w + 64) of every tile.  The j index is
// wave-uniform: an entry with lj_j.y == 0 (the hydrogens of water) is skipped by a uniform
// branch, its terms being exact zeros.  PBC: delta_r minimum image with the conformation's box,
// then r^2 <= rc^2 (k_bp_pairs' test).  Excluded partners carry no LJ.  The four waves' partial
// sums are added as (w0 + w1) + (w2 + w3); the epilogue writes g_sigma / 2 to grad[c][i] and
// 2 T' / lj_i.y to grad[c][N + i].
// LDS: two j tiles 16384 B (HAS_V) or 10240 B + partial sums 3072 B.
// ---------------------------------------------------------------------------------
constexpr int kLjI = 64;
constexpr int kLjJ = 256;

template <bool PBC, bool HAS_V>
__global__ void __launch_bounds__(kLjJ) k_blj_pairs(int n, double rc2, const double* __restrict__ boxes,
                                                    const double* __restrict__ pos_all,
                                                    const double2* __restrict__ lj,
                                                    const double* __restrict__ e_bar,
                                                    const double* __restrict__ v_all,
                                                    const int* __restrict__ ex_start, const int* __restrict__ ex_list,
                                                    double* __restrict__ grad_all) {
    __shared__ double4 sp[kLjJ];
    __shared__ double4 sv[HAS_V ? kLjJ : 1];
    __shared__ double se[HAS_V ? 1 : kLjJ];
    __shared__ double red[3][2][kLjI];   // partial sums of waves 1..3
    const size_t c = blockIdx.y;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* vel = HAS_V ? v_all + c * 3 * (size_t)n : nullptr;
    const double eb = e_bar ? e_bar[c] : 0.0;
    double3 L = make_double3(0.0, 0.0, 0.0), T = make_double3(0.0, 0.0, 0.0);
    if (PBC) load_box(boxes, c, L, T);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kLjI + lane;
    const bool active = i < n;
    double3 xi = make_double3(0, 0, 0), vi = make_double3(0, 0, 0);
    double2 li = make_double2(0, 0);
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        xi = ld3(pos, i);
        li = lj[i];
        if (HAS_V) vi = ld3(vel, i);
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int k = 0; k < kMaxRegExcl; k++) reg[k] = k < exc ? ex_list[ex0 + k] : -1;
    const bool work = active && li.y != 0.0;   // eps_i = 0: no LJ interaction, both gradients exactly 0
    double gs = 0, tp = 0;
    for (int base = 0; base < n; base += kLjJ) {
        const int j = base + threadIdx.x;
        __syncthreads();
        if (j < n) {
            const double2 l = lj[j];
            sp[threadIdx.x] = make_double4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], l.x);
            if (HAS_V) sv[threadIdx.x] = make_double4(vel[3 * j], vel[3 * j + 1], vel[3 * j + 2], l.y);
            else se[threadIdx.x] = l.y;
        }
        __syncthreads();
        const int t1 = min(64 * w + 64, n - base);
        if (!work) continue;
        for (int t = 64 * w; t < t1; t++) {
            double4 vj = make_double4(0, 0, 0, 0);
            double ey;
            if (HAS_V) { vj = sv[t]; ey = vj.w; }
            else ey = se[t];
            if (ey == 0.0) continue;   // wave-uniform
            const int jj = base + t;
            if (jj == i) continue;
            const double4 pj = sp[t];
            double3 d;
            if (PBC) d = delta_r(make_double3(pj.x, pj.y, pj.z), xi, L, 1, T);   // x_i - x_j
            else d = make_double3(xi.x - pj.x, xi.y - pj.y, xi.z - pj.z);
            const double r2 = d.x * d.x + d.y * d.y + d.z * d.z;
            if (PBC && !(r2 <= rc2)) continue;
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) continue;
            const double ir2 = 1.0 / r2;
            const double A = li.x + pj.w;
            const double A2 = A * A, ir6 = ir2 * ir2 * ir2;
            const double a5r6 = A2 * A2 * A * ir6;   // A^5 / r^6
            const double s6 = a5r6 * A;
            double cs = eb * (12 * s6 - 6);              // bracket of g_sigma
            double ct = eb * (s6 * (s6 - 1));            // bracket of T'
            if (HAS_V) {
                // rdot / r = d . (v_i - v_j) / r^2
                const double rr = (d.x * (vi.x - vj.x) + d.y * (vi.y - vj.y) + d.z * (vi.z - vj.z)) * ir2;
                cs += (144 * s6 - 36) * rr;
                ct += (12 * s6 * s6 - 6 * s6) * rr;
            }
            gs += li.y * ey * a5r6 * cs;
            tp += ey * ct;
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = gs;
        red[w - 1][1][lane] = tp;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    gs = (gs + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
    tp = (tp + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
    double* out = grad_all + c * 2 * (size_t)n;
    out[i] = work ? 0.5 * gs : 0.0;
    out[(size_t)n + i] = work ? 2.0 * tp / li.y : 0.0;
}

// ---------------------------------------------------------------------------------
// launcher: one pass of nconf <= kBatchMaxPass conformations, one launch
// ---------------------------------------------------------------------------------
void launch_batch_lj_vjp(Handle& h, int nconf, const double* pos, const double* boxes, const double* e_bar,
                         const double* f_bar, double* grad) {
    if (nconf <= 0 || nconf > kBatchMaxPass) throw std::invalid_argument("launch_batch_lj_vjp: pass size");
    if ((h.pbc != 0) != (boxes != nullptr)) throw std::invalid_argument("launch_batch_lj_vjp: boxes");
    const int n = h.n;
    const dim3 grid((n + kLjI - 1) / kLjI, nconf);
    const double rc2 = h.cutoff * h.cutoff;
#define CF_LJ_LAUNCH(PBC, HAS_V)                                                                              \
    hipLaunchKernelGGL((k_blj_pairs<PBC, HAS_V>), grid, dim3(kLjJ), 0, h.stream, n, rc2, boxes, pos, h.lj, e_bar, \
                       f_bar, h.ex_start, h.ex_list, grad)
    if (h.pbc) {
        if (f_bar) CF_LJ_LAUNCH(true, true);
        else CF_LJ_LAUNCH(true, false);
    } else {
        if (f_bar) CF_LJ_LAUNCH(false, true);
        else CF_LJ_LAUNCH(false, false);
    }
#undef CF_LJ_LAUNCH
}

}  // namespace cf
