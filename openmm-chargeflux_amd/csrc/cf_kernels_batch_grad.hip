// cf_kernels_batch_grad.hip -- cf_compute_batch_vjp: the reverse-mode product of the non-periodic
// batch (cf_kernels_batch.hip) with respect to the base charges and the flux parameters
// ("batched, parameter gradients").  Per conformation, with cotangents e_bar
// (scalar), q_bar[N] and v = F_bar[N][3], the scalar L = e_bar E + sum q_bar_i q_i + sum v_i . F_i
// has
//     dL/d(base charge i) = a_i = e_bar g_i + q_bar_i - h_i
//     g_i = dE/dq_i = ke sum_j q_j / r_ij                      (the forward path's dedq)
//     h_i = D_v g_i = ke sum_j [ qdot_j / r_ij - q_j (x_i - x_j).(v_i - v_j) / r_ij^3 ]
//     qdot = D_v q  (the charges' tangent along v: every flux term's tangent, gathered per atom)
// over the non-excluded j != i, and every flux parameter's gradient is a product of a_i, g_i and
// the term's geometry and its tangent (k_bg_terms).  A pass is k_b_flux, k_b_charges (as they are),
// then k_bg_tangent, k_bg_pairs, k_bg_terms: at most five launches whatever nconf.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N and the topology: a
// conformation's gradients are bitwise the same alone, in any batch and under any chunking.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms and the launch's own nconf: no device guard bits.
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

// ---------------------------------------------------------------------------------
// term geometry and its tangent along v, from positions alone (never through a division by a
// parameter: a term with k = 0 is legal).  x[] holds the value each parameter group multiplies,
// xd[] its tangent:
//   bond   x[0] = r                      xd[0] = rdot
//   angle  x[0] = theta                  xd[0] = thetadot = -cdot / sqrt(1 - c^2)
//   water  x = (r12, r13, r23)           xd = (r12dot, r13dot, r23dot)
// with rdot_ab = (x_b - x_a).(v_b - v_a) / r_ab and c the law-of-cosines cosine of flux_term.
// vel == nullptr: v = 0, xd = 0.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(double3 a, double3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double3 sub3(double3 a, double3 b) { return make_double3(a.x - b.x, a.y - b.y, a.z - b.z); }

__device__ __forceinline__ void term_geometry(int4 ti, const double* __restrict__ pos, const double* __restrict__ vel,
                                              double x[3], double xd[3]) {
    x[0] = x[1] = x[2] = 0.0;
    xd[0] = xd[1] = xd[2] = 0.0;
    if (ti.x == 0) {  // bond p1-p2
        const double3 d = sub3(ld3(pos, ti.z), ld3(pos, ti.y));
        const double r = sqrt(dot3(d, d));
        x[0] = r;
        if (vel) xd[0] = dot3(d, sub3(ld3(vel, ti.z), ld3(vel, ti.y))) / r;
    } else if (ti.x == 1) {  // angle p1-p2-p3, p2 central
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double3 d21 = sub3(x1, x2), d23 = sub3(x3, x2), d13 = sub3(x3, x1);
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
        const double3 d12 = sub3(x2, x1), d13 = sub3(x3, x1), d23 = sub3(x3, x2);
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
// 2. charge tangents: one lane per (conformation, atom).  qdot_i = sum over the atom's charge
//    slots, in qcsr slot order (the order k_b_charges adds the charge deltas), of the slot's
//    tangent: slot s is role s' of term t (bonds 2 slots: +, -; angles 3: 1, -2, 1; waters 3:
//    -(dq2 + dq3), dq2, dq3), recomputed from the term's geometry.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bg_tangent(int n, int nb, int na, const int4* __restrict__ tidx,
                                                    const double* __restrict__ tpar, const int* __restrict__ qs,
                                                    const int* __restrict__ qslot, const double* __restrict__ pos_all,
                                                    const double* __restrict__ v_all, double* __restrict__ qdot_all) {
    const size_t c = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* vel = v_all + c * 3 * (size_t)n;
    double qd = 0;
    for (int k = qs[i]; k < qs[i + 1]; k++) {
        const int s = qslot[k];
        int t, role;
        if (s < 2 * nb) { t = s >> 1; role = s & 1; }
        else { const int u = s - 2 * nb; t = nb + u / 3; role = u % 3; }   // angles then waters: 3 slots each
        const int4 ti = tidx[t];
        const double* p = tpar + 5 * t;
        double x[3], xd[3];
        term_geometry(ti, pos, vel, x, xd);
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
// 3. all pairs: the shape of k_b_pairs.  A block is kGradI = 64 i-atoms of one conformation, one
//    per lane, in each of its four waves; the j-atoms pass through LDS in tiles of 256 -- (x, y,
//    z, q) and, with a force cotangent, (v, qdot): 8 doubles per entry -- and wave w takes entries
//    [64 w, 64 w + 64) of every tile as an LDS broadcast.  The four waves' partial sums are added as
//    (w0 + w1) + (w2 + w3).  Excluded pairs are skipped by in_excl, as in the forward path.
//    HAS_V = false (no force cotangent): h = 0, only g is summed (no v / qdot traffic or
//    arithmetic; the choice is an instantiation, not a branch in the j loop).
//    Epilogue: g_i and a_i = e_bar g_i + q_bar_i - h_i to the workspace, a_i also to grad[c][i].
// ---------------------------------------------------------------------------------
constexpr int kGradI = 64;
constexpr int kGradJ = 256;

template <bool HAS_V>
__global__ void __launch_bounds__(kGradJ) k_bg_pairs(int n, long np, double ke, const double* __restrict__ pos_all,
                                                     const double* __restrict__ q_all, const double* __restrict__ v_all,
                                                     const double* __restrict__ qdot_all, const int* __restrict__ ex_start,
                                                     const int* __restrict__ ex_list, const double* __restrict__ e_bar,
                                                     const double* __restrict__ q_bar_all, double* __restrict__ g_all,
                                                     double* __restrict__ a_all, double* __restrict__ grad_all) {
    __shared__ double4 sp[kGradJ];
    __shared__ double4 sv[HAS_V ? kGradJ : 1];
    __shared__ double red[3][2][kGradI];   // partial sums of waves 1..3
    const size_t c = blockIdx.y;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    const double* vel = HAS_V ? v_all + c * 3 * (size_t)n : nullptr;
    const double* qdot = HAS_V ? qdot_all + c * (size_t)n : nullptr;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kGradI + lane;
    const bool active = i < n;
    double4 pi = make_double4(0, 0, 0, 0);
    double3 vi = make_double3(0, 0, 0);
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        pi = make_double4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], q[i]);
        if (HAS_V) vi = make_double3(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]);
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int k = 0; k < kMaxRegExcl; k++) reg[k] = k < exc ? ex_list[ex0 + k] : -1;
    double g = 0, hs = 0;
    for (int base = 0; base < n; base += kGradJ) {
        const int j = base + threadIdx.x;
        __syncthreads();
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
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) continue;
            const double4 pj = sp[t];
            const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            const double inv_r = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
            g += ke * pj.w * inv_r;
            if (HAS_V) {
                const double4 vj = sv[t];
                // (x_i - x_j).(v_i - v_j) = d.(v_j - v_i)
                const double s = dx * (vj.x - vi.x) + dy * (vj.y - vi.y) + dz * (vj.z - vi.z);
                hs += ke * inv_r * (vj.w - pj.w * s * inv_r * inv_r);
            }
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = g;
        if (HAS_V) red[w - 1][1][lane] = hs;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    g = (g + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
    double a = (e_bar ? e_bar[c] : 0.0) * g + (q_bar_all ? q_bar_all[c * (size_t)n + i] : 0.0);
    if (HAS_V) {
        hs = (hs + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
        a -= hs;
    }
    g_all[c * (size_t)n + i] = g;
    a_all[c * (size_t)n + i] = a;
    grad_all[c * (size_t)np + i] = a;
}

// ---------------------------------------------------------------------------------
// 4. term gradients: one lane per flattened (conformation, term), g = c * nterms + t.  The term's
//    geometry and tangent again (term_geometry), a and g of its atoms, its 2 or 5 gradients into
//    grad[c][N + ...] in the order of the cf_params arrays: bonds (k, b), angles (k, theta0),
//    waters (k1, k2, kub, b0, ub0).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bg_terms(int nconf, int n, int nterms, int nb, int na, long np,
                                                  const int4* __restrict__ tidx, const double* __restrict__ tpar,
                                                  const double* __restrict__ pos_all, const double* __restrict__ v_all,
                                                  const double* __restrict__ g_all, const double* __restrict__ a_all,
                                                  double* __restrict__ grad_all) {
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
    double x[3], xd[3];
    term_geometry(ti, pos, vel, x, xd);
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
// launcher: one pass of nconf <= min(w.cap, gw.cap) conformations, at most five launches
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

size_t batch_grad_doubles_per_conf(const Handle& h) { return 3 * (size_t)h.n; }   // qdot[N], g[N], a[N]

void batch_grad_carve(const Handle& h, double* base, int cap, BatchGradWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n;
    w.base = base; w.cap = cap;
    w.qdot = base;
    w.g = w.qdot + c * n;
    w.a = w.g + c * n;
}

void launch_batch_vjp(Handle& h, const BatchWs& w, const BatchGradWs& gw, int nconf, const double* pos,
                      const double* e_bar, const double* q_bar, const double* f_bar, double* grad) {
    if (nconf <= 0 || nconf > w.cap || nconf > gw.cap || nconf > kBatchMaxPass)
        throw std::invalid_argument("launch_batch_vjp: pass size");
    const int n = h.n;
    const long np = (long)n + 2L * h.nb + 2L * h.na + 5L * h.nw;
    launch_batch_flux_charges(h, w, nconf, pos, nullptr);
    if (f_bar)
        hipLaunchKernelGGL(k_bg_tangent, dim3(nblk(n, 256), nconf), dim3(256), 0, h.stream, n, h.nb, h.na, h.term_idx,
                           h.term_par, h.qcsr_start, h.qcsr_slot, pos, f_bar, gw.qdot);
    const dim3 grid(nblk(n, kGradI), nconf);
    if (f_bar)
        hipLaunchKernelGGL(k_bg_pairs<true>, grid, dim3(kGradJ), 0, h.stream, n, np, h.ke, pos, w.q, f_bar, gw.qdot,
                           h.ex_start, h.ex_list, e_bar, q_bar, gw.g, gw.a, grad);
    else
        hipLaunchKernelGGL(k_bg_pairs<false>, grid, dim3(kGradJ), 0, h.stream, n, np, h.ke, pos, w.q, nullptr, nullptr,
                           h.ex_start, h.ex_list, e_bar, q_bar, gw.g, gw.a, grad);
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bg_terms, dim3(nblk((int64_t)nconf * h.nterms, 256)), dim3(256), 0, h.stream, nconf, n,
                           h.nterms, h.nb, h.na, np, h.term_idx, h.term_par, pos, f_bar, gw.g, gw.a, grad);
}

}  // namespace cf
