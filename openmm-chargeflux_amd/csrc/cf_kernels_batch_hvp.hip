// cf_kernels_batch_hvp.hip -- cf_compute_batch_hvp: Hessian-vector products of the non-periodic
// batch (cf_kernels_batch.hip) with respect to the positions ("batched,
// Hessian-vector products").  Per conformation x and direction v, with F the forces of
// cf_compute_batch, H v = -D_v F in closed form (no finite differences):
//     (H v)_i = -D_v F_i^pair + sum_a (gdot_a D_ai + g_a Ddot_ai)
//     F_i^pair   = -sum_j s_ij d,   d = x_j - x_i,  s = (A + C) / r^2,  A = e4 s6 (12 s6 - 6),  C = ke q_i q_j / r
//     D_v F_i^pair = -sum_j (sdot d + s w),   w = v_j - v_i
//     sdot = [e4 s6 (48 - 168 s6) - 3 C] (d.w) / r^4 + ke (qdot_i q_j + q_i qdot_j) / r^3
//     g_a = dE/dq_a = ke sum_j q_j / r,   gdot_a = ke sum_j [qdot_j / r - q_j (d.w) / r^3]
//     D = dq/dx (the forward path's blocks),  Ddot = D_v D,  qdot = D_v q
// over the non-excluded j != i; the chain-rule sum runs over atom i's ccsr entries in entry order
// (chain_rule_atom's).  Ddot and the charge slots' tangents come from flux_term's expressions
// evaluated on dual numbers (cf_flux_dual.h).  Nothing divides by a parameter: k = 0 is legal.
//
// A pass is nconf conformations x kv directions; the kv directions of a conformation share its
// q and D (k_b_flux, k_b_charges: once per conformation).  Then k_bh_terms, k_bh_qdot, k_bh_pairs,
// k_bh_chain with the (conformation, direction) row cv = c * kv + k as the batch index: at most six
// launches whatever nconf and kv.  Ddot is STORED by k_bh_terms and read by k_bh_chain (an atom
// of a water gathers 9 entries: recomputing them there would evaluate each term's duals once per
// entry instead of once).
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N and the topology: the row of a
// (conformation, direction) is bitwise the same alone, at any position of any batch, for any number
// of directions and under any pass size.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms, kv and the launch's own row count: no device guard bits.
#include <stdexcept>

#include "cf_flux_dual.h"

namespace cf {

// ---------------------------------------------------------------------------------
// 1. term tangents: one lane per flattened (row, term), g = cv * nterms + t -- k_b_flux's layout
//    with the row in the conformation's place.  The lane's Ddot block goes to LDS and the block's
//    run is written coalesced (batch_flux_block's way); the tangents of the term's charge slots go
//    to dslot[cv][S].
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bh_terms(int nrows, int kv, int n, int nterms, int nb, int na, int nslots,
                                                  long nd3, const int4* __restrict__ tidx,
                                                  const double* __restrict__ tpar, const double* __restrict__ pos_all,
                                                  const double* __restrict__ vec_all, long vstride,
                                                  double* __restrict__ dslot_all, double* __restrict__ ddot_all) {
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
        flux_term_nopbc<Dual>(ti.x, tpar + 5 * t, x1, x2, x3, dq, [o](int e, Dual val) { o[e] = val.d; });
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
// 2. charge tangents: one lane per (row, atom), qdot_i = the atom's slot tangents added in qcsr
//    slot order (k_b_charges's gather)
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bh_qdot(int n, int nslots, const int* __restrict__ qs,
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
// 3. all pairs: the shape of k_bg_pairs.  A block is kHvpI = 64 i-atoms of one row, one per lane,
//    in each of its four waves; the j-atoms pass through LDS in tiles of 256 -- (x, y, z, q),
//    (v, qdot) and the LJ pair (sigma/2, 2 sqrt eps): 10 doubles per entry -- and wave w takes
//    entries [64 w, 64 w + 64) of every tile as an LDS broadcast.  The four waves' partial sums are
//    added as (w0 + w1) + (w2 + w3).  Excluded pairs are skipped by in_excl, as in the forward path.
//    Writes -D_v F^pair to out (overwriting it), g and gdot to the workspace.
// ---------------------------------------------------------------------------------
constexpr int kHvpI = 64;
constexpr int kHvpJ = 256;

__global__ void __launch_bounds__(kHvpJ) k_bh_pairs(int n, int kv, double ke, const double* __restrict__ pos_all,
                                                    const double* __restrict__ q_all, const double* __restrict__ vec_all,
                                                    long vstride, const double* __restrict__ qdot_all,
                                                    const double2* __restrict__ lj, const int* __restrict__ ex_start,
                                                    const int* __restrict__ ex_list, double* __restrict__ g_all,
                                                    double* __restrict__ gdot_all, double* __restrict__ out_all) {
    __shared__ double4 sp[kHvpJ];
    __shared__ double4 sv[kHvpJ];
    __shared__ double2 sl[kHvpJ];
    __shared__ double red[3][5][kHvpI];   // partial sums of waves 1..3
    const size_t cv = blockIdx.y;
    const size_t c = cv / (size_t)kv, k = cv % (size_t)kv;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    const double* vel = vec_all + c * (size_t)vstride + k * 3 * (size_t)n;
    const double* qdot = qdot_all + cv * (size_t)n;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kHvpI + lane;
    const bool active = i < n;
    double4 pi = make_double4(0, 0, 0, 0), vi = make_double4(0, 0, 0, 0);
    double2 li = make_double2(0, 0);
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        pi = make_double4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], q[i]);
        vi = make_double4(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], qdot[i]);
        li = lj[i];
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int m = 0; m < kMaxRegExcl; m++) reg[m] = m < exc ? ex_list[ex0 + m] : -1;
    double hx = 0, hy = 0, hz = 0, g = 0, gd = 0;
    for (int base = 0; base < n; base += kHvpJ) {
        const int j = base + threadIdx.x;
        __syncthreads();
        if (j < n) {
            sp[threadIdx.x] = make_double4(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], q[j]);
            sv[threadIdx.x] = make_double4(vel[3 * j], vel[3 * j + 1], vel[3 * j + 2], qdot[j]);
            sl[threadIdx.x] = lj[j];
        }
        __syncthreads();
        const int t1 = min(64 * w + 64, n - base);
        if (!active) continue;
        for (int t = 64 * w; t < t1; t++) {
            const int jj = base + t;
            if (jj == i) continue;
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) continue;
            const double4 pj = sp[t];
            const double4 vj = sv[t];
            const double2 lj2 = sl[t];
            const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;   // getDeltaR(i, j)
            const double wx = vj.x - vi.x, wy = vj.y - vi.y, wz = vj.z - vi.z;
            const double inv_r = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
            const double inv_r2 = inv_r * inv_r;
            const double dw = dx * wx + dy * wy + dz * wz;
            const double sig = li.x + lj2.x;
            double s2 = inv_r * sig; s2 *= s2;
            const double sig6 = s2 * s2 * s2;
            const double es6 = sig6 * li.y * lj2.y;
            const double kr = ke * inv_r;
            const double cq = kr * pi.w * pj.w;                                  // C
            const double s = (es6 * (12 * sig6 - 6) + cq) * inv_r2;
            const double sd = ((es6 * (48 - 168 * sig6) - 3 * cq) * (dw * inv_r2) + kr * (vi.w * pj.w + pi.w * vj.w)) * inv_r2;
            hx += sd * dx + s * wx;
            hy += sd * dy + s * wy;
            hz += sd * dz + s * wz;
            g += kr * pj.w;
            gd += kr * (vj.w - pj.w * dw * inv_r2);
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = hx; red[w - 1][1][lane] = hy; red[w - 1][2][lane] = hz;
        red[w - 1][3][lane] = g; red[w - 1][4][lane] = gd;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    hx = (hx + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
    hy = (hy + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
    hz = (hz + red[0][2][lane]) + (red[1][2][lane] + red[2][2][lane]);
    g = (g + red[0][3][lane]) + (red[1][3][lane] + red[2][3][lane]);
    gd = (gd + red[0][4][lane]) + (red[1][4][lane] + red[2][4][lane]);
    g_all[cv * (size_t)n + i] = g;
    gdot_all[cv * (size_t)n + i] = gd;
    double* o = out_all + c * (size_t)vstride + k * 3 * (size_t)n + 3 * (size_t)i;
    o[0] = hx; o[1] = hy; o[2] = hz;
}

// ---------------------------------------------------------------------------------
// 4. chain rule: one lane per (row, atom b).  out_b += sum_e (gdot[a_e] D_e + g[a_e] Ddot_e) over
//    the ccsr entries of b in entry order (chain_rule_atom's gather, batches of 4 entries in
//    flight), D of the row's conformation and Ddot of the row.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bh_chain(int n, int kv, long nd3, const int* __restrict__ cs,
                                                  const int2* __restrict__ ce, const double* __restrict__ g_all,
                                                  const double* __restrict__ gdot_all,
                                                  const double* __restrict__ dqdx_all,
                                                  const double* __restrict__ ddot_all, long vstride,
                                                  double* __restrict__ out_all) {
    const size_t cv = blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const size_t c = cv / (size_t)kv, k = cv % (size_t)kv;
    const double* gw = g_all + cv * (size_t)n;
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
// most six launches
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

size_t batch_hvp_doubles_per_row(const Handle& h) {
    // slot tangents, Ddot, qdot[N], g[N], gdot[N]
    return (size_t)h.nslots_dq + 3 * (size_t)h.nd + 3 * (size_t)h.n;
}

void batch_hvp_carve(const Handle& h, double* base, int cap, BatchHvpWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n;
    w.base = base; w.cap = cap;
    w.dslot = base;
    w.ddot = w.dslot + c * (size_t)h.nslots_dq;
    w.qdot = w.ddot + c * 3 * (size_t)h.nd;
    w.g = w.qdot + c * n;
    w.gdot = w.g + c * n;
}

void launch_batch_hvp(Handle& h, const BatchWs& w, const BatchHvpWs& hw, int nconf, int kv, const double* pos,
                      const double* vec, long vstride, double* out) {
    const int64_t rows64 = (int64_t)nconf * kv;
    if (nconf <= 0 || kv <= 0 || nconf > w.cap || rows64 > hw.cap || rows64 > kBatchMaxPass)
        throw std::invalid_argument("launch_batch_hvp: pass size");
    const int n = h.n, rows = (int)rows64;
    const long nd3 = 3L * h.nd;
    launch_batch_flux_charges(h, w, nconf, pos, nullptr);
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bh_terms, dim3(nblk((int64_t)rows * h.nterms, 256)), dim3(256), 0, h.stream, rows, kv, n,
                           h.nterms, h.nb, h.na, h.nslots_dq, nd3, h.term_idx, h.term_par, pos, vec, vstride, hw.dslot,
                           hw.ddot);
    hipLaunchKernelGGL(k_bh_qdot, dim3(nblk(n, 256), rows), dim3(256), 0, h.stream, n, h.nslots_dq, h.qcsr_start,
                       h.qcsr_slot, hw.dslot, hw.qdot);
    hipLaunchKernelGGL(k_bh_pairs, dim3(nblk(n, kHvpI), rows), dim3(kHvpJ), 0, h.stream, n, kv, h.ke, pos, w.q, vec,
                       vstride, hw.qdot, h.lj, h.ex_start, h.ex_list, hw.g, hw.gdot, out);
    hipLaunchKernelGGL(k_bh_chain, dim3(nblk(n, 256), rows), dim3(256), 0, h.stream, n, kv, nd3, h.ccsr_start,
                       h.ccsr_ent, hw.g, hw.gdot, w.dqdx, hw.ddot, vstride, out);
}

}  // namespace cf
