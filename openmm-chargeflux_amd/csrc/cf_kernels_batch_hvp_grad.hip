// cf_kernels_batch_hvp_grad.hip -- cf_compute_batch_hvp_vjp: the reverse-mode product of the
// Hessian-vector products of the non-periodic batch (cf_kernels_batch_hvp.hip) with respect to the base
// charges and the flux parameters ("batched, Hessian-vector parameter gradients").
// Per conformation x, with directions v_k and cotangents u_k, the scalar is
//     L = sum_k u_k . H(x) v_k = sum_k D_u D_v E.
// E depends on these parameters only through the charges q and is quadratic in them (E = E_LJ +
// q^T A q / 2, A_ij = ke / r_ij over the non-excluded pairs), so with g = A q and the directional
// derivatives q^u = D_u q, q^v = D_v q, q^uv = D_u D_v q of the charges after flux
//     dL/dtheta = sum_k sum_a [ g^uv_a dq_a/dtheta + g^u_a dq^v_a/dtheta + g^v_a dq^u_a/dtheta + g_a dq^uv_a/dtheta ]
//     g_i    = ke sum_j q_j / r
//     g^u_i  = ke sum_j [ q^u_j / r - q_j (d.w^u) / r^3 ]                      (g^v likewise)
//     g^uv_i = ke sum_j [ q^uv_j / r - (q^u_j (d.w^v) + q^v_j (d.w^u) + q_j (w^u.w^v)) / r^3
//                         + 3 q_j (d.w^u)(d.w^v) / r^5 ]
// with d = x_j - x_i, w^u = u_j - u_i, w^v = v_j - v_i over the non-excluded j != i.  Every flux piece
// is q_a += c_a k (gamma(x) - ref), so
//     dL/d(base charge i) = sum_k g^uv_i
//     dL/dk   += sum_k sum_a c_a [ g^uv_a (gamma - ref) + g^u_a gamma^v + g^v_a gamma^u + g_a gamma^uv ]
//     dL/dref += -k sum_k sum_a c_a g^uv_a
// with the pieces and signs of k_bg_terms, and gamma's derivatives from the term's geometry evaluated
// on hyper-dual numbers (cf_flux_dual.h: HDual).  LJ does not enter, and neither does dq/dx or its
// tangent.  Nothing divides by a parameter: k = 0 is legal.
//
// A pass is nconf conformations x kv directions: k_b_flux and k_b_charges once per conformation,
// then k_bhg_geom, k_bhg_qtan, k_bhg_pairs, k_bhg_rows: at most six launches.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N, the topology and the order of the
// directions: the last kernel adds a conformation's rows in ascending k to a running sum that
// starts at zero or, for a conformation whose directions take several passes, at what the earlier
// passes left in grad.  A conformation's gradient row is bitwise the same alone, at any position of
// any batch and however its directions are split into passes.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms, kv and the launch's own row count: no device guard bits.
#include <stdexcept>

#include "cf_flux_dual.h"

namespace cf {

// ---------------------------------------------------------------------------------
// 1. geometry tangents: one lane per flattened (row, term).  The term's atoms carry (x, u, v, 0) as
//    hyper-duals; the u, v and mixed parts of its geometries go to gam[row][0..3)[G].
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bhg_geom(int nrows, int kv, int n, int nterms, int nb, int na, int ngeo,
                                                  const int4* __restrict__ tidx, const double* __restrict__ pos_all,
                                                  const double* __restrict__ vec_all,
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
    term_gammas<HDual>(ti.x, x1, x2, x3, gam);
    double* o = gam_all + row * 3 * (size_t)ngeo + geom_start(t, nb, na);
    o[0] = gam[0].u; o[ngeo] = gam[0].w; o[2 * ngeo] = gam[0].uw;
    if (ti.x == 2) {
        o[1] = gam[1].u; o[ngeo + 1] = gam[1].w; o[2 * ngeo + 1] = gam[1].uw;
        o[2] = gam[2].u; o[ngeo + 2] = gam[2].w; o[2 * ngeo + 2] = gam[2].uw;
    }
}

// ---------------------------------------------------------------------------------
// 2. charge tangents: one lane per (row, atom).  q^u, q^v and q^uv of the atom = its slots'
//    tangents added in qcsr slot order (k_b_charges's gather); slot s is role s' of term t (bonds 2
//    slots: +, -; angles 3: 1, -2, 1; waters 3: -(dq2 + dq3), dq2, dq3), k times the geometry's tangent.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double slot_tangent(int type, int role, const double* __restrict__ p,
                                               const double* __restrict__ gm) {
    if (type == 0) {
        const double d = p[0] * gm[0];
        return role ? -d : d;
    }
    if (type == 1) {
        const double d = p[0] * gm[0];
        return role == 1 ? -2 * d : d;
    }
    const double d2 = p[0] * gm[0] + p[1] * gm[1] + p[2] * gm[2];
    const double d3 = p[0] * gm[1] + p[1] * gm[0] + p[2] * gm[2];
    return role == 0 ? -d2 - d3 : (role == 1 ? d2 : d3);
}

__global__ void __launch_bounds__(256) k_bhg_qtan(int n, int nb, int na, int ngeo, const double* __restrict__ tpar,
                                                  const int* __restrict__ qs, const int* __restrict__ qslot,
                                                  const double* __restrict__ gam_all, double* __restrict__ qt_all) {
    const size_t row = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* gam = gam_all + row * 3 * (size_t)ngeo;
    double qu = 0, qv = 0, quv = 0;
    for (int k = qs[i]; k < qs[i + 1]; k++) {
        const int s = qslot[k];
        int t, role;
        if (s < 2 * nb) { t = s >> 1; role = s & 1; }
        else { const int e = s - 2 * nb; t = nb + e / 3; role = e % 3; }   // angles then waters: 3 slots each
        const int type = t < nb ? 0 : (t < nb + na ? 1 : 2);
        const double* p = tpar + 5 * t;
        const double* gm = gam + geom_start(t, nb, na);
        qu += slot_tangent(type, role, p, gm);
        qv += slot_tangent(type, role, p, gm + ngeo);
        quv += slot_tangent(type, role, p, gm + 2 * ngeo);
    }
    double* o = qt_all + row * 3 * (size_t)n + i;
    o[0] = qu; o[n] = qv; o[2 * (size_t)n] = quv;
}

// ---------------------------------------------------------------------------------
// 3. all pairs, the hot path.  What a pair costs most -- the exclusion test, d, 1 / r and its powers --
//    does not depend on the direction, so a block is kHgI = 64 i-atoms of one conformation, one per
//    lane in each of its four waves, TIMES a chunk of kHgKC = 4 direction rows of that conformation:
//    blockIdx.y = conformation * nchunks + chunk.  The j-atoms pass through LDS in tiles of kHgJ = 128
//    entries -- (x, y, z, q) once, and per row of the chunk (u, q^u), (v, q^v) and q^uv, 9 doubles --
//    40 KB a block, so two blocks share a CU's LDS.  Wave w takes entries [32 w, 32 w + 32) of every
//    tile as LDS broadcasts; each lane keeps the chunk's 3 x 4 accumulators and g in registers, and
//    the four waves' partial sums are added as (w0 + w1) + (w2 + w3) through the LDS the tiles no
//    longer need.  A row the tail chunk does not have is zeros in LDS and registers, never a global
//    address.  g is summed by every chunk and written by chunk 0 alone.
//    Excluded pairs are skipped by in_excl, as in the forward path.
// ---------------------------------------------------------------------------------
constexpr int kHgI = 64;
constexpr int kHgJ = 128;
constexpr int kHgKC = 4;
constexpr int kHgSums = 3 * kHgKC + 1;
static_assert(3 * kHgSums * kHgI * sizeof(double) <= 2 * kHgKC * kHgJ * sizeof(double4), "the reduction reuses the row tiles");

__global__ void __launch_bounds__(256) k_bhg_pairs(int n, int kv, int nchunks, double ke,
                                                   const double* __restrict__ pos_all, const double* __restrict__ q_all,
                                                   const double* __restrict__ vec_all,
                                                   const double* __restrict__ ubar_all, long vstride,
                                                   const double* __restrict__ qt_all, const int* __restrict__ ex_start,
                                                   const int* __restrict__ ex_list, double* __restrict__ g_all,
                                                   double* __restrict__ gt_all) {
    __shared__ double4 sp[kHgJ];                 // (x, y, z, q)
    __shared__ double4 srow[2 * kHgKC][kHgJ];    // row k: [k] = (u, q^u), [kHgKC + k] = (v, q^v)
    __shared__ double sq[kHgKC][kHgJ];           // q^uv
    const size_t c = blockIdx.y / nchunks;
    const int k0 = (int)(blockIdx.y % nchunks) * kHgKC;
    const int kc = min(kHgKC, kv - k0);          // rows this chunk has
    const size_t row0 = c * (size_t)kv + k0;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    const size_t at0 = c * (size_t)vstride + (size_t)k0 * 3 * (size_t)n;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kHgI + lane;
    const bool active = i < n;
    double4 pi = make_double4(0, 0, 0, 0);
    double ui[kHgKC][3], vi[kHgKC][3];
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        pi = make_double4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], q[i]);
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int k = 0; k < kHgKC; k++) {
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
    double g = 0, gu[kHgKC], gv[kHgKC], guv[kHgKC];
#pragma unroll
    for (int k = 0; k < kHgKC; k++) gu[k] = gv[k] = guv[k] = 0;
    for (int base = 0; base < n; base += kHgJ) {
        __syncthreads();
        // the tile: item = slot * kHgJ + entry, slot 0 the atoms, slot 1 + k row k of the chunk
        for (int item = threadIdx.x; item < (1 + kHgKC) * kHgJ; item += 256) {
            const int e = item % kHgJ, slot = item / kHgJ;
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
            srow[k][e] = uj; srow[kHgKC + k][e] = vj; sq[k][e] = quv;
        }
        __syncthreads();
        const int t1 = min(32 * w + 32, n - base);
        if (!active) continue;
        for (int t = 32 * w; t < t1; t++) {
            const int jj = base + t;
            if (jj == i) continue;
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) continue;
            const double4 pj = sp[t];
            const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;   // getDeltaR(i, j)
            const double inv_r = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
            const double inv_r2 = inv_r * inv_r;
            const double kr = ke * inv_r;
            const double q3 = 3 * pj.w * inv_r2 * inv_r2;
            g += kr * pj.w;
#pragma unroll
            for (int k = 0; k < kHgKC; k++) {
                const double4 uj = srow[k][t], vj = srow[kHgKC + k][t];
                const double wux = uj.x - ui[k][0], wuy = uj.y - ui[k][1], wuz = uj.z - ui[k][2];
                const double wvx = vj.x - vi[k][0], wvy = vj.y - vi[k][1], wvz = vj.z - vi[k][2];
                const double du = dx * wux + dy * wuy + dz * wuz;
                const double dv = dx * wvx + dy * wvy + dz * wvz;
                const double uv = wux * wvx + wuy * wvy + wuz * wvz;
                gu[k] += kr * (uj.w - pj.w * du * inv_r2);
                gv[k] += kr * (vj.w - pj.w * dv * inv_r2);
                guv[k] += kr * (sq[k][t] - (uj.w * dv + vj.w * du + pj.w * uv) * inv_r2 + q3 * du * dv);
            }
        }
    }
    __syncthreads();   // every wave is done with the tiles: their LDS takes the partial sums of waves 1..3
    double (*red)[kHgSums][kHgI] = reinterpret_cast<double (*)[kHgSums][kHgI]>(&srow[0][0]);
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < kHgKC; k++) {
            red[w - 1][3 * k][lane] = gu[k]; red[w - 1][3 * k + 1][lane] = gv[k]; red[w - 1][3 * k + 2][lane] = guv[k];
        }
        red[w - 1][3 * kHgKC][lane] = g;
    }
    __syncthreads();
    if (w > 0 || !active) return;
#pragma unroll
    for (int k = 0; k < kHgKC; k++) {
        if (k < kc) {
            double* o = gt_all + (row0 + k) * 3 * (size_t)n + i;
            o[0] = (gu[k] + red[0][3 * k][lane]) + (red[1][3 * k][lane] + red[2][3 * k][lane]);
            o[n] = (gv[k] + red[0][3 * k + 1][lane]) + (red[1][3 * k + 1][lane] + red[2][3 * k + 1][lane]);
            o[2 * (size_t)n] = (guv[k] + red[0][3 * k + 2][lane]) + (red[1][3 * k + 2][lane] + red[2][3 * k + 2][lane]);
        }
    }
    if (k0 == 0)
        g_all[c * (size_t)n + i] = (g + red[0][3 * kHgKC][lane]) + (red[1][3 * kHgKC][lane] + red[2][3 * kHgKC][lane]);
}

// ---------------------------------------------------------------------------------
// 4. the gradient rows: one lane per flattened (conformation, owner), the owners of a conformation
//    being its N atoms and then its terms, so both kinds close the pass in one launch.
//    An atom: grad[c][i] = the running sum (zero, or what an earlier pass of this conformation's
//    directions left) + g^uv_i of the pass's rows in ascending k.
//    A term: its geometry from the positions (plain doubles), g of its atoms, then its rows in
//    ascending k: each row's contribution to the term's 2 or 5 gradients is formed and added to the
//    running sums, which start as an atom's does.  grad[c][N + ...] in the order of the cf_params
//    arrays: bonds (k, b), angles (k, theta0), waters (k1, k2, kub, b0, ub0).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bhg_rows(int nconf, int kv, int n, int nterms, int nb, int na, int ngeo,
                                                  long np, int first, const int4* __restrict__ tidx,
                                                  const double* __restrict__ tpar, const double* __restrict__ pos_all,
                                                  const double* __restrict__ g_all, const double* __restrict__ gt_all,
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
    const int a1 = ti.y, a2 = ti.z, a3 = ti.x == 0 ? ti.z : ti.w;
    double x1[3], x2[3], x3[3], gam[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 3; j++) { x1[j] = pos[3 * a1 + j]; x2[j] = pos[3 * a2 + j]; x3[j] = pos[3 * a3 + j]; }
    term_gammas<double>(ti.x, x1, x2, x3, gam);
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
// most six launches
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }
static inline size_t ngeom(const Handle& h) { return (size_t)h.nb + (size_t)h.na + 3 * (size_t)h.nw; }

int batch_hvp_grad_chunk() { return kHgKC; }

void launch_batch_hvp_qtan(Handle& h, int rows, const double* gam, double* qt) {
    hipLaunchKernelGGL(k_bhg_qtan, dim3(nblk(h.n, 256), rows), dim3(256), 0, h.stream, h.n, h.nb, h.na, (int)ngeom(h),
                       h.term_par, h.qcsr_start, h.qcsr_slot, gam, qt);
}

size_t batch_hvp_grad_doubles_per_row(const Handle& h) {
    // the geometries' three tangents, (q^u, q^v, q^uv)[N], (g^u, g^v, g^uv)[N], g[N]
    return 3 * ngeom(h) + 7 * (size_t)h.n;
}

void batch_hvp_grad_carve(const Handle& h, double* base, int cap, BatchHvpGradWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n;
    w.base = base; w.cap = cap;
    w.gam = base;
    w.qt = w.gam + c * 3 * ngeom(h);
    w.gt = w.qt + c * 3 * n;
    w.g = w.gt + c * 3 * n;
}

void launch_batch_hvp_vjp(Handle& h, const BatchWs& w, const BatchHvpGradWs& gw, int nconf, int kv, const double* pos,
                          const double* vec, const double* out_bar, long vstride, bool first, double* grad) {
    const int64_t rows64 = (int64_t)nconf * kv;
    if (nconf <= 0 || kv <= 0 || nconf > w.cap || rows64 > gw.cap || rows64 > kBatchMaxPass)
        throw std::invalid_argument("launch_batch_hvp_vjp: pass size");
    const int n = h.n, rows = (int)rows64, ngeo = (int)ngeom(h);
    const long np = (long)n + 2L * h.nb + 2L * h.na + 5L * h.nw;
    const int nchunks = nblk(kv, kHgKC);
    launch_batch_flux_charges(h, w, nconf, pos, nullptr);
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bhg_geom, dim3(nblk((int64_t)rows * h.nterms, 256)), dim3(256), 0, h.stream, rows, kv, n,
                           h.nterms, h.nb, h.na, ngeo, h.term_idx, pos, vec, out_bar, vstride, gw.gam);
    launch_batch_hvp_qtan(h, rows, gw.gam, gw.qt);
    hipLaunchKernelGGL(k_bhg_pairs, dim3(nblk(n, kHgI), nconf * nchunks), dim3(256), 0, h.stream, n, kv, nchunks, h.ke,
                       pos, w.q, vec, out_bar, vstride, gw.qt, h.ex_start, h.ex_list, gw.g, gw.gt);
    hipLaunchKernelGGL(k_bhg_rows, dim3(nblk((int64_t)nconf * (n + h.nterms), 256)), dim3(256), 0, h.stream, nconf, kv, n,
                       h.nterms, h.nb, h.na, ngeo, np, first ? 1 : 0, h.term_idx, h.term_par, pos, gw.g, gw.gt, gw.gam,
                       grad);
}

}  // namespace cf
