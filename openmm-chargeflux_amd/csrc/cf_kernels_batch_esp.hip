// cf_kernels_batch_esp.hip -- cf_compute_batch_esp and cf_compute_batch_esp_vjp: the electrostatic
// potential the charges of each conformation of a non-periodic batch produce at M probe points, and
// its reverse-mode product with respect to the base charges and the flux parameters (DESIGN.md §4.6,
// "batched, electrostatic potential").  Per conformation, with q the charges after flux
// (k_b_charges: the bits of cf_compute_batch),
//     V_p = ke sum_a q_a / |r_p - x_a|                                            (kJ/mol/e)
// over every atom: no exclusions, no LJ.  A forward pass is k_b_flux, k_b_charges (as they are), then
// k_be_esp.
//
// The VJP differentiates L = sum_p V_bar_p V_p.  With a_i = ke sum_p V_bar_p / r_pi, L's gradient is
// that of sum_i a_i q_i with a fixed: every flux term is a sum of pieces q_a += c_a k (g(x) - ref),
//     dL/d(base charge i) = a_i
//     dL/dk   += (sum_a c_a a_a) (g - ref)
//     dL/dref += -k sum_a c_a a_a
// (k_bd_terms's formulas without the polar-tensor part).  Nothing divides by a parameter (k = 0 is
// legal).  A pass is k_be_adjoint (a into grad[c][0, N), or its per-chunk partial sums), k_be_sum when
// M spans several point chunks, and k_be_terms, which reads a back from grad.
//
// Both pair kernels give the lanes to the POINTS: N is small (3, 24, 70 atoms are what ESP fits use)
// and M is large, so an atom per lane would idle most of a wave.  The atoms are wave-uniform: an LDS
// broadcast in the forward kernel, scalar registers in the adjoint.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N, M and the topology: a point's sum
// runs over the atoms in index order whatever the tiles, an atom's sum over the points in the fixed
// order of its chunk (thread t: points t, t + 256, ...; block_sum_256_store's tree), the chunks in
// index order.  A conformation's results are bitwise the same alone, in any batch and under any pass
// size, and a point's potential does not depend on the other points.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, npts, nterms and the launch's own nconf: no device guard bits.
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

constexpr int kEspTile = 256;          // atoms staged through LDS at a time
constexpr int kEspPpl = 2;             // points a lane holds (forward)
constexpr int kEspAtoms = 8;           // atoms a block of the adjoint accumulates
constexpr int kEspChunk = CF_BATCH_ESP_CHUNK;   // points a block of the adjoint sums
static_assert(kEspChunk % 256 == 0 && kEspChunk <= 4096, "the adjoint's chunk: whole rounds of the block, at most 4096");

// point p of a conformation's [npts][3] (3 p may pass 2^31: ld3 indexes with an int)
__device__ __forceinline__ double3 ld_point(const double* __restrict__ pts, long p) {
    return make_double3(pts[3 * (size_t)p], pts[3 * (size_t)p + 1], pts[3 * (size_t)p + 2]);
}

// ---------------------------------------------------------------------------------
// 1. potentials: grid (point tiles of 256 * kEspPpl, conformations).  Lane t owns points
//    tile + t + 256 u, u < kEspPpl (consecutive lanes, consecutive points), one accumulator each.
//    The conformation's atoms pass through LDS in tiles of 256 as (x, y, z, q): every lane of a wave
//    reads the same entry (a broadcast, no bank conflict), once for its kEspPpl points.  A tail lane
//    clamps its point index and skips the store: the atom loop is block-uniform.  A point's sum runs
//    over the atoms in index order, each pair 3 subtractions, a multiply and 2 FMAs, rsqrt_fp64, an
//    FMA; ke once at the end.  LDS: 256 * 32 = 8192 B.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_be_esp(int n, int npts, double ke, const double* __restrict__ pos_all,
                                                const double* __restrict__ q_all, const double* __restrict__ pts_all,
                                                double* __restrict__ esp_all) {
    __shared__ double4 atom[kEspTile];
    const size_t c = blockIdx.y;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    const double* pts = pts_all + c * 3 * (size_t)npts;
    const long p0 = (long)blockIdx.x * (256 * kEspPpl) + threadIdx.x;
    double3 r[kEspPpl];
    double acc[kEspPpl];
#pragma unroll
    for (int u = 0; u < kEspPpl; u++) {
        r[u] = ld_point(pts, min(p0 + 256L * u, (long)npts - 1));
        acc[u] = 0.0;
    }
    for (int t0 = 0; t0 < n; t0 += kEspTile) {
        const int len = min(kEspTile, n - t0);   // block-uniform
        if ((int)threadIdx.x < len) {
            const double3 x = ld3(pos, t0 + threadIdx.x);
            atom[threadIdx.x] = make_double4(x.x, x.y, x.z, q[t0 + threadIdx.x]);
        }
        __syncthreads();
        for (int j = 0; j < len; j++) {
            const double4 a = atom[j];
#pragma unroll
            for (int u = 0; u < kEspPpl; u++) {
                const double dx = r[u].x - a.x, dy = r[u].y - a.y, dz = r[u].z - a.z;
                const double r2 = fma(dz, dz, fma(dy, dy, dx * dx));
                acc[u] = fma(a.w, rsqrt_fp64(r2), acc[u]);
            }
        }
        __syncthreads();
    }
    double* esp = esp_all + c * (size_t)npts;
#pragma unroll
    for (int u = 0; u < kEspPpl; u++)
        if (p0 + 256L * u < npts) esp[p0 + 256L * u] = ke * acc[u];
}

// ---------------------------------------------------------------------------------
// 2. adjoint weights: grid (atom tiles of kEspAtoms x point chunks, conformations); blockIdx.x =
//    chunk * ntiles + tile.  The tile's atoms are block-uniform (scalar registers; a tail atom clamps
//    its index and is not stored), their kEspAtoms accumulators per lane are VGPRs.  Thread t adds
//    V_bar_p / r_pi over points t, t + 256, ... of the chunk in that order; the block then sums each
//    accumulator in block_sum_256_store's order.  One chunk (part null): ke * sum to grad[c][i].
//    Several: the bare sum to part[c][chunk][i], for k_be_sum.  LDS: 8 * 4 * 8 + 8 * 8 = 320 B.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_be_adjoint(int n, int npts, int ntiles, int nchunks, long np, double ke,
                                                    const double* __restrict__ pos_all,
                                                    const double* __restrict__ pts_all,
                                                    const double* __restrict__ vbar_all, double* __restrict__ part_all,
                                                    double* __restrict__ grad_all) {
    __shared__ double red[kEspAtoms][4];
    __shared__ double sum[kEspAtoms];
    const size_t c = blockIdx.y;
    const int tile = blockIdx.x % ntiles, chunk = blockIdx.x / ntiles;
    const int i0 = tile * kEspAtoms;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* pts = pts_all + c * 3 * (size_t)npts;
    const double* vbar = vbar_all + c * (size_t)npts;
    double3 x[kEspAtoms];
    double acc[kEspAtoms];
#pragma unroll
    for (int k = 0; k < kEspAtoms; k++) {
        x[k] = ld3(pos, min(i0 + k, n - 1));
        acc[k] = 0.0;
    }
    const long first = (long)chunk * kEspChunk;
    const long last = min(first + kEspChunk, (long)npts);
    for (long p = first + threadIdx.x; p < last; p += 256) {
        const double3 r = ld_point(pts, p);
        const double v = vbar[p];
#pragma unroll
        for (int k = 0; k < kEspAtoms; k++) {
            const double dx = r.x - x[k].x, dy = r.y - x[k].y, dz = r.z - x[k].z;
            const double r2 = fma(dz, dz, fma(dy, dy, dx * dx));
            acc[k] = fma(v, rsqrt_fp64(r2), acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < kEspAtoms; k++) block_sum_256_store(acc[k], red[k], &sum[k]);
    __syncthreads();
    const int k = threadIdx.x;
    if (k < kEspAtoms && i0 + k < n) {
        if (part_all)
            part_all[(c * (size_t)nchunks + (size_t)chunk) * (size_t)n + i0 + k] = sum[k];
        else
            grad_all[c * (size_t)np + i0 + k] = ke * sum[k];
    }
}

// ---------------------------------------------------------------------------------
// 3. several chunks: one lane per (conformation, atom) adds the chunks' partial sums in index order
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_be_sum(int n, int nchunks, long np, double ke,
                                                const double* __restrict__ part_all, double* __restrict__ grad_all) {
    const size_t c = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* part = part_all + c * (size_t)nchunks * (size_t)n + i;
    double a = part[0];
    for (int ch = 1; ch < nchunks; ch++) a += part[(size_t)ch * (size_t)n];
    grad_all[c * (size_t)np + i] = ke * a;
}

// ---------------------------------------------------------------------------------
// 4. term gradients: one lane per flattened (conformation, term), g = c * nterms + t.  a of the
//    term's two or three atoms back from grad[c][.], the term's geometry (flux_term's) from the
//    positions, its 2 or 5 gradients into grad[c][N + ...] in the order of the cf_params arrays:
//    bonds (k, b), angles (k, theta0), waters (k1, k2, kub, b0, ub0); the pieces and their c as
//    k_bd_terms.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double dist2(double3 a, double3 b) {
    const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ double dist(double3 a, double3 b) { return sqrt(dist2(a, b)); }

__global__ void __launch_bounds__(256) k_be_terms(int nconf, int n, int nterms, int nb, int na, long np,
                                                  const int4* __restrict__ tidx, const double* __restrict__ tpar,
                                                  const double* __restrict__ pos_all, double* grad_all) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long)nconf * nterms) return;
    const size_t c = (size_t)(gi / nterms);
    const int t = (int)(gi % nterms);
    const int4 ti = tidx[t];
    const double* p = tpar + 5 * t;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* a = grad_all + c * (size_t)np;
    double* out = grad_all + c * (size_t)np + n;
    if (ti.x == 0) {  // bond p1-p2
        const double da = a[ti.y] - a[ti.z];
        const double r = dist(ld3(pos, ti.y), ld3(pos, ti.z));
        out += 2 * t;
        out[0] = da * (r - p[1]);
        out[1] = -p[0] * da;
    } else if (ti.x == 1) {  // angle p1-p2-p3, p2 central
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double wa = a[ti.y] - 2 * a[ti.z] + a[ti.w];
        const double r21_2 = dist2(x2, x1), r23_2 = dist2(x2, x3), r13_2 = dist2(x1, x3);
        const double cost = (r23_2 + r21_2 - r13_2) / 2 / sqrt(r21_2) / sqrt(r23_2);   // flux_term's law-of-cosines cosine
        out += 2 * nb + 2 * (t - nb);
        out[0] = wa * (acos(cost) - p[1]);
        out[1] = -p[0] * wa;
    } else {  // water O,H1,H2
        const double3 x1 = ld3(pos, ti.y), x2 = ld3(pos, ti.z), x3 = ld3(pos, ti.w);
        const double a1 = a[ti.y];
        const double a2 = a[ti.z] - a1, a3 = a[ti.w] - a1;
        const double r12 = dist(x1, x2), r13 = dist(x1, x3), r23 = dist(x2, x3);
        const double b0 = p[3], ub0 = p[4];
        out += 2 * nb + 2 * na + 5 * (t - nb - na);
        out[0] = a2 * (r12 - b0) + a3 * (r13 - b0);
        out[1] = a2 * (r13 - b0) + a3 * (r12 - b0);
        out[2] = (a2 + a3) * (r23 - ub0);
        out[3] = -(p[0] + p[1]) * (a2 + a3);
        out[4] = -p[2] * (a2 + a3);
    }
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
static inline int64_t nblk64(int64_t n, int64_t b) { return (n + b - 1) / b; }

int batch_esp_chunks(int npts) { return (int)nblk64(npts, kEspChunk); }

// one pass of nconf <= w.cap conformations: at most three launches
void launch_batch_esp(Handle& h, const BatchWs& w, int nconf, const double* pos, int npts, const double* points,
                      double* esp, double* charges) {
    if (nconf <= 0 || nconf > w.cap || nconf > kBatchMaxPass) throw std::invalid_argument("launch_batch_esp: pass size");
    if (npts <= 0) throw std::invalid_argument("launch_batch_esp: npts");
    launch_batch_flux_charges(h, w, nconf, pos, charges);
    if (esp)
        hipLaunchKernelGGL(k_be_esp, dim3((unsigned)nblk64(npts, 256 * kEspPpl), nconf), dim3(256), 0, h.stream, h.n, npts,
                           h.ke, pos, w.q, points, esp);
}

// one pass of nconf <= kBatchMaxPass conformations: at most three launches.  part: null when the
// points fit one chunk, else [nconf][chunks][N]
void launch_batch_esp_vjp(Handle& h, int nconf, const double* pos, int npts, const double* points,
                          const double* esp_bar, double* part, double* grad) {
    if (nconf <= 0 || nconf > kBatchMaxPass) throw std::invalid_argument("launch_batch_esp_vjp: pass size");
    if (npts <= 0) throw std::invalid_argument("launch_batch_esp_vjp: npts");
    const int n = h.n;
    const long np = (long)n + 2L * h.nb + 2L * h.na + 5L * h.nw;
    const int nchunks = batch_esp_chunks(npts);
    const int64_t ntiles = nblk64(n, kEspAtoms);
    if (ntiles * nchunks > 0x7fffffffLL) throw std::invalid_argument("launch_batch_esp_vjp: N * npts too large for one grid");
    if ((nchunks > 1) != (part != nullptr)) throw std::invalid_argument("launch_batch_esp_vjp: scratch");
    hipLaunchKernelGGL(k_be_adjoint, dim3((unsigned)(ntiles * nchunks), nconf), dim3(256), 0, h.stream, n, npts,
                       (int)ntiles, nchunks, np, h.ke, pos, points, esp_bar, part, grad);
    if (part)
        hipLaunchKernelGGL(k_be_sum, dim3((unsigned)nblk64(n, 256), nconf), dim3(256), 0, h.stream, n, nchunks, np, h.ke,
                           part, grad);
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_be_terms, dim3((unsigned)nblk64((int64_t)nconf * h.nterms, 256)), dim3(256), 0, h.stream,
                           nconf, n, h.nterms, h.nb, h.na, np, h.term_idx, h.term_par, pos, grad);
}

}  // namespace cf
