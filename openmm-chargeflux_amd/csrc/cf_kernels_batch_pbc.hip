// cf_kernels_batch_pbc.hip -- cf_compute_batch_periodic: B conformations of one periodic system,
// each with its own box, in a fixed number of launches ("batched, periodic").
// Per conformation the result is cf_compute's with that box and the exact k-sum:
//
//   1. k_bp_flux     flux terms with the conformation's box-vector minimum image (batch_flux_block)
//   2. k_b_charges   the slot gather (cf_kernels_batch.hip, as it is)
//   3. k_bp_tables   per-axis phases e^{i m (2 pi / L_a) x_a}, m < kmax_a, of the wrapped coordinates
//   4. k_bp_sfac     S(k) over all atoms per (conformation, k tile) -> coefficients, energy terms
//   5. k_bp_pairs    all pairs by minimum image within the cutoff (erfc table in LDS), the erf
//                    correction for excluded partners, the self term
//   6. k_bp_recip    per-atom reciprocal force and dE/dq over all k (coefficients in LDS)
//   7. k_bp_assemble chain rule + the conformation's energy
//
// No cell list, no neighbour list: at the target sizes (up to ~2000 atoms per box, thousands of
// boxes) all pairs fills the chip and needs no sort or build launches.  Larger systems are correct
// through the tile loops, not fast.
//
// Numerics: fp64, no atomics.  Every sum's order depends only on N, the topology and kmax, never
// on the batch: a conformation's results are bitwise the same alone, at any position of any batch
// and under any pass size.  Every index is topological (validated by cf_create) or derived from
// blockIdx / threadIdx against n, nterms, khalf and the launch's own nconf: no data-dependent
// index, so no device guard bits.
#include <algorithm>
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

// ---------------------------------------------------------------------------------
// 1. flux terms: k_b_flux with the conformation's L, T and pbc = 1 (the T != 0 branch of delta_r
//    is per conformation here: a batch may mix orthorhombic and triclinic boxes).  pbc is a kernel
//    argument (always 1), not a compile-time constant: with the branch structure of k_flux_terms
//    the compiler contracts the term bodies into the same FMAs, and the charges come out with
//    cf_compute's bits (as a constant, ~5 % of them differed in the last place)
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bp_flux(int nconf, int n, int nterms, int nb, int na, int nslots, long nd3,
                                                 const int4* __restrict__ tidx, const double* __restrict__ tpar,
                                                 const double* __restrict__ pos_all, const double* __restrict__ boxes,
                                                 int pbc, double* __restrict__ dq_slot_all,
                                                 double* __restrict__ dqdx_all) {
    __shared__ double st[256 * 27];
    batch_flux_block<true>(nconf, n, nterms, nb, na, nslots, nd3, tidx, tpar, pos_all, boxes, pbc, dq_slot_all, dqdx_all,
                           st);
}

// ---------------------------------------------------------------------------------
// 3. phase tables: one lane per (conformation, atom, entry); row of atom i = [X_0..X_{KX-1} |
//    Y_0..Y_{KY-1} | Z_0..Z_{KZ-1}], entry m of axis a = (cos, sin)(m (2 pi / L_a) xw_a) with xw_a
//    the coordinate wrapped into [0, L_a) by the box DIAGONAL (the reference's reciprocal part reads
//    only the diagonals, RCK:513-517, also for a triclinic box): the factor is unchanged and the
//    sincos argument stays below 2 pi kmax.  Written twice: atom-major [N][KS] for k_bp_sfac (a
//    wave's 64 k-vectors read one atom's row: 2-3 cache lines) and entry-major [KS][N] for
//    k_bp_recip (a wave's 64 atoms read one entry: coalesced; from the atom-major copy every lane
//    touched its own cache line and the kernel took 62 % of the batch)
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bp_tables(long total, int n, int KX, int KY, int KZ,
                                                   const double* __restrict__ pos_all,
                                                   const double* __restrict__ boxes, double2* __restrict__ tab_all,
                                                   double2* __restrict__ tab_t_all) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int KS = KX + KY + KZ;
    const long per = (long)n * KS;
    const size_t c = (size_t)(g / per);
    const long r = g % per;
    const int i = (int)(r / KS);
    int m = (int)(r % KS);
    const size_t gt = c * (size_t)per + (size_t)m * n + i;   // the entry-major copy's slot
    int axis = 0;
    if (m >= KX) { m -= KX; axis = 1; }
    if (axis == 1 && m >= KY) { m -= KY; axis = 2; }
    const double x = pos_all[c * 3 * (size_t)n + 3 * (size_t)i + axis];
    const double L = boxes[8 * c + axis];
    const double xw = x - L * floor(x / L);
    double s, co;
    sincos((m * (2.0 * kPi / L)) * xw, &s, &co);
    tab_all[g] = make_double2(co, s);
    tab_t_all[gt] = make_double2(co, s);
}

// ---------------------------------------------------------------------------------
// 4. structure factor: one lane per (conformation, k) of the reference's half-space set
//    (half_space_k), summed over the atoms in atom order (RCK:523-531).  Output per k:
//    coef = 2 c eak (Re S, Im S) for the force stage and ek = c eak |S|^2 for the energy,
//    c = 4 pi ke / V, eak = exp(-k^2 / 4 alpha^2) / k^2 with the conformation's box diagonals.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bp_sfac(int n, int KX, int KY, int KZ, long khalf, double ke, double one_a2,
                                                 const double* __restrict__ boxes, const double* __restrict__ q_all,
                                                 const double2* __restrict__ tab_all, double2* __restrict__ coef_all,
                                                 double* __restrict__ ek_all) {
    const size_t c = blockIdx.y;
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= khalf) return;
    int nx, ny, nz;
    half_space_k(k, KY, KZ, nx, ny, nz);
    const int KS = KX + KY + KZ;
    const double2* row = tab_all + c * (size_t)n * KS;
    const double* q = q_all + c * (size_t)n;
    double cs = 0, ss = 0;
    for (int i = 0; i < n; i++) {
        const double2 e = phase(row + (size_t)i * KS, 1, KX, KY, nx, ny, nz);
        const double qi = q[i];
        cs += qi * e.x;
        ss += qi * e.y;
    }
    double3 L, T;
    load_box(boxes, c, L, T);
    const double kx = nx * (2.0 * kPi / L.x), ky = ny * (2.0 * kPi / L.y), kz = nz * (2.0 * kPi / L.z);
    const double k2 = kx * kx + ky * ky + kz * kz;
    const double eak = exp(-k2 * 0.25 * one_a2) / k2;
    const double cst = 4.0 / L.x / L.y / L.z * kPi * ke;   // RCK:517
    coef_all[c * (size_t)khalf + k] = make_double2(2.0 * cst * eak * cs, 2.0 * cst * eak * ss);
    ek_all[c * (size_t)khalf + k] = cst * eak * (cs * cs + ss * ss);
}

// ---------------------------------------------------------------------------------
// 5. direct space, in the shape of k_b_pairs: a block is kPbcI = 64 i-atoms of one conformation,
//    one per lane, in each of its four waves; the j-atoms pass through LDS in tiles of 256 and
//    wave w takes entries [64 w, 64 w + 64) of every tile.  Per pair: delta_r minimum image with
//    the conformation's box, then an excluded partner gets the erf correction (any distance, no
//    cutoff test: k_excl), any other partner within the cutoff the erfc pair term (ewald_pair,
//    the handle's erfcx table in LDS).  The four waves' partial sums are added as
//    (w0 + w1) + (w2 + w3), then the self term: per atom F, dE/dq and energy
//    (self + direct / 2 + exclusion).
// ---------------------------------------------------------------------------------
constexpr int kPbcI = 64;
constexpr int kPbcJ = 256;

__global__ void __launch_bounds__(kPbcJ) k_bp_pairs(int n, int include_forces, double ke, double alpha, double rc2,
                                                    double erfc_scale, const double* __restrict__ erfc_tab,
                                                    const double* __restrict__ boxes,
                                                    const double* __restrict__ pos_all, const double* __restrict__ q_all,
                                                    const double2* __restrict__ lj, const int* __restrict__ ex_start,
                                                    const int* __restrict__ ex_list, double* __restrict__ dedq_all,
                                                    double* __restrict__ f_part_all, double* __restrict__ e_atom_all) {
    __shared__ double tab[kErfcMaxM * (kErfcDeg + 1)];
    __shared__ double4 sp[kPbcJ];
    __shared__ double2 sl[kPbcJ];
    __shared__ double red[3][6][kPbcI];   // partial sums of waves 1..3
    for (int e = threadIdx.x; e < kErfcMaxM * (kErfcDeg + 1); e += kPbcJ) tab[e] = erfc_tab[e];
    const size_t c = blockIdx.y;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    double3 L, T;
    load_box(boxes, c, L, T);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kPbcI + lane;
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
    double ex_e = 0;
    for (int base = 0; base < n; base += kPbcJ) {
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
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) {
                CF_EXCL_PAIR(ke, alpha, include_forces, qi, pj.w, d, acc.fx, acc.fy, acc.fz, acc.dq, ex_e)
                continue;
            }
            const double r2 = d.x * d.x + d.y * d.y + d.z * d.z;
            if (r2 <= rc2) ewald_pair(acc, ke, alpha, erfc_scale, include_forces, tab, qi, li, pj.w, sl[t], d.x, d.y, d.z, r2);
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = acc.fx; red[w - 1][1][lane] = acc.fy; red[w - 1][2][lane] = acc.fz;
        red[w - 1][3][lane] = acc.dq; red[w - 1][4][lane] = acc.e; red[w - 1][5][lane] = ex_e;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    const double cself = ke * alpha / sqrt(kPi);   // RCK:507-510
    const double e = (acc.e + red[0][4][lane]) + (red[1][4][lane] + red[2][4][lane]);
    ex_e = (ex_e + red[0][5][lane]) + (red[1][5][lane] + red[2][5][lane]);
    e_atom_all[c * (size_t)n + i] = (-cself * qi * qi + 0.5 * e) + ex_e;
    if (include_forces) {
        const double fx = (acc.fx + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
        const double fy = (acc.fy + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
        const double fz = (acc.fz + red[0][2][lane]) + (red[1][2][lane] + red[2][2][lane]);
        const double dq = (acc.dq + red[0][3][lane]) + (red[1][3][lane] + red[2][3][lane]);
        dedq_all[c * (size_t)n + i] = -2 * cself * qi + dq;
        double* f = f_part_all + c * 3 * (size_t)n + 3 * (size_t)i;
        f[0] = fx; f[1] = fy; f[2] = fz;
    }
}

// ---------------------------------------------------------------------------------
// 6. reciprocal force and dE/dq (RCK:533-545): 64 atoms per block, one per lane, in each of the
//    four waves; the k-vectors pass through LDS in tiles of 256 (coefficient 2 c eak S(k) and the
//    integer triple) and wave w takes entries [64 w, 64 w + 64) of every tile.  The partial sums
//    are added as (w0 + w1) + (w2 + w3) and then to the pair kernel's dE/dq and F (this lane's own
//    atom: a plain read-modify-write).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bp_recip(int n, int KX, int KY, int KZ, long khalf,
                                                  const double* __restrict__ boxes, const double* __restrict__ q_all,
                                                  const double2* __restrict__ tab_t_all,
                                                  const double2* __restrict__ coef_all, double* __restrict__ dedq_all,
                                                  double* __restrict__ f_part_all) {
    __shared__ double2 sc[256];
    __shared__ int4 sn[256];
    __shared__ double red[3][4][64];
    const size_t c = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const bool active = i < n;
    const int KS = KX + KY + KZ;
    const double2* row = tab_t_all + c * (size_t)n * KS + (active ? i : 0);   // entry m at row[m * n]
    const double2* coef = coef_all + c * (size_t)khalf;
    double t0 = 0, gx = 0, gy = 0, gz = 0;
    for (long base = 0; base < khalf; base += 256) {
        const long k = base + threadIdx.x;
        __syncthreads();
        if (k < khalf) {
            int nx, ny, nz;
            half_space_k(k, KY, KZ, nx, ny, nz);
            sc[threadIdx.x] = coef[k];
            sn[threadIdx.x] = make_int4(nx, ny, nz, 0);
        }
        __syncthreads();
        const int t1 = (int)min((long)(64 * w + 64), khalf - base);
        if (!active) continue;
        for (int t = 64 * w; t < t1; t++) {
            const double2 ab = sc[t];
            const int4 nn = sn[t];
            const double2 e = phase(row, (size_t)n, KX, KY, nn.x, nn.y, nn.z);
            t0 += ab.x * e.x + ab.y * e.y;
            const double g = ab.x * e.y - ab.y * e.x;
            gx += g * nn.x; gy += g * nn.y; gz += g * nn.z;
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = t0; red[w - 1][1][lane] = gx; red[w - 1][2][lane] = gy; red[w - 1][3][lane] = gz;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    t0 = (t0 + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
    gx = (gx + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
    gy = (gy + red[0][2][lane]) + (red[1][2][lane] + red[2][2][lane]);
    gz = (gz + red[0][3][lane]) + (red[1][3][lane] + red[2][3][lane]);
    double3 L, T;
    load_box(boxes, c, L, T);
    const double qi = q_all[c * (size_t)n + i];
    dedq_all[c * (size_t)n + i] += t0;
    double* f = f_part_all + c * 3 * (size_t)n + 3 * (size_t)i;
    f[0] += qi * (gx * (2.0 * kPi / L.x));
    f[1] += qi * (gy * (2.0 * kPi / L.y));
    f[2] += qi * (gz * (2.0 * kPi / L.z));
}

// ---------------------------------------------------------------------------------
// 7. chain rule + energy: k_b_assemble's gather (chain_rule_atom).  The first block of every
//    conformation sums its energy: thread t adds the per-atom energies (self + direct +
//    exclusion) of atoms t, t + 256, ... and, with include_recip, the reciprocal terms of k-vectors
//    t, t + 256, ..., then block_sum_256_store.  The reference's quirk (RCK:507-633): the atom part is
//    accumulated whatever the flags, the reciprocal part only with CF_INCLUDE_ENERGY.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bp_assemble(int n, long nd3, long khalf, const int* __restrict__ cs,
                                                     const int2* __restrict__ ce, const double* __restrict__ dedq_all,
                                                     const double* __restrict__ dqdx_all,
                                                     const double* __restrict__ f_part_all, double* __restrict__ out_all,
                                                     const double* __restrict__ e_atom_all,
                                                     const double* __restrict__ ek_all, int include_recip,
                                                     double* __restrict__ energy_out) {
    __shared__ double red[4];
    const size_t c = blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (out_all && b < n) {
        const double* f_part = f_part_all + c * 3 * (size_t)n;
        double* out = out_all + c * 3 * (size_t)n;
        double fx = f_part[3 * b], fy = f_part[3 * b + 1], fz = f_part[3 * b + 2];
        chain_rule_atom(b, cs, ce, dedq_all + c * (size_t)n, dqdx_all + c * (size_t)nd3, fx, fy, fz);
        out[3 * b] += fx;
        out[3 * b + 1] += fy;
        out[3 * b + 2] += fz;
    }
    if (blockIdx.x != 0 || !energy_out) return;   // block-uniform
    double a = 0, r = 0;
    const double* e_atom = e_atom_all + c * (size_t)n;
    for (int k = threadIdx.x; k < n; k += 256) a += e_atom[k];
    if (include_recip) {
        const double* ek = ek_all + c * (size_t)khalf;
        for (long k = threadIdx.x; k < khalf; k += 256) r += ek[k];
    }
    block_sum_256_store(a + r, red, energy_out + c);
}

// ---------------------------------------------------------------------------------
// launcher: one pass of nconf <= w.cap conformations, at most seven launches whatever nconf
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

size_t batch_pbc_doubles_per_conf(const Handle& h) {
    const size_t n = (size_t)h.n, ks = (size_t)h.kmax[0] + h.kmax[1] + h.kmax[2], kh = (size_t)h.khalf;
    // phases [N][KS] x 2 in both layouts, coefficients [khalf] x 2, energy terms [khalf], then as the
    // non-periodic batch: q[N], dq slots, dq/dx, dE/dq[N], F_part[3N], per-atom energies[N]
    return 4 * n * ks + 2 * kh + kh + n + (size_t)h.nslots_dq + 3 * (size_t)h.nd + n + 3 * n + n;
}

void batch_pbc_carve(const Handle& h, double* base, int cap, BatchPbcWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n, ks = (size_t)h.kmax[0] + h.kmax[1] + h.kmax[2];
    const size_t kh = (size_t)h.khalf;
    w.base = base; w.cap = cap;
    w.tab = reinterpret_cast<double2*>(base);
    w.tab_t = w.tab + c * n * ks;
    w.coef = w.tab_t + c * n * ks;
    w.ek = reinterpret_cast<double*>(w.coef + c * kh);
    w.q = w.ek + c * kh;
    w.dq_slot = w.q + c * n;
    w.dqdx = w.dq_slot + c * (size_t)h.nslots_dq;
    w.dedq = w.dqdx + c * 3 * (size_t)h.nd;
    w.f_part = w.dedq + c * n;
    w.e_atom = w.f_part + c * 3 * n;
}

void launch_batch_pbc_flux_charges(Handle& h, const BatchPbcWs& w, int nconf, const double* pos, const double* boxes,
                                   double* charges) {
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_bp_flux, dim3(nblk((int64_t)nconf * h.nterms, 256)), dim3(256), 0, h.stream, nconf, h.n,
                           h.nterms, h.nb, h.na, h.nslots_dq, 3L * h.nd, h.term_idx, h.term_par, pos, boxes, h.pbc,
                           w.dq_slot, w.dqdx);
    launch_batch_charges(h, nconf, w.dq_slot, w.q, charges);
}

void launch_batch_pbc_tables(Handle& h, const BatchPbcWs& w, int nconf, const double* pos, const double* boxes) {
    const int KX = h.kmax[0], KY = h.kmax[1], KZ = h.kmax[2];
    const long total = (long)nconf * h.n * (KX + KY + KZ);
    hipLaunchKernelGGL(k_bp_tables, dim3(nblk(total, 256)), dim3(256), 0, h.stream, total, h.n, KX, KY, KZ, pos, boxes,
                       w.tab, w.tab_t);
}

void launch_batch_pbc(Handle& h, const BatchPbcWs& w, int nconf, const double* pos, const double* boxes, int flags,
                      double* forces, double* energy, double* charges) {
    if (nconf <= 0 || nconf > w.cap || nconf > kBatchMaxPass) throw std::invalid_argument("launch_batch_pbc: pass size");
    const int n = h.n;
    const int KX = h.kmax[0], KY = h.kmax[1], KZ = h.kmax[2];
    const long khalf = (long)h.khalf;
    const bool do_f = (flags & CF_INCLUDE_FORCES) && forces;
    const bool do_er = (flags & CF_INCLUDE_ENERGY) && energy;   // the reciprocal energy (the rest: whatever the flags)
    const long nd3 = 3L * h.nd;
    launch_batch_pbc_flux_charges(h, w, nconf, pos, boxes, charges);
    if (do_f || do_er) {
        launch_batch_pbc_tables(h, w, nconf, pos, boxes);
        hipLaunchKernelGGL(k_bp_sfac, dim3(nblk(khalf, 256), nconf), dim3(256), 0, h.stream, n, KX, KY, KZ, khalf, h.ke,
                           1.0 / (h.alpha * h.alpha), boxes, w.q, w.tab, w.coef, w.ek);
    }
    if (do_f || energy)
        hipLaunchKernelGGL(k_bp_pairs, dim3(nblk(n, kPbcI), nconf), dim3(kPbcJ), 0, h.stream, n, do_f ? 1 : 0, h.ke,
                           h.alpha, h.cutoff * h.cutoff, h.erfc_scale, h.erfc_tab, boxes, pos, w.q, h.lj, h.ex_start,
                           h.ex_list, w.dedq, w.f_part, w.e_atom);
    if (do_f)
        hipLaunchKernelGGL(k_bp_recip, dim3(nblk(n, 64), nconf), dim3(256), 0, h.stream, n, KX, KY, KZ, khalf, boxes, w.q,
                           w.tab_t, w.coef, w.dedq, w.f_part);
    if (do_f || energy)
        hipLaunchKernelGGL(k_bp_assemble, dim3(nblk(n, 256), nconf), dim3(256), 0, h.stream, n, nd3, khalf,
                           h.ccsr_start, h.ccsr_ent, w.dedq, w.dqdx, w.f_part, do_f ? forces : nullptr, w.e_atom, w.ek,
                           do_er ? 1 : 0, energy);
}

}  // namespace cf
