// cf_kernels_batch.hip -- cf_compute_batch: B conformations of one non-periodic system in a fixed
// number of launches ("batched").  The four stages of the single evaluation
// (k_flux_terms, k_atoms_prep, k_nopbc, k_assemble_energy in cf_kernels_core.hip) with the
// conformation as blockIdx.y (flux terms: folded into blockIdx.x), so that a batch of small
// clusters fills the chip instead of running
// one workgroup at a time.  The topology (term table, CSR gathers, exclusions, LJ, base charges)
// is the handle's, shared by every conformation; positions, outputs and the workspace are
// conformation-major.
//
// Numerics: fp64, no atomics.  Every per-atom sum and every energy is added in an order that
// depends only on the system (N and the topology), never on the batch: a conformation's results
// are bitwise the same alone, in any batch and under any chunking.
//
// Every index used here is topological (validated by cf_create) or derived from blockIdx /
// threadIdx against n, nterms and the launch's own nconf: no data-dependent index, so no device
// guard bits.
#include <algorithm>
#include <stdexcept>

#include "cf_flux.h"

namespace cf {

// ---------------------------------------------------------------------------------
// 1. flux terms: one lane per (conformation, term); the block's dq/dx blocks staged in LDS and
//    written as one coalesced run, as k_flux_terms
// ---------------------------------------------------------------------------------
//    The (conformation, term) pairs are flattened, g = c * nterms + t, so that a system with few
//    terms still fills its blocks; dq/dx is [conformation][D * 3], and a conformation's terms end
//    where the next one's begin, so a block's output is one contiguous run across conformations.
__global__ void __launch_bounds__(256) k_b_flux(int nconf, int n, int nterms, int nb, int na, int nslots, long nd3,
                                                const int4* __restrict__ tidx, const double* __restrict__ tpar,
                                                const double* __restrict__ pos_all, double* __restrict__ dq_slot_all,
                                                double* __restrict__ dqdx_all) {
    __shared__ double st[256 * 27];
    batch_flux_block<false>(nconf, n, nterms, nb, na, nslots, nd3, tidx, tpar, pos_all, nullptr, 0, dq_slot_all,
                            dqdx_all, st);
}

// ---------------------------------------------------------------------------------
// 2. charges: one lane per (conformation, atom), the slot gather of k_atoms_prep (the same
//    order: the same bits as cf_compute's charges)
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_b_charges(int n, int nslots, const double* __restrict__ q0,
                                                   const int* __restrict__ qs, const int* __restrict__ qslot,
                                                   const double* __restrict__ dq_slot_all, double* __restrict__ q_all,
                                                   double* __restrict__ charges_out) {
    const size_t c = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* dq_slot = dq_slot_all + c * (size_t)nslots;
    double qi = q0[i];
    for (int s = qs[i]; s < qs[i + 1]; s++) qi += dq_slot[qslot[s]];
    q_all[c * (size_t)n + i] = qi;
    if (charges_out) charges_out[c * (size_t)n + i] = qi;
}

// ---------------------------------------------------------------------------------
// 3. all pairs (RCK:436-491, excluded pairs skipped as in k_nopbc).  A block is kBatchI = 64
//    i-atoms of one conformation, one per lane, in each of its four waves; the j-atoms pass
//    through LDS in tiles of 256 and wave w takes entries [64 w, 64 w + 64) of every tile (every
//    lane of a wave reads the same entry: an LDS broadcast).  The four waves' partial sums are
//    added in the fixed order (w0 + w1) + (w2 + w3).  A 256-atom conformation is 4 workgroups
//    of 4 waves (k_nopbc: one workgroup, each lane walking all 256 partners).
// ---------------------------------------------------------------------------------
constexpr int kBatchI = 64;
constexpr int kBatchJ = 256;

__global__ void __launch_bounds__(kBatchJ) k_b_pairs(int n, int include_forces, int include_energy, double ke,
                                                     const double* __restrict__ pos_all, const double* __restrict__ q_all,
                                                     const double2* __restrict__ lj, const int* __restrict__ ex_start,
                                                     const int* __restrict__ ex_list, double* __restrict__ dedq_all,
                                                     double* __restrict__ f_part_all, double* __restrict__ e_atom_all) {
    __shared__ double4 sp[kBatchJ];
    __shared__ double2 sl[kBatchJ];
    __shared__ double red[3][5][kBatchI];   // partial sums of waves 1..3
    const size_t c = blockIdx.y;
    const double* pos = pos_all + c * 3 * (size_t)n;
    const double* q = q_all + c * (size_t)n;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kBatchI + lane;
    const bool active = i < n;
    double4 pi = make_double4(0, 0, 0, 0);
    double2 li = make_double2(0, 0);
    int ex0 = 0, exc = 0;
    int reg[kMaxRegExcl];
    if (active) {
        pi = make_double4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], q[i]);
        li = lj[i];
        ex0 = ex_start[i]; exc = ex_start[i + 1] - ex0;
    }
#pragma unroll
    for (int k = 0; k < kMaxRegExcl; k++) reg[k] = k < exc ? ex_list[ex0 + k] : -1;
    double fx = 0, fy = 0, fz = 0, dq = 0, e = 0;
    for (int base = 0; base < n; base += kBatchJ) {
        const int j = base + threadIdx.x;
        __syncthreads();
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
            if (exc && in_excl(jj, reg, exc, ex_list, ex0)) continue;
            const double4 pj = sp[t];
            const double2 lj2 = sl[t];
            const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;  // getDeltaR(i, j)
            nopbc_pair(dx, dy, dz, pi.w, pj.w, li, lj2, ke, include_forces, include_energy, fx, fy, fz, dq, e);
        }
    }
    if (w > 0) {
        red[w - 1][0][lane] = fx; red[w - 1][1][lane] = fy; red[w - 1][2][lane] = fz;
        red[w - 1][3][lane] = dq; red[w - 1][4][lane] = e;
    }
    __syncthreads();
    if (w > 0 || !active) return;
    e = (e + red[0][4][lane]) + (red[1][4][lane] + red[2][4][lane]);
    e_atom_all[c * (size_t)n + i] = e;
    if (include_forces) {
        fx = (fx + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
        fy = (fy + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
        fz = (fz + red[0][2][lane]) + (red[1][2][lane] + red[2][2][lane]);
        dq = (dq + red[0][3][lane]) + (red[1][3][lane] + red[2][3][lane]);
        dedq_all[c * (size_t)n + i] = dq;
        double* f = f_part_all + c * 3 * (size_t)n + 3 * (size_t)i;
        f[0] = fx; f[1] = fy; f[2] = fz;
    }
}

// ---------------------------------------------------------------------------------
// 4. chain rule + energy.  Per (conformation, atom b): F_b += F_part_b - sum_e dE/dq[a_e]
//    dq_{a_e}/dx_b over the shared ccsr topology in entry order (k_assemble_energy's gather), with
//    this conformation's dE/dq and dq/dx.  The first block of every conformation also sums the
//    conformation's per-atom energies: thread t adds atoms t, t + 256, ... in order, then a
//    butterfly within each wave and the four waves in wave order -- one block, so no tickets
//    and nothing that depends on block scheduling.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_b_assemble(int n, long nd3, const int* __restrict__ cs,
                                                    const int2* __restrict__ ce, const double* __restrict__ dedq_all,
                                                    const double* __restrict__ dqdx_all,
                                                    const double* __restrict__ f_part_all, double* __restrict__ out_all,
                                                    const double* __restrict__ e_atom_all, int include_energy,
                                                    double* __restrict__ energy_out) {
    __shared__ double red[4];
    const size_t c = blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (out_all && b < n) {
        const double* dedq = dedq_all + c * (size_t)n;
        const double* dqdx = dqdx_all + c * (size_t)nd3;
        const double* f_part = f_part_all + c * 3 * (size_t)n;
        double* out = out_all + c * 3 * (size_t)n;
        double fx = f_part[3 * b], fy = f_part[3 * b + 1], fz = f_part[3 * b + 2];
        chain_rule_atom(b, cs, ce, dedq, dqdx, fx, fy, fz);
        out[3 * b] += fx;
        out[3 * b + 1] += fy;
        out[3 * b + 2] += fz;
    }
    if (blockIdx.x != 0 || !energy_out) return;   // block-uniform
    double a = 0;
    if (include_energy) {
        const double* e_atom = e_atom_all + c * (size_t)n;
        for (int k = threadIdx.x; k < n; k += 256) a += e_atom[k];
    }
    block_sum_256_store(a, red, energy_out + c);
}

// ---------------------------------------------------------------------------------
// launcher: one pass of nconf <= w.cap conformations, at most four launches whatever nconf
// ---------------------------------------------------------------------------------
static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

size_t batch_doubles_per_conf(const Handle& h) {
    // q[N], dq slots, dq/dx, dE/dq[N], F_part[3N], per-atom energies[N]
    return (size_t)h.n + (size_t)h.nslots_dq + 3 * (size_t)h.nd + (size_t)h.n + 3 * (size_t)h.n + (size_t)h.n;
}

void batch_carve(const Handle& h, double* base, int cap, BatchWs& w) {
    const size_t c = (size_t)cap, n = (size_t)h.n;
    w.base = base; w.cap = cap;
    w.q = base;
    w.dq_slot = w.q + c * n;
    w.dqdx = w.dq_slot + c * (size_t)h.nslots_dq;
    w.dedq = w.dqdx + c * 3 * (size_t)h.nd;
    w.f_part = w.dedq + c * n;
    w.e_atom = w.f_part + c * 3 * n;
}

// k_b_charges for nconf conformations (also the charges stage of the periodic batch)
void launch_batch_charges(Handle& h, int nconf, const double* dq_slot, double* q, double* charges) {
    hipLaunchKernelGGL(k_b_charges, dim3(nblk(h.n, 256), nconf), dim3(256), 0, h.stream, h.n, h.nslots_dq, h.q0,
                       h.qcsr_start, h.qcsr_slot, dq_slot, q, charges);
}

void launch_batch_flux_charges(Handle& h, const BatchWs& w, int nconf, const double* pos, double* charges) {
    if (h.nterms > 0)
        hipLaunchKernelGGL(k_b_flux, dim3(nblk((int64_t)nconf * h.nterms, 256)), dim3(256), 0, h.stream, nconf, h.n,
                           h.nterms, h.nb, h.na, h.nslots_dq, 3L * h.nd, h.term_idx, h.term_par, pos, w.dq_slot, w.dqdx);
    launch_batch_charges(h, nconf, w.dq_slot, w.q, charges);
}

void launch_batch(Handle& h, const BatchWs& w, int nconf, const double* pos, int flags, double* forces,
                  double* energy, double* charges) {
    if (nconf <= 0 || nconf > w.cap || nconf > kBatchMaxPass) throw std::invalid_argument("launch_batch: pass size");
    const int n = h.n;
    const bool do_f = (flags & CF_INCLUDE_FORCES) && forces;
    const bool do_e = (flags & CF_INCLUDE_ENERGY) && energy;
    const long nd3 = 3L * h.nd;
    launch_batch_flux_charges(h, w, nconf, pos, charges);
    if (do_f || do_e)
        hipLaunchKernelGGL(k_b_pairs, dim3(nblk(n, kBatchI), nconf), dim3(kBatchJ), 0, h.stream, n, do_f ? 1 : 0,
                           do_e ? 1 : 0, h.ke, pos, w.q, h.lj, h.ex_start, h.ex_list, w.dedq, w.f_part, w.e_atom);
    if (do_f || energy)
        hipLaunchKernelGGL(k_b_assemble, dim3(nblk(n, 256), nconf), dim3(256), 0, h.stream, n, nd3, h.ccsr_start,
                           h.ccsr_ent, w.dedq, w.dqdx, w.f_part, do_f ? forces : nullptr, w.e_atom, do_e ? 1 : 0,
                           energy);
}

}  // namespace cf
