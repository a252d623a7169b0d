/*
 * chargeflux.h — C-ABI boundary of the MI355X-native ChargeFlux (CoulForce) evaluator.
 *
 * This is the drop-in boundary for the reference's hot path
 *   CoulPlugin::CalcCoulForceKernel::{initialize, execute}
 *   (reference: openmmapi/include/CoulKernels.h:15-38,
 *    platforms/reference/src/ReferenceCoulKernels.cpp:230-636).
 *
 * Plain C: pointers, sizes and int error codes only.  No C++ exceptions, no torch
 * types cross it.  An OpenMM plugin or a ctypes/cffi binding
 * calls these functions; the Python mirror `openmmcoul` in this repo does exactly that.
 *
 * Units follow the reference (OpenMM): nm, e, kJ/mol, rad.  All arithmetic is fp64.
 */
#ifndef CHARGEFLUX_H_
#define CHARGEFLUX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define CF_EXPORT __declspec(dllexport)
#else
#define CF_EXPORT __attribute__((visibility("default")))
#endif

#define CF_API_VERSION 4   /* 2: cf_params.one_4pi_eps0; 3: cf_options.handover, pair_list, variants, list_capacity;
                              4: device index guards (cf_get_device_errors), cf_compute_openmm, octant list removed;
                              still 4 (purely additive): cf_compute_batch, cf_compute_batch_host,
                              cf_set_batch_limit, cf_get_batch_stats; cf_compute_batch_periodic,
                              cf_compute_batch_periodic_host; cf_get_param_counts, cf_compute_batch_vjp,
                              cf_compute_batch_vjp_host; cf_compute_batch_periodic_vjp,
                              cf_compute_batch_periodic_vjp_host; cf_compute_batch_lj_vjp,
                              cf_compute_batch_lj_vjp_host; cf_compute_batch_dipole,
                              cf_compute_batch_dipole_host, cf_compute_batch_dipole_vjp,
                              cf_compute_batch_dipole_vjp_host; cf_compute_batch_hvp,
                              cf_compute_batch_hvp_host */

/* Error codes (negative).  cf_last_error() returns the message of the last failure
 * on the calling thread.  Mirrors the reference's OpenMMException paths. */
#define CF_OK 0
#define CF_ERR_INVALID -1  /* bad argument / parameter validation failed     */
#define CF_ERR_HIP -2      /* a HIP runtime call failed                       */
#define CF_ERR_STATE -3    /* call sequence error (e.g. end without begin)    */
#define CF_ERR_NOMEM -4    /* device allocation failed                        */

/* Coulomb constant ONE_4PI_EPS0 (kJ mol^-1 nm e^-2).  The reference takes it from the
 * OpenMM it is compiled against (openmm/reference/SimTKOpenMMRealType.h, included at
 * ReferenceCoulKernels.cpp:7; used at :508, :517, :580-589, :608-619), so its value depends on
 * the OpenMM version: 138.935456 in OpenMM 7.x headers, 138.93545764438198 (CODATA 2018) in
 * OpenMM 8.x.  cf_params.one_4pi_eps0 carries the loading OpenMM's value; 0 selects the
 * default below (OpenMM 7.x). */
#define CF_ONE_4PI_EPS0 138.935456
#define CF_ONE_4PI_EPS0_CODATA2018 138.93545764438198

/*
 * Force parameters: the flat storage of CoulPlugin::CoulForce
 * (reference: openmmapi/include/CoulForce.h:138-149, openmmapi/src/CoulForce.cpp:12-140).
 * Arrays are host memory, read only during cf_create.
 */
typedef struct cf_params {
    int32_t num_particles;
    const double* charges;  /* [N]  addParticle(charge, ...)          CoulForce.cpp:18-22 */
    const double* sigmas;   /* [N]  LJ sigma (nm)                                          */
    const double* epsilons; /* [N]  LJ epsilon (kJ/mol)                                    */

    int32_t num_exceptions;
    const int32_t* exceptions; /* [2E] excluded pairs (p1,p2)         CoulForce.cpp:56-68 */

    int32_t num_flux_bonds;
    const int32_t* flux_bond_idx;    /* [2B] (p1,p2)                  CoulForce.cpp:78-94   */
    const double* flux_bond_params;  /* [2B] (k [e/nm], b [nm])                             */
    int32_t num_flux_angles;
    const int32_t* flux_angle_idx;   /* [3A] (p1,p2,p3), p2 central   CoulForce.cpp:96-114  */
    const double* flux_angle_params; /* [2A] (k [e/rad], theta0 [rad])                      */
    int32_t num_flux_waters;
    const int32_t* flux_water_idx;   /* [3W] (O,H1,H2)                CoulForce.cpp:116-140 */
    const double* flux_water_params; /* [5W] (k1,k2,kub [e/nm], b0,ub0 [nm])                */

    int32_t use_pbc;          /* setUsesPeriodicBoundaryConditions   CoulForce.cpp:52-54   */
    double cutoff;            /* setCutoffDistance (nm), PBC only                          */
    double ewald_tol;         /* setEwaldErrorTolerance                                    */
    double default_box[9];    /* System::getDefaultPeriodicBoxVectors, rows a,b,c (nm);
                                 kmax is derived from THIS box (ReferenceCoulKernels.cpp:399-420) */
    double one_4pi_eps0;      /* Coulomb constant of the OpenMM the force is evaluated for
                                 (its ONE_4PI_EPS0); 0 = CF_ONE_4PI_EPS0.  Must be >= 0, finite */
} cf_params;

/* Execution options (all-zero = single GPU, device 0, default stream). */
typedef struct cf_options {
    int32_t device;      /* HIP device ordinal                                             */
    void* stream;        /* hipStream_t to enqueue on (NULL = the null stream)             */
    int32_t rank;        /* atom-decomposition rank (0..world_size-1)                       */
    int32_t world_size;  /* 0 or 1 = single GPU                                            */
    int32_t kspace_algo; /* reciprocal sum of ReferenceCoulKernels.cpp:513-556:
                            0 = default: exact k-sum, fp64 MFMA separable form
                            1 = exact k-sum, direct VALU sincos (check path)
                            2 = grid: the same k-sum through ES-kernel spreading, pruned DFT
                                and interpolation (error set by grid_width) */
    int32_t grid_width;  /* kspace_algo 2: ES kernel width in grid points, 4..16 (0 = 13, or 8 mixed) */
    int32_t precision;   /* CF_PRECISION_DOUBLE (0, default) or CF_PRECISION_MIXED (1): the
                            direct-space pair kernel computes in fp32 (positions, erfc, LJ) and
                            accumulates forces in fp32 and energies in fp64 per atom; every
                            other term stays fp64.  Accuracy target: RMS
                            relative force error <= 1e-4 against the fp64 build. */
    int32_t handover;    /* fork / join of the handle's second stream (grid k-space, see cf_set_overlap):
                            CF_HANDOVER_EVENT (0, default): hipEvents, waited on by the command
                            processor -- safe under any dispatch order;
                            CF_HANDOVER_MEMORY (1): a one-thread counter kernel + hipStreamWaitValue64,
                            ~5 us per hand-over cheaper, but the runtime executes the wait as a
                            polling kernel, so a tool that serializes dispatches (rocprofv3 counter
                            collection) can deadlock it.  Same results either way. */
    int32_t pair_list;   /* direct-space neighbour list (periodic):
                            CF_PAIR_LIST_AUTO (0): cluster-pair half list on one rank (fp64 and mixed),
                              per-atom full list on several ranks;
                            CF_PAIR_LIST_CLUSTER (1): the cluster-pair half list wherever its cell window
                              fits (also mixed precision, and several ranks with an ownership filter);
                            CF_PAIR_LIST_ATOM_HALF (2): the per-atom half list on one rank (full on several);
                            CF_PAIR_LIST_FULL (3): the per-atom full (two-sided) list.
                            (API 3's CF_PAIR_LIST_OCTANT (4) was removed in API 4: CF_ERR_INVALID.)
                            Same pair set and the same results up to the fp64 summation order. */
    int32_t variants;    /* CF_VARIANT_* bits: alternative kernels of the same sums, kept for A/B
                            verification (0 = the production kernels) */
    int32_t list_capacity;   /* neighbour-list capacity cap: cluster-pair entries per i-cluster, and
                            entries per sub-list of the per-atom lists; 0 = automatic (the density of
                            the denser of the default and the current box).  A list that overflows it
                            is evaluated by the fp64 rescan (slow, same results; tests force it). */
    int32_t reserved[1];
} cf_options;

#define CF_PRECISION_DOUBLE 0
#define CF_PRECISION_MIXED 1

#define CF_HANDOVER_EVENT 0
#define CF_HANDOVER_MEMORY 1

#define CF_PAIR_LIST_AUTO 0
#define CF_PAIR_LIST_CLUSTER 1
#define CF_PAIR_LIST_ATOM_HALF 2
#define CF_PAIR_LIST_FULL 3

/* cf_options.variants (grid k-space; each equal to the production kernel to <= 1e-12 relative) */
#define CF_VARIANT_GEMM_DFT 1        /* the DFT stages as fp64-MFMA complex GEMMs (k_g_cgemm), not the
                                        8 x Q factorized stages (also used when a grid exceeds those) */
#define CF_VARIANT_VECTOR_SPREAD 2   /* W > 9: the VALU spread (k_g_spread_tile), not the matrix cores */
#define CF_VARIANT_MFMA_SPREAD 4     /* W <= 9: the matrix-core spread (k_g_spread_mfma) */
#define CF_VARIANT_INTERP1 8         /* one atom per wave interpolation (k_g_interp) */
#define CF_VARIANT_INTERP2 16        /* W <= 8: two atoms per wave (k_g_interp2), not four */
#define CF_VARIANT_BLOCK_ROUNDS(r) (((r) & 15) << 8)   /* grid bin sort and energy kernels: r rounds of
                                        256 atoms per block (1..8; 0 = by N) */

/* compute flags */
#define CF_INCLUDE_FORCES 1
#define CF_INCLUDE_ENERGY 2

typedef struct cf_handle cf_handle;

CF_EXPORT int cf_api_version(void);
CF_EXPORT const char* cf_last_error(void);

/* Replaces ReferenceCalcCoulForceKernel::initialize (ReferenceCoulKernels.cpp:230-422). */
CF_EXPORT int cf_create(const cf_params* params, const cf_options* options, cf_handle** out);
CF_EXPORT int cf_destroy(cf_handle* h);

/* Ewald parameters chosen at initialize: alpha (nm^-1) and odd kmax per axis
 * (ReferenceCoulKernels.cpp:32-35, 401-420). */
CF_EXPORT int cf_get_ewald_params(const cf_handle* h, double* alpha, int32_t kmax[3]);
/* Grid of the kspace_algo 2 reciprocal path: points per axis and the ES kernel width
 * (zeros for the exact k-sum paths and without PBC). */
CF_EXPORT int cf_get_grid_shape(const cf_handle* h, int32_t ng[3], int32_t* width);
/* Owned atom range [lo, hi) of this rank (all atoms when world_size <= 1). */
CF_EXPORT int cf_get_owned_range(const cf_handle* h, int32_t* lo, int32_t* hi);
/* Host-only (no device needed): the atom decomposition cf_create would use.  Ranges are
 * contiguous and never split a molecule (connected component of flux terms + exceptions). */
CF_EXPORT int cf_partition(const cf_params* params, int32_t world_size, int32_t rank, int32_t* lo, int32_t* hi);

/* Persistent neighbour list (the reference rebuilds its voxel-hash list on
 * every call, ReferenceCoulKernels.cpp:559).  skin = 0 (default): rebuild on every
 * evaluation.  skin > 0 (nm): the list holds pairs within cutoff + skin and is kept while
 * the box is unchanged and no atom has moved more than skin/2 since the last build (decided
 * on the device).  The evaluated pair set is identical either way (every pair is tested
 * against the exact cutoff); only the fp64 summation order can differ.  Positions must be
 * continuous between calls (a re-wrapped atom just triggers a rebuild).  The skin is capped
 * at half the smallest box length minus the cutoff. */
CF_EXPORT int cf_set_neighbor_skin(cf_handle* h, double skin);
/* updateParametersInContext (the reference's CoulForce has none): replace
 * the charges, LJ parameters and flux-term parameters of a created handle.  The topology
 * must be unchanged -- the same particle count, flux terms on the same particles in the same
 * order, the same set of excluded pairs -- and so must periodicity, cutoff and Ewald
 * tolerance (alpha and kmax stay those of cf_create); otherwise CF_ERR_INVALID.  The next
 * evaluation rebuilds the neighbour list.  Not allowed between cf_compute_begin and _end. */
CF_EXPORT int cf_update_parameters(cf_handle* h, const cf_params* params);
/* The direct-space list the handle evaluates with (cf_options.pair_list resolved for this system and
 * box: CF_PAIR_LIST_CLUSTER, CF_PAIR_LIST_ATOM_HALF or CF_PAIR_LIST_FULL; CF_PAIR_LIST_AUTO before the
 * first periodic evaluation and without periodic boundaries).  A cluster or per-atom half list that
 * does not fit the box (fewer than 4 cells per axis, an 18-cell window over 4096 atoms at the
 * density of the box, several ranks without CF_PAIR_LIST_CLUSTER) resolves to CF_PAIR_LIST_FULL. */
CF_EXPORT int cf_get_pair_list(const cf_handle* h, int32_t* kind);
/* Number of neighbour-list builds and evaluations since cf_create. */
CF_EXPORT int cf_get_neighbor_stats(const cf_handle* h, int64_t* builds, int64_t* evaluations);
/* Slow-path diagnostics since cf_create (synchronises the stream): evaluations whose half-list
 * partner sums could not be used, so that every atom's pair sums were recomputed by the fp64 cell
 * rescan (same results, several times slower); list rows rescanned after a full-list overflow;
 * and the union of the reasons for the first (CF_FALLBACK_* bits).  Nonzero values on a
 * production system mean the neighbour-list capacity or the cell geometry does not suit it
 * (DESIGN.md §4.4).  Any output may be NULL. */
#define CF_FALLBACK_WINDOW 1        /* a cell's 18-cell window held more than 4096 atoms */
#define CF_FALLBACK_LIST 2          /* a list row overflowed, or the builder could not place it */
#define CF_FALLBACK_FIXED_POINT 4   /* a partner-side term beyond the fixed-point range (|F| >= 2^16) */
CF_EXPORT int cf_get_fallback_stats(const cf_handle* h, int64_t* half_list_fallbacks, int64_t* rows_rescanned,
                                    int32_t* reasons);

/* Device index guards.  The kernels check the data-dependent indices they are about to address
 * (cell and grid-bin bounds, the cluster table, list entries) against the buffers they index;
 * an index outside its buffer -- impossible by construction, so a bug or corrupted device
 * memory -- skips the access and sets a CF_GUARD_* bit instead of faulting the GPU.  The bit is
 * copied to host-mapped memory at the end of the evaluation, and every later entry point of the
 * handle (cf_compute*, cf_synchronize, cf_get_charges / _dedq / _energy_terms; cf_compute_host in
 * the same call) then returns CF_ERR_STATE naming the guard.  Sticky: re-create the handle.
 * cf_get_device_errors synchronises the handle's streams and returns the bits (0 = none).
 * The batched path (cf_compute_batch) adds no guard bits: every index it uses is topological,
 * validated by cf_create, or derived from the launch's own grid against N and nconf.  A guard that
 * is already set makes cf_compute_batch fail like every other entry point. */
#define CF_GUARD_CELL_BOUNDS 1
#define CF_GUARD_CLUSTER_TABLE 2
#define CF_GUARD_LIST_ENTRY 4
#define CF_GUARD_GRID_BINS 8
#define CF_GUARD_NEIGHBOR 16
#define CF_GUARD_ATOM_INDEX 32   /* cf_compute_openmm: an atom_index entry outside [0, N) */
#define CF_GUARD_REBUILD_FLAG 64 /* the neighbour-list rebuild flag found clear on a handle without a skin */
CF_EXPORT int cf_get_device_errors(cf_handle* h, int32_t* bits);

/*
 * Replaces ReferenceCalcCoulForceKernel::execute (ReferenceCoulKernels.cpp:424-636).
 * Device-resident, asynchronous on the handle's stream:
 *   pos_dev    [N*3] fp64 positions (nm), AoS x,y,z, DEVICE memory
 *   box9       host array, current periodic box vectors (rows) in OpenMM's reduced form
 *              a = (ax,0,0), b = (bx,by,0), c = (cx,cy,cz), |bx|,|cx| <= ax/2, |cy| <= by/2
 *              (triclinic boxes take the all-pairs neighbour list); ignored without PBC
 *   forces_dev [N*3] fp64 DEVICE buffer; forces are ADDED (+=) like the reference
 *              (ReferenceCoulKernels.cpp:426, 455, 585, 630).  Only owned atoms when world_size>1.
 *   energy_dev [1] fp64 DEVICE scalar, OVERWRITTEN with the (partial, per rank) energy.
 * Either output may be NULL.  Energy semantics follow the reference, including its
 * quirk that the self/real-space/exclusion terms are accumulated even without
 * CF_INCLUDE_ENERGY in periodic mode (ReferenceCoulKernels.cpp:507-510, 592, 619).
 */
CF_EXPORT int cf_compute(cf_handle* h, const double* pos_dev, const double* box9, int flags,
                         double* forces_dev, double* energy_dev);

/*
 * The same evaluation on an OpenMM GPU platform's own device buffers, without copies -- the
 * conventions the reference's CUDA platform binds its kernels to (CudaCalcCoulForceKernel::execute,
 * platforms/cuda/src/CudaCoulKernels.cpp:523-600: cu.getPosq(), cu.getAtomIndexArray(),
 * cu.getForce(), cu.getEnergyBuffer(), cu.getPaddedNumAtoms()).  Single rank only.
 *   posq        [N] real4 in the platform's sorted order: posq[s] = (x, y, z, w) of atom
 *               atom_index[s] (nm; w -- the platform's charge slot -- is never read or written).
 *               posq_kind: CF_POSQ_DOUBLE4 (double precision: double4) or CF_POSQ_FLOAT4
 *               (single / mixed precision: float4; posq_correction, if not NULL, is the mixed
 *               platform's float4 posqCorrection, added in fp64)
 *   atom_index  [N] int32 DEVICE array: sorted slot -> atom index (cu.getAtomIndexArray())
 *   padded_n    paddedNumAtoms: the stride of the force planes (>= N)
 *   force_buf   [3 * padded_n] long long DEVICE array, fixed point in units of 2^-32 kJ/mol/nm, the
 *               x, y, z planes one after the other, indexed by sorted slot: forces are ADDED
 *               (OpenMM's conversion (long long)(f * 2^32), 64-bit atomic adds).  NULL: no forces.
 *   energy_buf  DEVICE address of one energy-buffer element (cu.getEnergyBuffer()): the energy
 *               is ADDED to it; energy_kind CF_ENERGY_DOUBLE (mixed / double: `mixed` = double)
 *               or CF_ENERGY_FLOAT (single).  NULL: not written.
 * Energy semantics and flags as cf_compute.  The positions are gathered into the handle's atom
 * order and the forces scattered back by two small kernels on the handle's stream (~2 x 3 us at
 * C3); everything between is cf_compute's device-resident path (graph replay included).
 */
#define CF_POSQ_DOUBLE4 0
#define CF_POSQ_FLOAT4 1
#define CF_ENERGY_DOUBLE 0
#define CF_ENERGY_FLOAT 1
CF_EXPORT int cf_compute_openmm(cf_handle* h, const void* posq, const void* posq_correction, int32_t posq_kind,
                                const int32_t* atom_index, int32_t padded_n, const double* box9, int flags,
                                long long* force_buf, void* energy_buf, int32_t energy_kind);

/* Split-phase form for multi-GPU: begin computes charges and this rank's partial
 * structure factors; the caller all-reduces (sum) the buffer returned by
 * cf_kspace_buffer (fp64, on device, on the handle's stream ordering); end finishes. */
CF_EXPORT int cf_compute_begin(cf_handle* h, const double* pos_dev, const double* box9, int flags);
CF_EXPORT int cf_kspace_buffer(cf_handle* h, double** buf_dev, int64_t* count);
/* Optional, between cf_compute_begin and cf_compute_end: launch the direct-space and
 * exclusion kernels now.  They do not depend on the structure factors, so a multi-rank
 * caller launches them after starting the S(k) all-reduce and before waiting for it (the
 * two overlap).  cf_compute_end runs them itself if this was not called. */
CF_EXPORT int cf_compute_direct(cf_handle* h);
CF_EXPORT int cf_compute_end(cf_handle* h, double* forces_dev, double* energy_dev);

/* Graph replay: enable = 1 captures the launches of an evaluation into hipGraphs (on a private
 * stream) and replays them on the handle's stream while the calls look the same to the host:
 * same device buffers, flags, box and neighbour-list decision (a rebuild under a kept skin is
 * decided on the device, inside the graph).  A change re-captures.  A single-rank cf_compute /
 * cf_compute_host is one graph; the split-phase calls of a multi-rank step are three (begin,
 * direct, end: the caller's all-reduce runs between them on the same stream).  Evaluations with
 * timing on run eagerly.  Results are identical either way (the same kernels in the same order). */
CF_EXPORT int cf_set_graph(cf_handle* h, int enable);
/* Number of graph captures and replays since cf_set_graph(h, 1). */
CF_EXPORT int cf_get_graph_stats(const cf_handle* h, int64_t* captures, int64_t* replays);

/* Second stream (default on; cf_options.handover selects its fork / join): with the
 * grid k-space a single-rank cf_compute runs the reciprocal chain, and the split-phase calls of
 * a multi-rank step run the direct-space chain, on a second stream of the handle, joined before
 * the chain rule.  Results are bitwise those of the one-stream order.  enable = 0 launches
 * everything on the handle's stream (kernel durations are then the kernels' own). */
CF_EXPORT int cf_set_overlap(cf_handle* h, int enable);

/* Synchronous host-memory convenience (H2D positions, D2H forces/energy): what an
 * OpenMM Reference/CPU-platform adapter calls.  forces_host is ADDED to. */
CF_EXPORT int cf_compute_host(cf_handle* h, const double* pos_host, const double* box9, int flags,
                              double* forces_host, double* energy_host);

/*
 * Batched evaluation: nconf conformations of the handle's system in one call -- what fitting a
 * charge-flux model needs (charges, energies and forces of thousands of small gas-phase
 * conformations).  Non-periodic handles on one rank only: a periodic handle gives CF_ERR_INVALID,
 * world_size > 1 CF_ERR_STATE, as does a call between cf_compute_begin and _end.
 *   pos_dev     [nconf][N][3] fp64 DEVICE, conformation-major
 *   forces_dev  [nconf][N][3] fp64 DEVICE, ADDED to (as cf_compute); NULL or no CF_INCLUDE_FORCES: untouched
 *   energy_dev  [nconf] fp64 DEVICE, OVERWRITTEN (0 without CF_INCLUDE_ENERGY); NULL: not written
 *   charges_dev [nconf][N] fp64 DEVICE, OVERWRITTEN with the charges after flux; NULL: not written
 * Per conformation the result is cf_compute's on a non-periodic handle: the same flux formulas, the
 * all-pairs sum with excluded pairs skipped, the chain rule, one_4pi_eps0; always fp64.  nconf = 0
 * is a no-op.  A pass is at most four kernel launches whatever nconf (each kernel's grid spans
 * conformations x atom tiles); every sum is taken in an order fixed by the system alone, so a
 * conformation's results are bitwise reproducible and independent of what else is in the batch,
 * of nconf and of the pass size.
 * Asynchronous on the handle's stream: inputs and outputs must stay valid until the stream reaches
 * them.  The first call, and any call that needs a larger workspace, allocates it and so
 * synchronises the handle's streams.  The batch path has its own workspace: cf_get_charges /
 * _dedq / _energy_terms / _neighbor_stats / _graph_stats keep reporting the last cf_compute, and
 * the next cf_compute is unaffected.  Batch launches are always eager (never captured or replayed;
 * the handle's graph mode stays as it was) and are not recorded by cf_set_timing.
 * cf_update_parameters takes effect on the next batch call (the same parameter buffers are read).
 */
CF_EXPORT int cf_compute_batch(cf_handle* h, int32_t nconf, const double* pos_dev, int flags,
                               double* forces_dev, double* energy_dev, double* charges_dev);
/* synchronous host-memory form of the same (H2D, evaluate, D2H); forces_host ADDED to */
CF_EXPORT int cf_compute_batch_host(cf_handle* h, int32_t nconf, const double* pos_host, int flags,
                                    double* forces_host, double* energy_host, double* charges_host);
/*
 * The same for a PERIODIC handle, one box per conformation -- condensed-phase training frames
 * (small boxes from NVT / NPT trajectories).  Arrays as cf_compute_batch, plus
 *   boxes_host  [nconf][9] fp64 HOST, box vectors a, b, c per conformation as cf_compute's box9
 *               (OpenMM's reduced form, orthorhombic or triclinic; a batch may mix both)
 * boxes_host is read during the call (copied to a pinned buffer of the handle and uploaded from
 * there): the caller may free or overwrite it as soon as the call returns.  Reusing the pinned
 * buffer makes a call wait until the box upload of the previous periodic batch call on this handle
 * has finished (that upload precedes the previous call's kernels on the stream; no other
 * synchronisation in steady state).
 * Every box is checked on the host by cf_compute's rules (reduced form, lengths > 0, cutoff <= half
 * of each diagonal length), all of them before anything is launched: a bad box gives CF_ERR_INVALID
 * with a message naming the conformation index, no output touched, no statistic counted.
 * Per conformation the result is cf_compute's on this handle with that box and kspace_algo 0: flux
 * charges with the box-vector minimum image, the self term, the exact reciprocal sum over the
 * reference's half-space k set (box diagonals), real space over every pair once by minimum image
 * within the cutoff with excluded pairs left out, the erf correction of every excluded pair (any
 * distance), the chain rule.  alpha and kmax are cf_create's (from the default box) whatever the
 * conformation's box, as in cf_compute.  The energy follows cf_compute's flags on a periodic
 * handle, the reference's quirk included: self, direct and exclusion energy are accumulated
 * without CF_INCLUDE_ENERGY, the reciprocal part only with it.  Always fp64 and the exact k-sum,
 * all pairs without a cell or neighbour list: the handle's kspace_algo, grid_width, precision,
 * pair_list, skin and graph mode are ignored and left as they are.
 * A non-periodic handle gives CF_ERR_INVALID, world_size > 1 and a call between cf_compute_begin
 * and _end CF_ERR_STATE, NULL pos or boxes and nconf < 0 CF_ERR_INVALID; nconf = 0 is a no-op.  A
 * pass is at most seven kernel launches whatever nconf; every sum's order depends only on N, the
 * topology and kmax, so a conformation's results are bitwise the same alone, at any position of
 * any batch and under any pass size.  Asynchrony, the lazily grown workspace of its own (growth
 * allocates and synchronises; cf_destroy frees it), isolation from cf_compute and its diagnostics,
 * eager launches outside cf_set_timing, cf_update_parameters: as cf_compute_batch.  No guard bits.
 */
CF_EXPORT int cf_compute_batch_periodic(cf_handle* h, int32_t nconf, const double* pos_dev,
                                        const double* boxes_host, int flags, double* forces_dev,
                                        double* energy_dev, double* charges_dev);
/* synchronous host-memory form of the same (H2D, evaluate, D2H); forces_host ADDED to */
CF_EXPORT int cf_compute_batch_periodic_host(cf_handle* h, int32_t nconf, const double* pos_host,
                                             const double* boxes_host, int flags, double* forces_host,
                                             double* energy_host, double* charges_host);
/*
 * Parameter gradients of the non-periodic batch: the reverse-mode product (VJP) of cf_compute_batch
 * with respect to the base charges and the flux parameters -- what an optimiser step of a
 * charge-flux fit needs.  Per conformation, with the cotangents e_bar (scalar), q_bar[N] and
 * F_bar[N][3] of its energy, its charges after flux and its forces, the call writes the gradient
 * of  L = e_bar E + sum_i q_bar_i q_i + sum_i F_bar_i . F_i  with respect to every parameter.
 *   counts[4]       N, 2 * bonds, 2 * angles, 5 * waters: the lengths of the four parameter groups;
 *                   P = their sum
 *   pos_dev         [nconf][N][3] fp64 DEVICE, conformation-major
 *   energy_bar_dev  [nconf] fp64 DEVICE, or NULL (= zero)
 *   charges_bar_dev [nconf][N] fp64 DEVICE, or NULL (= zero)
 *   forces_bar_dev  [nconf][N][3] fp64 DEVICE, or NULL (= zero)
 *   grad_dev        [nconf][P] fp64 DEVICE, OVERWRITTEN: per conformation the base charges [N], then
 *                   the bonds' (k, b) pairs, the angles' (k, theta0) pairs and the waters'
 *                   (k1, k2, kub, b0, ub0) 5-tuples -- the order and layout of the cf_params arrays
 * The gradients of the conformations are NOT summed: a fit sums them with its own weights.  With all
 * three cotangents NULL grad is set to exact zeros (one memset, no pass).
 * Closed form (every flux term is linear in each of its parameters, the energy quadratic in the
 * charges): with g_i = dE/dq_i, h_i the directional derivative of g_i along F_bar and
 * a_i = e_bar g_i + q_bar_i - h_i, the base charge i receives a_i and every flux parameter a
 * product of the a and g of its term's atoms with the term's geometry and its tangent along F_bar
 * ("Batched, parameter gradients").  No formula divides by a parameter: a term with
 * k = 0 is legal.
 * Periodic handles have cf_compute_batch_periodic_vjp (here: CF_ERR_INVALID, as cf_compute_batch).
 * The LJ sigma / epsilon have cf_compute_batch_lj_vjp.  Out of scope: gradients with respect to the
 * positions.
 * Errors and states as cf_compute_batch: a periodic handle CF_ERR_INVALID; world_size > 1 or a call
 * between cf_compute_begin and _end CF_ERR_STATE; NULL pos or grad, or nconf < 0, CF_ERR_INVALID;
 * nconf = 0 is a no-op; a NULL handle is rejected without touching a device.
 * Always fp64, eager launches on the handle's stream (never captured or replayed, not recorded by
 * cf_set_timing), asynchronous: inputs and outputs must stay valid until the stream reaches them.  A
 * pass is at most five kernel launches whatever nconf, without atomics; every sum's order depends
 * only on N and the topology, so a conformation's gradients are bitwise the same alone, at any
 * position of any batch and under any pass size.  It uses the batch workspace and, allocated on the
 * first call (growth allocates and synchronises; cf_destroy frees it), three more arrays of N doubles
 * per conformation; cf_compute's state and diagnostics are not touched.  It reads the parameter
 * buffers cf_update_parameters last wrote.  No guard bits.
 */
CF_EXPORT int cf_get_param_counts(const cf_handle* h, int32_t counts[4]);
CF_EXPORT int cf_compute_batch_vjp(cf_handle* h, int32_t nconf, const double* pos_dev,
                                   const double* energy_bar_dev, const double* charges_bar_dev,
                                   const double* forces_bar_dev, double* grad_dev);
/* synchronous host-memory form of the same (H2D, evaluate, D2H) */
CF_EXPORT int cf_compute_batch_vjp_host(cf_handle* h, int32_t nconf, const double* pos_host,
                                        const double* energy_bar_host, const double* charges_bar_host,
                                        const double* forces_bar_host, double* grad_host);
/*
 * The same for a PERIODIC handle, one box per conformation: the reverse-mode product of
 * cf_compute_batch_periodic with respect to the base charges and the flux parameters.  Cotangents
 * and grad as cf_compute_batch_vjp (rows in the order of cf_get_param_counts, not summed over the
 * conformations, NULL cotangents = zeros, all three NULL = one memset of grad); boxes_host
 * [nconf][9] fp64 HOST as cf_compute_batch_periodic: copied through the handle's pinned buffer and
 * uploaded (the same reuse rule), every box checked by cf_compute's rules before anything is
 * launched -- a bad box gives CF_ERR_INVALID with a message naming the conformation index, no output
 * touched, no statistic counted.
 * The scalar differentiated per conformation is L = e_bar E + sum_i q_bar_i q_i + sum_i F_bar_i . F_i
 * with E, q, F what cf_compute_batch_periodic returns for that conformation and box with both
 * CF_INCLUDE_* flags (all four energy terms): fp64, the exact k-sum over the half-space k set, all
 * pairs by minimum image; alpha and kmax are cf_create's, the Coulomb constant the handle's.  Closed
 * form as cf_compute_batch_vjp, with g_i and h_i now summing the erfc pair terms within the cutoff,
 * the erf correction of excluded pairs, the self term and the reciprocal sum with the structure
 * factor S(k) and its tangent along F_bar, and the term geometry taken from minimum-image vectors
 * ("Batched, periodic, parameter gradients").  The box is fixed: no box derivatives.  No
 * formula divides by a parameter.
 * A non-periodic handle gives CF_ERR_INVALID; world_size > 1 or a call between cf_compute_begin and
 * _end CF_ERR_STATE; NULL pos, boxes or grad, or nconf < 0, CF_ERR_INVALID; nconf = 0 is a no-op
 * that counts nothing; a NULL handle is rejected without touching a device.
 * Eager launches on the handle's stream (never captured or replayed, not recorded by
 * cf_set_timing), asynchronous.  A pass is at most eight kernel launches whatever nconf, without
 * atomics; every sum's order depends only on N, the topology and kmax, so a conformation's gradients
 * are bitwise the same alone, at any position of any batch and under any pass size.  It uses the
 * periodic batch workspace and, allocated on the first call (growth allocates and synchronises;
 * cf_destroy frees it), a block of its own: qdot[N], g[N], a[N] and a second coefficient array of 2
 * doubles per k-vector per conformation.  cf_compute's state and diagnostics are not touched.  It
 * reads the parameter buffers cf_update_parameters last wrote.  No guard bits.
 */
CF_EXPORT int cf_compute_batch_periodic_vjp(cf_handle* h, int32_t nconf, const double* pos_dev,
                                            const double* boxes_host, const double* energy_bar_dev,
                                            const double* charges_bar_dev, const double* forces_bar_dev,
                                            double* grad_dev);
/* synchronous host-memory form of the same (H2D, evaluate, D2H) */
CF_EXPORT int cf_compute_batch_periodic_vjp_host(cf_handle* h, int32_t nconf, const double* pos_host,
                                                 const double* boxes_host, const double* energy_bar_host,
                                                 const double* charges_bar_host, const double* forces_bar_host,
                                                 double* grad_host);
/*
 * LJ parameter gradients of both batches: the reverse-mode product of cf_compute_batch (non-periodic
 * handle) or cf_compute_batch_periodic (periodic handle) with respect to every atom's Lennard-Jones
 * sigma and epsilon -- the parameters a charge-flux model is fitted together with.  One entry point
 * serves both kinds of handle:
 *   boxes_host      periodic handle: [nconf][9] fp64 HOST as cf_compute_batch_periodic (the same
 *                   pinned copy, upload and reuse rule; every box checked by cf_compute's rules
 *                   before anything is launched or counted -- a bad box gives CF_ERR_INVALID with a
 *                   message naming the conformation index); NULL gives CF_ERR_INVALID.
 *                   Non-periodic handle: must be NULL, anything else gives CF_ERR_INVALID
 *   pos_dev         [nconf][N][3] fp64 DEVICE, conformation-major
 *   energy_bar_dev  [nconf] fp64 DEVICE, or NULL (= zero)
 *   forces_bar_dev  [nconf][N][3] fp64 DEVICE, or NULL (= zero)
 *   grad_dev        [nconf][2 N] fp64 DEVICE, OVERWRITTEN: per conformation dL/dsigma[N], then
 *                   dL/depsilon[N]; not summed over the conformations
 * with L = e_bar E + sum_i F_bar_i . F_i per conformation.  There is no charge cotangent: the charges
 * do not depend on sigma or epsilon, and neither does the pair set, so only the LJ term of E and F
 * enters (no flux, charge or k-space stage).  With both cotangents NULL grad is set to exact zeros
 * (one memset; the call and its conformations are counted, no pass).
 * Closed form: the handle stores lj_i = (sigma_i / 2, 2 sqrt(eps_i)); a pair carries
 * U_ij = e4 s6 (s6 - 1) with A = lj_i.x + lj_j.x, e4 = lj_i.y lj_j.y, s6 = (A / r)^6, over every
 * non-excluded pair (periodic: minimum image within the cutoff).  With rdot_ij = d_ij . (F_bar_i -
 * F_bar_j) / r:
 *   dL/dsigma_i = 1/2 sum_j e4 (A^5 / r^6) [e_bar (12 s6 - 6) + (144 s6 - 36) rdot_ij / r]
 *   dL/deps_i   = (2 / lj_i.y) sum_j lj_j.y [e_bar s6 (s6 - 1) + (12 s6^2 - 6 s6) rdot_ij / r]
 * Nothing divides by sigma: sigma_i = sigma_j = 0 is legal and gives 0.
 * CONVENTION: an atom with eps_i = 0 receives exactly 0 for dL/deps_i (and, by the formula, for
 * dL/dsigma_i).  The true derivative of sqrt(eps_i eps_j) is singular there; such an atom has no LJ
 * interaction, and a fit leaves it at 0.
 * Errors and states as the other VJP calls: a NULL handle is rejected without touching a device; NULL
 * pos or grad, or nconf < 0, CF_ERR_INVALID; world_size > 1 or a call between cf_compute_begin and
 * _end CF_ERR_STATE; nconf = 0 is a no-op that counts nothing; a guard bit already set fails the call.
 * Always fp64, eager launches on the handle's stream (never captured or replayed, not recorded by
 * cf_set_timing), asynchronous.  One kernel launch per pass and no workspace; a pass is
 * min(cf_set_batch_limit or 65535, nconf) conformations.  No atomics; every sum's order depends only
 * on N and the topology, so a conformation's row is bitwise the same alone, at any position of any
 * batch, under any pass size and in the host and the device form.  cf_get_batch_stats counts it;
 * cf_compute's state and diagnostics are not touched.  It reads the LJ buffer cf_update_parameters
 * last wrote.  No guard bits.
 */
CF_EXPORT int cf_compute_batch_lj_vjp(cf_handle* h, int32_t nconf, const double* pos_dev, const double* boxes_host,
                                      const double* energy_bar_dev, const double* forces_bar_dev,
                                      double* grad_dev);
/* synchronous host-memory form of the same (H2D, evaluate, D2H) */
CF_EXPORT int cf_compute_batch_lj_vjp_host(cf_handle* h, int32_t nconf, const double* pos_host,
                                           const double* boxes_host, const double* energy_bar_host,
                                           const double* forces_bar_host, double* grad_host);
/*
 * Dipoles and atomic polar tensors (APT) of the non-periodic batch -- what a fit to dipole surfaces
 * and IR intensities targets.  Per conformation, with q the charges after flux (exactly
 * cf_compute_batch's charges, to the bit):
 *   mu[al]        = sum_a q_a x_a[al]                          (e nm)
 *   P[b][al][be]  = d mu[al] / d x_b[be]
 *                 = q_b delta(al, be) + sum_a x_a[al] dq_a/dx_b[be]            (e)
 * The origin is the coordinate origin: the dipole of a charged system moves with a translation d by
 * (sum_a q_a) d; P does not.  sum_b P_b = (sum_a q_a) I.
 *   pos_dev      [nconf][N][3] fp64 DEVICE, conformation-major
 *   dipole_dev   [nconf][3] fp64 DEVICE, or NULL
 *   apt_dev      [nconf][N][3][3] fp64 DEVICE indexed [b][al][be] as above, or NULL
 *   charges_dev  [nconf][N] fp64 DEVICE, or NULL
 * All outputs are OVERWRITTEN.  With all three NULL the call and its conformations are counted and
 * nothing is launched.  A pass is at most three kernel launches whatever nconf (flux terms, charges,
 * one kernel for mu and P), in the batch workspace of cf_compute_batch with its pass size.  The
 * charge-flux part of P is gathered over atom b's chain-rule entries in the order of the force's
 * chain rule; no atomics, every sum's order depends only on N and the topology, so a conformation's
 * results are bitwise the same alone, at any position of any batch, under any pass size and in the
 * host and the device form.
 *
 * cf_compute_batch_dipole_vjp: the reverse-mode product with respect to the base charges and the
 * flux parameters.  Per conformation, with cotangents mu_bar[3] and P_bar[N][3][3], the scalar is
 * L = mu_bar . mu + sum_b P_bar_b : P_b.
 *   dipole_bar_dev  [nconf][3] fp64 DEVICE, or NULL (= zero)
 *   apt_bar_dev     [nconf][N][3][3] fp64 DEVICE, or NULL (= zero)
 *   grad_dev        [nconf][P] fp64 DEVICE, OVERWRITTEN: rows in the order of cf_get_param_counts, as
 *                   cf_compute_batch_vjp; not summed over the conformations
 * With both cotangents NULL grad is set to exact zeros (one memset; the call and its conformations
 * are counted, no pass).
 * Closed form: every flux term is a sum of pieces q_a += c_a k (g(x) - ref) over its atoms (bond:
 * g = r, c = (1, -1); angle: g = theta, c = (1, -2, 1); water: r12, r13 and r23 with the signs of its
 * three charge slots).  With a_i = mu_bar . x_i + tr P_bar_i and w = sum_a c_a x_a:
 *   dL/d(base charge i) = a_i
 *   dL/dk   += (sum_a c_a a_a) (g - ref) + sum_b w^T P_bar_b grad_b g
 *   dL/dref += -k sum_a c_a a_a
 * Nothing divides by a parameter: a term with k = 0 is legal.  There is no pair sum and no workspace:
 * at most two kernel launches per pass; a pass is min(cf_set_batch_limit or 65535, nconf)
 * conformations.  The same bitwise guarantees as the forward call.
 *
 * Errors and states of both as cf_compute_batch_vjp: a periodic handle CF_ERR_INVALID (the dipole of
 * a periodic cell is not defined); world_size > 1 or a call between cf_compute_begin and _end
 * CF_ERR_STATE; NULL pos, NULL grad or nconf < 0 CF_ERR_INVALID; nconf = 0 is a no-op that counts
 * nothing; a NULL handle is rejected without touching a device; a guard bit already set fails the
 * call.  Always fp64, eager launches on the handle's stream (never captured or replayed, not recorded
 * by cf_set_timing), asynchronous: inputs and outputs must stay valid until the stream reaches them.
 * cf_get_batch_stats counts both; cf_compute's state and diagnostics are not touched; both read the
 * parameter buffers cf_update_parameters last wrote.  No guard bits.  Out of scope: periodic handles,
 * gradients with respect to the positions.
 */
CF_EXPORT int cf_compute_batch_dipole(cf_handle* h, int32_t nconf, const double* pos_dev, double* dipole_dev,
                                      double* apt_dev, double* charges_dev);
/* synchronous host-memory form of the same (H2D, evaluate, D2H) */
CF_EXPORT int cf_compute_batch_dipole_host(cf_handle* h, int32_t nconf, const double* pos_host, double* dipole_host,
                                           double* apt_host, double* charges_host);
CF_EXPORT int cf_compute_batch_dipole_vjp(cf_handle* h, int32_t nconf, const double* pos_dev,
                                          const double* dipole_bar_dev, const double* apt_bar_dev, double* grad_dev);
/* synchronous host-memory form of the same (H2D, evaluate, D2H) */
CF_EXPORT int cf_compute_batch_dipole_vjp_host(cf_handle* h, int32_t nconf, const double* pos_host,
                                               const double* dipole_bar_host, const double* apt_bar_host,
                                               double* grad_host);
/*
 * Hessian-vector products of the non-periodic batch -- normal modes (with the polar tensors: IR
 * spectra), Newton-CG geometry optimisation, harmonic validation of a fitted model.  H = d2E/dxdx is
 * the Hessian with respect to the positions of exactly the energy cf_compute_batch returns with both
 * flags: all non-excluded pairs, Coulomb with the charges after flux, LJ, the handle's one_4pi_eps0.
 * Per conformation c and direction k:   out[c][k] = H(x_c) v_ck = -D_v F,   F = cf_compute_batch's
 * forces, D_v the directional derivative along v.
 *   pos_dev   [nconf][N][3] fp64 DEVICE, conformation-major (nm)
 *   vec_dev   [nconf][nvec][N][3] fp64 DEVICE (nm): nvec directions per conformation
 *   out_dev   [nconf][nvec][N][3] fp64 DEVICE, OVERWRITTEN (kJ/mol/nm^2 times the unit of v)
 * The nvec directions of a conformation share its positions: flux, charges and dq/dx are computed once
 * per conformation.  The 3N unit vectors give the full Hessian, one row (= column) per direction.
 * Closed form, no finite differences anywhere: with d = x_j - x_i, w = v_j - v_i, qdot = D_v q and
 * D = dq/dx,
 *   (H v)_i = sum_j (sdot d + s w) + sum_a (gdot_a D_ai + g_a Ddot_ai)
 *   s    = (A + C) / r^2,  A = e4 s6 (12 s6 - 6),  C = ke q_i q_j / r      (the forward pair term)
 *   sdot = [e4 s6 (48 - 168 s6) - 3 C] (d.w) / r^4 + ke (qdot_i q_j + q_i qdot_j) / r^3
 *   g_a  = ke sum_j q_j / r,  gdot_a = ke sum_j [qdot_j / r - q_j (d.w) / r^3]
 * over the non-excluded j != i, and Ddot = D_v D from the flux terms' own expressions evaluated on
 * (value, tangent) pairs.  Nothing divides by a parameter: a term with k = 0 is legal.
 * A pass is at most six kernel launches whatever nconf and nvec (flux terms, charges, term tangents,
 * charge tangents, all pairs, chain rule), in the workspace of cf_compute_batch plus, per
 * (conformation, direction), the slot tangents, the tangent of dq/dx, qdot[N], g[N] and gdot[N].  No
 * atomics; every sum's order depends only on N and the topology, so the row of a (conformation,
 * direction) is bitwise the same alone, at any position of any batch, for any nvec, under any pass
 * size and in the host and the device form.
 *
 * Errors and states as cf_compute_batch_vjp: a periodic handle CF_ERR_INVALID; world_size > 1 or a
 * call between cf_compute_begin and _end CF_ERR_STATE; NULL pos, vec or out, nconf < 0 or nvec < 0
 * CF_ERR_INVALID; nconf = 0 or nvec = 0 is a no-op that counts nothing; a NULL handle is rejected
 * without touching a device; a guard bit already set fails the call.  Always fp64, eager launches on
 * the handle's stream (never captured or replayed, not recorded by cf_set_timing), asynchronous:
 * inputs and outputs must stay valid until the stream reaches them.  cf_get_batch_stats counts the
 * call, its nconf conformations and its passes; cf_compute's state and diagnostics are not touched; it
 * reads the parameter buffers cf_update_parameters last wrote.  No guard bits.  Out of scope: periodic
 * handles, the derivative of H with respect to the parameters.
 */
CF_EXPORT int cf_compute_batch_hvp(cf_handle* h, int32_t nconf, const double* pos_dev, int32_t nvec,
                                   const double* vec_dev, double* out_dev);
/* synchronous host-memory form of the same (H2D, evaluate, D2H) */
CF_EXPORT int cf_compute_batch_hvp_host(cf_handle* h, int32_t nconf, const double* pos_host, int32_t nvec,
                                        const double* vec_host, double* out_host);
/* cap on the conformations evaluated per pass (bounds the batch workspace); 0 = automatic: as many
 * as keep the workspace (per conformation q[N], the flux slots, dq/dx, dE/dq[N], F[3N], e[N]; a
 * periodic batch also the phase tables, 4 doubles per [N][kmax_x + kmax_y + kmax_z] entry, and 3
 * doubles per k-vector; cf_compute_batch_vjp also qdot[N], g[N], a[N]; cf_compute_batch_periodic_vjp
 * those three and 2 more doubles per k-vector) at or below 256 MiB, and never more than 65535
 * (cf_compute_batch_lj_vjp and cf_compute_batch_dipole_vjp have no workspace: automatic is 65535).
 * cf_compute_batch_hvp: a pass is conformations x directions with conformations * directions <= 65535;
 * per conformation the doubles of cf_compute_batch, per (conformation, direction) S + 3 D + 3 N more
 * (S charge slots: 2 per bond, 3 per angle or water; D dq/dx entries: 4 per bond, 9 per angle or
 * water); the limit caps its conformations, and a conformation whose nvec directions alone exceed
 * 256 MiB or 65535 takes its directions in several passes.  A
 * larger batch runs as consecutive passes.  Applies to every batch form; cf_get_batch_stats counts
 * them all (a VJP call with all cotangents NULL counts its call and conformations, and no pass). */
CF_EXPORT int cf_set_batch_limit(cf_handle* h, int32_t max_conformations);
/* since cf_create: batch calls, conformations evaluated, passes (chunks) launched; any output may be NULL */
CF_EXPORT int cf_get_batch_stats(const cf_handle* h, int64_t* calls, int64_t* conformations, int64_t* passes);

/* Diagnostics of the last evaluation (synchronous, host outputs).
 *   charges [N]  realcharges after charge flux          (ReferenceCoulKernels.cpp:37-228)
 *   dedq    [N]  dE/dq_i (complete: self+recip+direct+exclusion)
 *   terms   [4]  E_self, E_recip, E_direct(incl. LJ), E_exclusion (PBC); [0,0,E,0] without PBC */
CF_EXPORT int cf_get_charges(cf_handle* h, double* charges_host);
CF_EXPORT int cf_get_dedq(cf_handle* h, double* dedq_host);
CF_EXPORT int cf_get_energy_terms(cf_handle* h, double terms[4]);
CF_EXPORT int cf_synchronize(cf_handle* h);

/* Per-kernel timing: when enabled, start/stop hipEvents are recorded on the handle's
 * stream around every kernel launch of every evaluation (negligible overhead).
 * cf_get_timing synchronises and returns, per phase, the summed milliseconds and the
 * number of recorded launches since cf_set_timing; names are 16-byte NUL-padded. */
CF_EXPORT int cf_set_timing(cf_handle* h, int enable);
/* As cf_set_timing, but only the phases whose bit is set in phase_mask (bit p = the p-th
 * phase name cf_get_timing reports) are bracketed by events; 0 disables timing.  Each timed
 * launch costs two event records on the stream, so a benchmark times only what it reports. */
CF_EXPORT int cf_set_timing_mask(cf_handle* h, uint32_t phase_mask);
CF_EXPORT int cf_get_timing(cf_handle* h, int32_t max_phases, char* names, double* total_ms, int32_t* calls,
                            int32_t* nphases);

#ifdef __cplusplus
}
#endif
#endif /* CHARGEFLUX_H_ */
