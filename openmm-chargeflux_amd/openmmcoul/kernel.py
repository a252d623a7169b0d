"""The HIP implementation of CalcCoulForceKernel, plus a minimal OpenMM-shaped
System/Context/State so the force can be driven (and tested) the way the reference is
driven from OpenMM.

Reference interfaces mirrored:
  CalcCoulForceKernel::{Name, initialize, execute}   openmmapi/include/CoulKernels.h:15-38
  CoulForceImpl::{initialize, calcForcesAndEnergy}   openmmapi/src/CoulForceImpl.cpp:16-27
  System::getDefaultPeriodicBoxVectors               (used at ReferenceCoulKernels.cpp:399-400)

Device arrays are torch tensors (PyTorch is plumbing here: device memory and streams);
host arrays are numpy.  Every evaluation runs in libchargeflux_hip.so — there is no
Python or CPU compute path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _cabi
from .force import CoulForce

DP = C.POINTER(C.c_double)


def _dp(a: np.ndarray):
    return a.ctypes.data_as(DP)


class System:
    """Minimal stand-in for openmm.System (particle count + default box + forces)."""

    def __init__(self):
        self._masses: list[float] = []
        self._box = np.diag([2.0, 2.0, 2.0]).astype(np.float64)
        self._forces: list = []

    def addParticle(self, mass):
        self._masses.append(float(mass))
        return len(self._masses) - 1

    def getNumParticles(self):
        return len(self._masses)

    def setDefaultPeriodicBoxVectors(self, a, b, c):
        self._box = np.array([a, b, c], dtype=np.float64).reshape(3, 3)

    def getDefaultPeriodicBoxVectors(self):
        return [self._box[0].copy(), self._box[1].copy(), self._box[2].copy()]

    def addForce(self, force):
        self._forces.append(force)
        return len(self._forces) - 1

    def getForces(self):
        return list(self._forces)


def _box9(box) -> np.ndarray:
    if box is None:
        return np.zeros(9)
    return np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(9))


class HipCalcCoulForceKernel:
    """CalcCoulForceKernel on MI355X.  initialize() ~ ReferenceCalcCoulForceKernel::initialize
    (ReferenceCoulKernels.cpp:230-422); execute() ~ ...::execute (:424-636)."""

    @staticmethod
    def Name():
        return "CalcCoulForce"

    # reciprocal-sum algorithms (cf_options.kspace_algo, include/chargeflux.h)
    KSPACE_EXACT_MFMA = 0   # exact k-sum, fp64 MFMA separable form
    KSPACE_EXACT_VALU = 1   # exact k-sum, direct sincos (check path)
    KSPACE_GRID = 2         # same k-sum via ES-kernel grid (spread, pruned DFT, interpolate)

    PAIR_LISTS = {"auto": _cabi.CF_PAIR_LIST_AUTO, "cluster": _cabi.CF_PAIR_LIST_CLUSTER,
                  "atom_half": _cabi.CF_PAIR_LIST_ATOM_HALF, "full": _cabi.CF_PAIR_LIST_FULL}
    HANDOVERS = {"event": _cabi.CF_HANDOVER_EVENT, "memory": _cabi.CF_HANDOVER_MEMORY}

    def __init__(self, device: int = 0, stream=None, rank: int = 0, world_size: int = 1, kspace_algo: int = 0,
                 grid_width: int = 0, precision: str = "double", one_4pi_eps0: float = 0.0,
                 pair_list: str = "auto", handover: str = "event", variants: int = 0, list_capacity: int = 0):
        """one_4pi_eps0: ONE_4PI_EPS0 of the OpenMM the force is evaluated for (the reference
        takes it from openmm/reference/SimTKOpenMMRealType.h, ReferenceCoulKernels.cpp:7);
        0 = 138.935456 (OpenMM 7.x), _cabi.ONE_4PI_EPS0_CODATA2018 for OpenMM 8.x.
        pair_list, handover, variants, list_capacity: cf_options fields (include/chargeflux.h):
        the neighbour-list kind ("auto", "cluster", "atom_half", "full"), the second stream's
        fork / join ("event" or the opt-in "memory"), CF_VARIANT_* bits (alternative kernels of the
        same sums) and the cluster-pair list capacity (0 = automatic)."""
        if pair_list not in self.PAIR_LISTS:
            raise ValueError(f"pair_list must be one of {sorted(self.PAIR_LISTS)}")
        if handover not in self.HANDOVERS:
            raise ValueError(f"handover must be one of {sorted(self.HANDOVERS)}")
        self._pair_list = self.PAIR_LISTS[pair_list]
        self._handover = self.HANDOVERS[handover]
        self._variants = int(variants)
        self._list_capacity = int(list_capacity)
        self._lib = _cabi.load_library()
        self._ke = float(one_4pi_eps0)
        self._grid_width = grid_width
        if precision not in ("double", "mixed"):
            raise ValueError("precision must be 'double' or 'mixed'")
        self._precision = _cabi.CF_PRECISION_MIXED if precision == "mixed" else _cabi.CF_PRECISION_DOUBLE
        self._h = C.c_void_p()
        self._device = device
        self._stream = stream
        self._rank, self._world = rank, world_size
        self._algo = kspace_algo
        self._n = 0
        self._pbc = False

    # -------------------------------------------------------------------------------
    def initialize(self, system, force: CoulForce):
        if system.getNumParticles() != force.getNumParticles():
            raise _cabi.ChargeFluxError(_cabi.CF_ERR_INVALID,
                                        "System and CoulForce have different numbers of particles")
        a, b, c = system.getDefaultPeriodicBoxVectors()
        box = np.array([a, b, c], dtype=np.float64).reshape(9)
        params, keep = force.to_cparams(box, self._ke)
        opt = _cabi.cf_options()
        opt.device = self._device
        opt.stream = C.c_void_p(self._stream) if self._stream else None
        opt.rank, opt.world_size, opt.kspace_algo = self._rank, self._world, self._algo
        opt.grid_width = self._grid_width
        opt.precision = self._precision
        opt.handover, opt.pair_list = self._handover, self._pair_list
        opt.variants, opt.list_capacity = self._variants, self._list_capacity
        self.destroy()
        _cabi.check(self._lib.cf_create(C.byref(params), C.byref(opt), C.byref(self._h)), self._lib)
        del keep
        self._n = force.getNumParticles()
        self._pbc = force.usesPeriodicBoundaryConditions()
        return self

    def copyParametersToContext(self, force: CoulForce):
        """New charges / LJ / flux parameters on the same topology (cf_update_parameters; the
        reference has no updateParametersInContext)."""
        if force.getNumParticles() != self._n:
            raise _cabi.ChargeFluxError(_cabi.CF_ERR_INVALID, "the number of particles has changed")
        params, keep = force.to_cparams(None, self._ke)
        _cabi.check(self._lib.cf_update_parameters(self._h, C.byref(params)), self._lib)
        del keep

    def destroy(self):
        if self._h:
            self._lib.cf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -------------------------------------------------------------------------------
    def ewald_params(self):
        alpha = C.c_double()
        kmax = (C.c_int32 * 3)()
        _cabi.check(self._lib.cf_get_ewald_params(self._h, C.byref(alpha), kmax), self._lib)
        return alpha.value, tuple(kmax)

    def grid_shape(self):
        """Grid points per axis of the grid reciprocal path ((0, 0, 0) for the exact paths)."""
        ng = (C.c_int32 * 3)()
        w = C.c_int32()
        _cabi.check(self._lib.cf_get_grid_shape(self._h, ng, C.byref(w)), self._lib)
        return tuple(ng)

    def grid_width(self) -> int:
        """ES kernel width W the grid reciprocal path uses (0 for the exact paths)."""
        ng = (C.c_int32 * 3)()
        w = C.c_int32()
        _cabi.check(self._lib.cf_get_grid_shape(self._h, ng, C.byref(w)), self._lib)
        return int(w.value)

    def set_neighbor_skin(self, skin: float):
        """Persistent neighbour list with a skin (nm); 0 = rebuild on every execute (the
        reference's behaviour, ReferenceCoulKernels.cpp:559).  See include/chargeflux.h."""
        _cabi.check(self._lib.cf_set_neighbor_skin(self._h, float(skin)), self._lib)
        return self

    def set_graph(self, enable: bool = True):
        """Replay single-rank evaluations as a captured hipGraph (cf_set_graph): the same kernels
        in the same order, without the per-launch host cost."""
        _cabi.check(self._lib.cf_set_graph(self._h, 1 if enable else 0), self._lib)
        return self

    def set_overlap(self, enable: bool = True):
        """Second stream for the grid path (cf_set_overlap, default on): off launches every kernel
        on the handle's stream, so that kernel durations are the kernels' own; same results."""
        _cabi.check(self._lib.cf_set_overlap(self._h, 1 if enable else 0), self._lib)
        return self

    def graph_stats(self):
        """(captures, replays) since set_graph(True)."""
        c, r = C.c_int64(), C.c_int64()
        _cabi.check(self._lib.cf_get_graph_stats(self._h, C.byref(c), C.byref(r)), self._lib)
        return c.value, r.value

    def pair_list(self):
        """The direct-space list in use: "cluster", "atom_half" or "full" ("auto" before the first
        periodic evaluation and without PBC) -- cf_get_pair_list."""
        k = C.c_int32()
        _cabi.check(self._lib.cf_get_pair_list(self._h, C.byref(k)), self._lib)
        return {v: n for n, v in self.PAIR_LISTS.items()}[k.value]

    def neighbor_stats(self):
        """(list builds, evaluations) since initialize."""
        b, e = C.c_int64(), C.c_int64()
        _cabi.check(self._lib.cf_get_neighbor_stats(self._h, C.byref(b), C.byref(e)), self._lib)
        return b.value, e.value

    def fallback_stats(self):
        """(evaluations that fell back to the fp64 rescan of every atom, list rows rescanned
        after a full-list overflow, union of the reasons: 1 window > 4096 atoms, 2 list overflow /
        unplaceable rows, 4 fixed-point range) since initialize: slow-path diagnostics."""
        a, b, r = C.c_int64(), C.c_int64(), C.c_int32()
        _cabi.check(self._lib.cf_get_fallback_stats(self._h, C.byref(a), C.byref(b), C.byref(r)), self._lib)
        return a.value, b.value, r.value

    def owned_range(self):
        lo, hi = C.c_int32(), C.c_int32()
        _cabi.check(self._lib.cf_get_owned_range(self._h, C.byref(lo), C.byref(hi)), self._lib)
        return lo.value, hi.value

    @staticmethod
    def _flags(include_forces, include_energy):
        return (_cabi.CF_INCLUDE_FORCES if include_forces else 0) | (_cabi.CF_INCLUDE_ENERGY if include_energy else 0)

    def execute_host(self, positions, box=None, includeForces=True, includeEnergy=True, forces=None):
        """Host-memory execute: positions (N,3) nm; forces (N,3) float64 array ADDED to
        (created if None).  Returns (energy, forces)."""
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(self._n, 3))
        if forces is None:
            forces = np.zeros((self._n, 3))
        if forces.dtype != np.float64 or not forces.flags.c_contiguous or forces.shape != (self._n, 3):
            raise ValueError("forces must be a C-contiguous float64 (N,3) array")
        e = C.c_double()
        b9 = _box9(box)
        _cabi.check(self._lib.cf_compute_host(self._h, _dp(pos), _dp(b9), self._flags(includeForces, includeEnergy),
                                              _dp(forces), C.byref(e)), self._lib)
        return e.value, forces

    def execute_device(self, positions, box=None, includeForces=True, includeEnergy=True, forces=None, energy=None):
        """Device execute on torch tensors (float64, cuda): forces (N,3) ADDED to, energy
        (1,) overwritten.  Asynchronous on the kernel's stream."""
        b9 = _box9(box)
        fptr = forces.data_ptr() if forces is not None else None
        eptr = energy.data_ptr() if energy is not None else None
        _cabi.check(self._lib.cf_compute(self._h, C.c_void_p(positions.data_ptr()), _dp(b9),
                                         self._flags(includeForces, includeEnergy), C.c_void_p(fptr),
                                         C.c_void_p(eptr)), self._lib)

    def execute_openmm(self, posq, atom_index, padded_n, box=None, includeForces=True, includeEnergy=True,
                       force_buffer=None, energy_buffer=None, posq_correction=None):
        """Execute on an OpenMM GPU platform's own buffers (cf_compute_openmm; the reference's CUDA
        platform binds them at CudaCoulKernels.cpp:523-600): posq (N, 4) float64 or float32 torch
        tensor in the platform's sorted order, atom_index (N,) int32 (sorted slot -> atom),
        force_buffer (3 * padded_n,) int64 fixed point (2^-32 kJ/mol/nm, x | y | z planes by sorted
        slot) ADDED to, energy_buffer a one-element float64 / float32 tensor ADDED to; posq_correction
        (N, 4) float32 for the mixed-precision platform.  posq is never written."""
        import torch
        kind = _cabi.CF_POSQ_FLOAT4 if posq.dtype == torch.float32 else _cabi.CF_POSQ_DOUBLE4
        ekind = _cabi.CF_ENERGY_FLOAT if (energy_buffer is not None and energy_buffer.dtype == torch.float32) \
            else _cabi.CF_ENERGY_DOUBLE
        b9 = _box9(box)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _cabi.check(self._lib.cf_compute_openmm(self._h, ptr(posq), ptr(posq_correction), kind, ptr(atom_index),
                                                int(padded_n), _dp(b9), self._flags(includeForces, includeEnergy),
                                                ptr(force_buffer), ptr(energy_buffer), ekind), self._lib)

    # batched evaluation (cf_compute_batch: non-periodic systems; boxes=: periodic ones; one rank) ---
    def _check_batch_array(self, a, name, trailing, module=np):
        """(B,) + trailing, float64, C-contiguous -- checked before the C call."""
        shape = tuple(a.shape)
        if len(shape) != 1 + len(trailing) or shape[1:] != trailing:
            raise ValueError(f"{name} must have shape (B,) + {trailing}, got {shape}")
        if module is np:
            ok = a.dtype == np.float64 and a.flags.c_contiguous
        else:
            ok = a.dtype == module.float64 and a.is_contiguous()
        if not ok:
            raise ValueError(f"{name} must be a C-contiguous float64 array")
        return shape[0]

    @staticmethod
    def _batch_boxes(boxes, nconf):
        """boxes of a periodic batch -> C-contiguous float64 (nconf, 3, 3) host array: (B, 3, 3), or
        (3, 3) broadcast to every conformation -- checked before the C call."""
        if not isinstance(boxes, np.ndarray) or boxes.dtype != np.float64 or not boxes.flags.c_contiguous:
            raise ValueError("boxes must be a C-contiguous float64 numpy array (host memory)")
        if boxes.shape == (3, 3):
            return np.ascontiguousarray(np.broadcast_to(boxes, (nconf, 3, 3)))
        if boxes.ndim != 3 or boxes.shape[1:] != (3, 3):
            raise ValueError(f"boxes must have shape (B, 3, 3) or (3, 3), got {boxes.shape}")
        if boxes.shape[0] != nconf:
            raise ValueError(f"boxes holds {boxes.shape[0]} boxes for {nconf} conformations")
        return boxes

    def execute_batch_host(self, positions, includeForces=True, includeEnergy=True, forces=None,
                           return_charges=True, *, boxes=None):
        """B conformations of the system in one call (cf_compute_batch_host): positions (B,N,3)
        float64 C-contiguous numpy array; forces (B,N,3) ADDED to (created if None).  Returns
        (energies (B,), forces (B,N,3), charges (B,N) after flux, or None).
        boxes (periodic systems, cf_compute_batch_periodic_host): float64 numpy (B,3,3), one box
        per conformation (rows a, b, c, OpenMM's reduced form), or (3,3) for all of them."""
        if not isinstance(positions, np.ndarray):
            raise ValueError("positions must be a numpy array of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3))
        if forces is None:
            forces = np.zeros((nconf, self._n, 3))
        elif not isinstance(forces, np.ndarray) or self._check_batch_array(forces, "forces", (self._n, 3)) != nconf:
            raise ValueError("forces must be a float64 numpy array shaped like positions")
        energies = np.zeros(nconf)
        charges = np.zeros((nconf, self._n)) if return_charges else None
        if boxes is not None:
            b = self._batch_boxes(boxes, nconf)
            _cabi.check(self._lib.cf_compute_batch_periodic_host(
                self._h, nconf, _dp(positions), _dp(b), self._flags(includeForces, includeEnergy), _dp(forces),
                _dp(energies), _dp(charges) if return_charges else None), self._lib)
            return energies, forces, charges
        _cabi.check(self._lib.cf_compute_batch_host(self._h, nconf, _dp(positions),
                                                    self._flags(includeForces, includeEnergy), _dp(forces),
                                                    _dp(energies), _dp(charges) if return_charges else None),
                    self._lib)
        return energies, forces, charges

    def execute_batch_device(self, positions, includeForces, includeEnergy, forces=None, energies=None,
                             charges=None, *, boxes=None):
        """The same on torch tensors (float64, on the kernel's device, contiguous): positions
        (B,N,3); forces (B,N,3) ADDED to, energies (B,) and charges (B,N) overwritten; each output
        may be None.  Asynchronous on the kernel's stream.
        boxes (periodic systems, cf_compute_batch_periodic): as execute_batch_host -- a numpy array
        in HOST memory here too, read during the call."""
        import torch
        if not isinstance(positions, torch.Tensor):
            raise ValueError("positions must be a torch tensor of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3), torch)
        for t, name, trailing in ((forces, "forces", (self._n, 3)), (energies, "energies", ()),
                                  (charges, "charges", (self._n,))):
            if t is not None and (not isinstance(t, torch.Tensor)
                                  or self._check_batch_array(t, name, trailing, torch) != nconf):
                raise ValueError(f"{name} must be a float64 torch tensor for {nconf} conformations")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if boxes is not None:
            b = self._batch_boxes(boxes, nconf)
            _cabi.check(self._lib.cf_compute_batch_periodic(
                self._h, nconf, ptr(positions), _dp(b), self._flags(includeForces, includeEnergy), ptr(forces),
                ptr(energies), ptr(charges)), self._lib)
            return
        _cabi.check(self._lib.cf_compute_batch(self._h, nconf, ptr(positions),
                                               self._flags(includeForces, includeEnergy), ptr(forces),
                                               ptr(energies), ptr(charges)), self._lib)

    # parameter gradients of the batch (cf_compute_batch_vjp; boxes=: cf_compute_batch_periodic_vjp) --
    def param_counts(self):
        """(N, 2 * bonds, 2 * angles, 5 * waters): the lengths of the four parameter groups of a
        gradient row (cf_get_param_counts); P is their sum."""
        c = (C.c_int32 * 4)()
        _cabi.check(self._lib.cf_get_param_counts(self._h, c), self._lib)
        return tuple(c)

    def _check_cotangents(self, nconf, energy_bar, charges_bar, forces_bar, module, kind):
        for t, name, trailing in ((energy_bar, "energy_bar", ()), (charges_bar, "charges_bar", (self._n,)),
                                  (forces_bar, "forces_bar", (self._n, 3))):
            if t is not None and (not isinstance(t, kind)
                                  or self._check_batch_array(t, name, trailing, module) != nconf):
                raise ValueError(f"{name} must be a float64 {kind.__name__} for {nconf} conformations")

    def execute_batch_vjp_host(self, positions, energy_bar=None, charges_bar=None, forces_bar=None, *, boxes=None):
        """Gradients of L = energy_bar . E + charges_bar . q + forces_bar . F with respect to the base
        charges and the flux parameters, per conformation (cf_compute_batch_vjp_host; non-periodic
        systems).  positions (B,N,3), energy_bar (B,), charges_bar (B,N), forces_bar (B,N,3):
        C-contiguous float64 numpy arrays, a cotangent may be None (= zero).  Returns a dict:
        charges (B,N), bonds (B,nb,2) as (k, b), angles (B,na,2) as (k, theta0), waters (B,nw,5) as
        (k1, k2, kub, b0, ub0) -- views of one (B,P) array, which is returned as flat.
        boxes (periodic systems, cf_compute_batch_periodic_vjp_host): as execute_batch_host --
        float64 numpy (B,3,3), one box per conformation, or (3,3) for all of them."""
        if not isinstance(positions, np.ndarray):
            raise ValueError("positions must be a numpy array of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3))
        self._check_cotangents(nconf, energy_bar, charges_bar, forces_bar, np, np.ndarray)
        b = self._batch_boxes(boxes, nconf) if boxes is not None else None
        counts = self.param_counts()
        flat = np.zeros((nconf, sum(counts)))
        opt = lambda a: _dp(a) if a is not None else None
        if b is not None:
            _cabi.check(self._lib.cf_compute_batch_periodic_vjp_host(
                self._h, nconf, _dp(positions), _dp(b), opt(energy_bar), opt(charges_bar), opt(forces_bar),
                _dp(flat)), self._lib)
            return self.split_gradient(flat, counts)
        _cabi.check(self._lib.cf_compute_batch_vjp_host(self._h, nconf, _dp(positions), opt(energy_bar),
                                                        opt(charges_bar), opt(forces_bar), _dp(flat)), self._lib)
        return self.split_gradient(flat, counts)

    @staticmethod
    def split_gradient(flat, counts):
        """Views of a (B,P) gradient array (numpy or torch) by parameter group."""
        n, b2, a2, w5 = counts
        nconf = flat.shape[0]
        o1, o2, o3 = n, n + b2, n + b2 + a2
        return {"flat": flat, "charges": flat[:, :o1], "bonds": flat[:, o1:o2].reshape(nconf, b2 // 2, 2),
                "angles": flat[:, o2:o3].reshape(nconf, a2 // 2, 2),
                "waters": flat[:, o3:o3 + w5].reshape(nconf, w5 // 5, 5)}

    def execute_batch_vjp_device(self, positions, grad, energy_bar=None, charges_bar=None, forces_bar=None, *,
                                 boxes=None):
        """The same on torch tensors (float64, on the kernel's device, contiguous): grad (B,P) is
        overwritten (split_gradient gives its views).  Asynchronous on the kernel's stream.
        boxes (periodic systems, cf_compute_batch_periodic_vjp): a numpy array in HOST memory here
        too, read during the call."""
        import torch
        if not isinstance(positions, torch.Tensor):
            raise ValueError("positions must be a torch tensor of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3), torch)
        self._check_cotangents(nconf, energy_bar, charges_bar, forces_bar, torch, torch.Tensor)
        b = self._batch_boxes(boxes, nconf) if boxes is not None else None
        if not isinstance(grad, torch.Tensor):
            raise ValueError("grad must be a torch tensor of shape (B, P)")
        if self._check_batch_array(grad, "grad", (sum(self.param_counts()),), torch) != nconf:
            raise ValueError(f"grad must hold {nconf} conformations")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if b is not None:
            _cabi.check(self._lib.cf_compute_batch_periodic_vjp(
                self._h, nconf, ptr(positions), _dp(b), ptr(energy_bar), ptr(charges_bar), ptr(forces_bar),
                ptr(grad)), self._lib)
            return
        _cabi.check(self._lib.cf_compute_batch_vjp(self._h, nconf, ptr(positions), ptr(energy_bar), ptr(charges_bar),
                                                   ptr(forces_bar), ptr(grad)), self._lib)

    # LJ sigma / epsilon gradients of both batches (cf_compute_batch_lj_vjp) ---------------------------
    def execute_batch_lj_vjp_host(self, positions, energy_bar=None, forces_bar=None, *, boxes=None):
        """Gradients of L = energy_bar . E + forces_bar . F with respect to every atom's LJ sigma and
        epsilon, per conformation (cf_compute_batch_lj_vjp_host).  positions (B,N,3), energy_bar
        (B,), forces_bar (B,N,3): C-contiguous float64 numpy arrays, a cotangent may be None
        (= zero).  Returns a dict: sigmas (B,N), epsilons (B,N) -- views of one (B,2N) array, which
        is returned as flat.  An atom with epsilon = 0 receives exactly 0 for both.
        boxes: required for a periodic system, as execute_batch_host -- float64 numpy (B,3,3), one
        box per conformation, or (3,3) for all of them; None for a non-periodic one."""
        if not isinstance(positions, np.ndarray):
            raise ValueError("positions must be a numpy array of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3))
        self._check_cotangents(nconf, energy_bar, None, forces_bar, np, np.ndarray)
        b = self._batch_boxes(boxes, nconf) if boxes is not None else None
        flat = np.zeros((nconf, 2 * self._n))
        opt = lambda a: _dp(a) if a is not None else None
        _cabi.check(self._lib.cf_compute_batch_lj_vjp_host(self._h, nconf, _dp(positions), opt(b), opt(energy_bar),
                                                           opt(forces_bar), _dp(flat)), self._lib)
        return {"flat": flat, "sigmas": flat[:, :self._n], "epsilons": flat[:, self._n:]}

    def execute_batch_lj_vjp_device(self, positions, grad, energy_bar=None, forces_bar=None, *, boxes=None):
        """The same on torch tensors (float64, on the kernel's device, contiguous): grad (B,2N) is
        overwritten, sigmas then epsilons per conformation.  Asynchronous on the kernel's stream.
        boxes: a numpy array in HOST memory here too, read during the call."""
        import torch
        if not isinstance(positions, torch.Tensor):
            raise ValueError("positions must be a torch tensor of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3), torch)
        self._check_cotangents(nconf, energy_bar, None, forces_bar, torch, torch.Tensor)
        b = self._batch_boxes(boxes, nconf) if boxes is not None else None
        if not isinstance(grad, torch.Tensor):
            raise ValueError("grad must be a torch tensor of shape (B, 2 N)")
        if self._check_batch_array(grad, "grad", (2 * self._n,), torch) != nconf:
            raise ValueError(f"grad must hold {nconf} conformations")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _cabi.check(self._lib.cf_compute_batch_lj_vjp(self._h, nconf, ptr(positions), _dp(b) if b is not None else None,
                                                      ptr(energy_bar), ptr(forces_bar), ptr(grad)), self._lib)

    # dipoles and atomic polar tensors of the non-periodic batch (cf_compute_batch_dipole, _vjp) --------
    def execute_batch_dipole_host(self, positions):
        """Dipoles and atomic polar tensors of B conformations (cf_compute_batch_dipole_host;
        non-periodic systems).  positions (B,N,3): C-contiguous float64 numpy array.  Returns
        (dipoles (B,3) in e nm about the coordinate origin, apts (B,N,3,3) with apts[c, b, i, j] =
        d dipole_i / d x_bj in e, charges (B,N) after flux: execute_batch_host's, to the bit)."""
        if not isinstance(positions, np.ndarray):
            raise ValueError("positions must be a numpy array of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3))
        dipoles, apts, charges = np.zeros((nconf, 3)), np.zeros((nconf, self._n, 3, 3)), np.zeros((nconf, self._n))
        _cabi.check(self._lib.cf_compute_batch_dipole_host(self._h, nconf, _dp(positions), _dp(dipoles), _dp(apts),
                                                           _dp(charges)), self._lib)
        return dipoles, apts, charges

    def execute_batch_dipole_device(self, positions, dipoles=None, apts=None, charges=None):
        """The same on torch tensors (float64, on the kernel's device, contiguous): positions
        (B,N,3); dipoles (B,3), apts (B,N,3,3) and charges (B,N) overwritten, each may be None.
        Asynchronous on the kernel's stream."""
        import torch
        if not isinstance(positions, torch.Tensor):
            raise ValueError("positions must be a torch tensor of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3), torch)
        for t, name, trailing in ((dipoles, "dipoles", (3,)), (apts, "apts", (self._n, 3, 3)),
                                  (charges, "charges", (self._n,))):
            if t is not None and (not isinstance(t, torch.Tensor)
                                  or self._check_batch_array(t, name, trailing, torch) != nconf):
                raise ValueError(f"{name} must be a float64 torch tensor for {nconf} conformations")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _cabi.check(self._lib.cf_compute_batch_dipole(self._h, nconf, ptr(positions), ptr(dipoles), ptr(apts),
                                                      ptr(charges)), self._lib)

    def _check_dipole_cotangents(self, nconf, dipole_bar, apt_bar, module, kind):
        for t, name, trailing in ((dipole_bar, "dipole_bar", (3,)), (apt_bar, "apt_bar", (self._n, 3, 3))):
            if t is not None and (not isinstance(t, kind)
                                  or self._check_batch_array(t, name, trailing, module) != nconf):
                raise ValueError(f"{name} must be a float64 {kind.__name__} for {nconf} conformations")

    def execute_batch_dipole_vjp_host(self, positions, dipole_bar=None, apt_bar=None):
        """Gradients of L = dipole_bar . dipole + apt_bar : apt with respect to the base charges and
        the flux parameters, per conformation (cf_compute_batch_dipole_vjp_host).  positions (B,N,3),
        dipole_bar (B,3), apt_bar (B,N,3,3): C-contiguous float64 numpy arrays, a cotangent may be
        None (= zero).  Returns the dict of execute_batch_vjp_host (split_gradient)."""
        if not isinstance(positions, np.ndarray):
            raise ValueError("positions must be a numpy array of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3))
        self._check_dipole_cotangents(nconf, dipole_bar, apt_bar, np, np.ndarray)
        counts = self.param_counts()
        flat = np.zeros((nconf, sum(counts)))
        opt = lambda a: _dp(a) if a is not None else None
        _cabi.check(self._lib.cf_compute_batch_dipole_vjp_host(self._h, nconf, _dp(positions), opt(dipole_bar),
                                                               opt(apt_bar), _dp(flat)), self._lib)
        return self.split_gradient(flat, counts)

    def execute_batch_dipole_vjp_device(self, positions, grad, dipole_bar=None, apt_bar=None):
        """The same on torch tensors (float64, on the kernel's device, contiguous): grad (B,P) is
        overwritten (split_gradient gives its views).  Asynchronous on the kernel's stream."""
        import torch
        if not isinstance(positions, torch.Tensor):
            raise ValueError("positions must be a torch tensor of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3), torch)
        self._check_dipole_cotangents(nconf, dipole_bar, apt_bar, torch, torch.Tensor)
        if not isinstance(grad, torch.Tensor):
            raise ValueError("grad must be a torch tensor of shape (B, P)")
        if self._check_batch_array(grad, "grad", (sum(self.param_counts()),), torch) != nconf:
            raise ValueError(f"grad must hold {nconf} conformations")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _cabi.check(self._lib.cf_compute_batch_dipole_vjp(self._h, nconf, ptr(positions), ptr(dipole_bar),
                                                          ptr(apt_bar), ptr(grad)), self._lib)

    # Hessian-vector products of the non-periodic batch (cf_compute_batch_hvp) --------------------------
    def _check_hvp_vectors(self, vectors, nconf, module, kind):
        if not isinstance(vectors, kind):
            raise ValueError(f"vectors must be a float64 {kind.__name__} of shape (B, K, N, 3)")
        shape = tuple(vectors.shape)
        if len(shape) != 4:
            raise ValueError(f"vectors must have shape (B, K, N, 3), got {shape}")
        if self._check_batch_array(vectors, "vectors", (shape[1], self._n, 3), module) != nconf:
            raise ValueError(f"vectors holds {shape[0]} conformations, positions {nconf}")
        return shape[1]

    def execute_batch_hvp_host(self, positions, vectors):
        """Hessian-vector products of B conformations (cf_compute_batch_hvp_host; non-periodic
        systems).  positions (B,N,3) in nm, vectors (B,K,N,3): C-contiguous float64 numpy arrays, K
        directions per conformation.  Returns (B,K,N,3): H(x_b) v_bk, with H = d2E/dxdx of the energy
        execute_batch_host returns (kJ/mol/nm^2 for v in nm)."""
        if not isinstance(positions, np.ndarray):
            raise ValueError("positions must be a numpy array of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3))
        nvec = self._check_hvp_vectors(vectors, nconf, np, np.ndarray)
        out = np.zeros((nconf, nvec, self._n, 3))
        _cabi.check(self._lib.cf_compute_batch_hvp_host(self._h, nconf, _dp(positions), nvec, _dp(vectors), _dp(out)),
                    self._lib)
        return out

    def execute_batch_hvp_device(self, positions, vectors, out=None):
        """The same on torch tensors (float64, on the kernel's device, contiguous): out (B,K,N,3) is
        overwritten (created if None) and returned.  Asynchronous on the kernel's stream."""
        import torch
        if not isinstance(positions, torch.Tensor):
            raise ValueError("positions must be a torch tensor of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3), torch)
        nvec = self._check_hvp_vectors(vectors, nconf, torch, torch.Tensor)
        if out is None:
            out = torch.empty_like(vectors)
        elif (not isinstance(out, torch.Tensor)
              or self._check_batch_array(out, "out", (nvec, self._n, 3), torch) != nconf):
            raise ValueError("out must be a float64 torch tensor shaped like vectors")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        _cabi.check(self._lib.cf_compute_batch_hvp(self._h, nconf, ptr(positions), nvec, ptr(vectors), ptr(out)),
                    self._lib)
        return out

    def hessians_host(self, positions, symmetrize=True):
        """Full Hessians (B,3N,3N) of B conformations: one execute_batch_hvp_host call with the 3N unit
        vectors per conformation, symmetrised as (H + H^T) / 2 (symmetrize=False: the products as they
        come, row k = H e_k)."""
        if not isinstance(positions, np.ndarray):
            raise ValueError("positions must be a numpy array of shape (B, N, 3)")
        nconf = self._check_batch_array(positions, "positions", (self._n, 3))
        n3 = 3 * self._n
        units = np.ascontiguousarray(np.broadcast_to(np.eye(n3).reshape(n3, self._n, 3), (nconf, n3, self._n, 3)))
        hess = self.execute_batch_hvp_host(positions, units).reshape(nconf, n3, n3)
        return 0.5 * (hess + hess.transpose(0, 2, 1)) if symmetrize else hess

    def set_batch_limit(self, n: int):
        """Conformations evaluated per pass of a batch (bounds the batch workspace); 0 = automatic
        (a 256 MiB workspace).  Results do not depend on it."""
        _cabi.check(self._lib.cf_set_batch_limit(self._h, int(n)), self._lib)
        return self

    def batch_stats(self):
        """(batch calls, conformations evaluated, passes launched) since initialize."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _cabi.check(self._lib.cf_get_batch_stats(self._h, C.byref(a), C.byref(b), C.byref(c)), self._lib)
        return a.value, b.value, c.value

    def device_errors(self):
        """CF_GUARD_* bits of the device index guards tripped so far (0 = none; synchronises)."""
        v = C.c_int32()
        _cabi.check(self._lib.cf_get_device_errors(self._h, C.byref(v)), self._lib)
        return v.value

    # split-phase (multi-GPU): begin -> all-reduce kspace_buffer -> end
    def begin(self, positions, box=None, includeForces=True, includeEnergy=True):
        self._b9 = _box9(box)
        _cabi.check(self._lib.cf_compute_begin(self._h, C.c_void_p(positions.data_ptr()), _dp(self._b9),
                                               self._flags(includeForces, includeEnergy)), self._lib)

    def kspace_buffer(self):
        ptr, n = C.c_void_p(), C.c_int64()
        _cabi.check(self._lib.cf_kspace_buffer(self._h, C.byref(ptr), C.byref(n)), self._lib)
        return ptr.value, n.value

    def kspace_tensor(self, device):
        """The structure-factor buffer as a zero-copy torch tensor (None without PBC)."""
        ptr, n = self.kspace_buffer()
        if not n:
            return None
        from .distributed import device_buffer_as_tensor
        return device_buffer_as_tensor(ptr, n, device)

    def direct(self):
        """Launch the direct-space kernels of the begun evaluation now (optional; lets a
        multi-rank caller overlap them with the S(k) all-reduce)."""
        _cabi.check(self._lib.cf_compute_direct(self._h), self._lib)

    def end(self, forces=None, energy=None):
        fptr = forces.data_ptr() if forces is not None else None
        eptr = energy.data_ptr() if energy is not None else None
        _cabi.check(self._lib.cf_compute_end(self._h, C.c_void_p(fptr), C.c_void_p(eptr)), self._lib)

    def execute(self, context, includeForces, includeEnergy):
        """OpenMM-style execute(ContextImpl&, bool, bool) -> energy (ReferenceCoulKernels.cpp:424)."""
        return context._execute_kernel(self, includeForces, includeEnergy)

    # diagnostics ----------------------------------------------------------------------
    def charges(self):
        out = np.zeros(self._n)
        _cabi.check(self._lib.cf_get_charges(self._h, _dp(out)), self._lib)
        return out

    def dedq(self):
        out = np.zeros(self._n)
        _cabi.check(self._lib.cf_get_dedq(self._h, _dp(out)), self._lib)
        return out

    def energy_terms(self):
        out = np.zeros(4)
        _cabi.check(self._lib.cf_get_energy_terms(self._h, _dp(out)), self._lib)
        return out

    # phase names in cf_get_timing order (bit p of cf_set_timing_mask)
    PHASES = ("flux_terms", "atoms_prep", "cell_sort", "neighbor_list", "kspace_tables", "kspace_sfac",
              "kspace_coeffs", "kspace_force", "direct_pairs", "assemble", "energy", "grid_sort", "grid_spread",
              "grid_dft_fwd", "grid_dft_inv", "grid_interp", "direct_excl")

    def set_timing(self, enable=True, phases=None):
        """Per-kernel HIP-event timing of every phase, or only of the named phases."""
        if phases is None:
            _cabi.check(self._lib.cf_set_timing(self._h, 1 if enable else 0), self._lib)
        else:
            mask = 0
            for p in phases:
                mask |= 1 << self.PHASES.index(p)
            _cabi.check(self._lib.cf_set_timing_mask(self._h, mask if enable else 0), self._lib)

    def timing(self):
        """{phase: (total_ms, launches)} recorded since set_timing(True)."""
        nmax = 32
        names = C.create_string_buffer(16 * nmax)
        tot = (C.c_double * nmax)()
        calls = (C.c_int32 * nmax)()
        nph = C.c_int32()
        _cabi.check(self._lib.cf_get_timing(self._h, nmax, names, tot, calls, C.byref(nph)), self._lib)
        out = {}
        for p in range(nph.value):
            nm = names.raw[16 * p:16 * p + 16].split(b"\0")[0].decode()
            out[nm] = (tot[p], calls[p])
        return out

    def synchronize(self):
        _cabi.check(self._lib.cf_synchronize(self._h), self._lib)


class State:
    def __init__(self, energy, forces):
        self._e, self._f = energy, forces

    def getPotentialEnergy(self):
        return self._e

    def getForces(self, asNumpy=True):
        return self._f


class Context:
    """Minimal OpenMM-Context mirror: owns one HipCalcCoulForceKernel per CoulForce in the
    System (CoulForceImpl::initialize, CoulForceImpl.cpp:16-21) and evaluates them with the
    force-group test of CoulForceImpl::calcForcesAndEnergy (CoulForceImpl.cpp:23-27)."""

    def __init__(self, system: System, device: int = 0, kspace_algo: int = 0, grid_width: int = 0,
                 precision: str = "double", one_4pi_eps0: float = 0.0):
        self._system = system
        self._n = system.getNumParticles()
        self._pos = np.zeros((self._n, 3))
        a, b, c = system.getDefaultPeriodicBoxVectors()
        self._box = np.array([a, b, c], dtype=np.float64)
        self._impls = []
        for f in system.getForces():
            if isinstance(f, CoulForce):
                k = HipCalcCoulForceKernel(device=device, kspace_algo=kspace_algo, grid_width=grid_width,
                                           precision=precision, one_4pi_eps0=one_4pi_eps0).initialize(system, f)
                self._impls.append((f, k))

    def setPositions(self, positions):
        self._pos = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(self._n, 3))

    def setPeriodicBoxVectors(self, a, b, c):
        self._box = np.array([a, b, c], dtype=np.float64)

    def kernels(self):
        return [k for _, k in self._impls]

    def _update_force_parameters(self, force):
        hit = False
        for f, k in self._impls:
            if f is force:
                k.copyParametersToContext(force)
                hit = True
        if not hit:
            raise ValueError("this CoulForce is not part of the Context's System")

    def _execute_kernel(self, kernel, include_forces, include_energy):
        forces = np.zeros((self._n, 3))
        e, _ = kernel.execute_host(self._pos, self._box, include_forces, include_energy, forces)
        self._last_forces = forces
        return e

    def getState(self, getEnergy=False, getForces=False, groups=-1):
        energy = 0.0
        forces = np.zeros((self._n, 3))
        for f, k in self._impls:
            if (groups & (1 << f.getForceGroup())) == 0:
                continue
            e, _ = k.execute_host(self._pos, self._box, bool(getForces), bool(getEnergy), forces)
            energy += e
        return State(energy if getEnergy else None, forces if getForces else None)
