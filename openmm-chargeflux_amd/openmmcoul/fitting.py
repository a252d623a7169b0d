"""Fitting a charge-flux model: the batched evaluation as a differentiable torch function of the
base charges, the flux parameters and, optionally, the LJ sigma / epsilon.

    model = BatchedChargeFlux(kernel, force)          # kernel initialised with force
    energies, forces, charges = model(q, bonds, angles, waters, positions)
    energies, forces, charges = model(q, bonds, angles, waters, positions, boxes=boxes)   # periodic
    loss = ((forces - target) ** 2).mean()
    loss.backward()                                   # q.grad, bonds.grad, angles.grad, waters.grad

    sigmas, epsilons = model.lj_parameters()          # fitted together with the LJ parameters
    energies, forces, charges = model(q, bonds, angles, waters, positions, sigmas=sigmas, epsilons=epsilons)
    loss.backward()                                   # ... and sigmas.grad, epsilons.grad

Forward is cf_compute_batch, backward one cf_compute_batch_vjp (include/chargeflux.h); with boxes=,
for a periodic kernel, cf_compute_batch_periodic and one cf_compute_batch_periodic_vjp with the same
boxes.  With sigmas= and epsilons= backward adds one cf_compute_batch_lj_vjp (either kind of kernel,
the same boxes) if one of the two requires grad, and skips the other VJP call when none of its four
inputs does.  Without them the LJ parameters are taken from `force` unchanged and the path is the
one above: no extra call.  All run in libchargeflux_hip.so.  Gradients exist for the parameters
only -- not for the positions or the boxes.

    dipoles, apts = model.dipoles(q, bonds, angles, waters, positions)   # non-periodic: (B,3), (B,N,3,3)
    loss = ((dipoles - target) ** 2).sum()
    loss.backward()                                   # q.grad, bonds.grad, angles.grad, waters.grad

dipoles() is cf_compute_batch_dipole forward and one cf_compute_batch_dipole_vjp backward: the dipole
mu = sum_a q_a x_a about the coordinate origin (that of a charged system moves with a translation) and
the atomic polar tensors apts[c, b, i, j] = d mu_i / d x_bj, charge-flux part included.

Convention (cf_compute_batch_lj_vjp): an atom with epsilon = 0 receives exactly 0 for its sigma and
epsilon gradients.  The true derivative of sqrt(eps_i eps_j) is singular there; such an atom has no
LJ interaction, and an optimiser leaves it at 0.
"""
from __future__ import annotations

import torch

from .force import CoulForce
from .kernel import HipCalcCoulForceKernel


class _BatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, charges, bonds, angles, waters, sigmas, epsilons, positions, boxes):
        given = (charges, bonds, angles, waters) + (() if sigmas is None else (sigmas, epsilons))
        params = tuple(t.detach().to("cpu", torch.float64).contiguous() for t in given)
        model._load(params)
        k = model.kernel
        nconf, n = positions.shape[0], positions.shape[1]
        energies = torch.empty(nconf, dtype=torch.float64, device=positions.device)
        forces = torch.zeros((nconf, n, 3), dtype=torch.float64, device=positions.device)
        q = torch.empty((nconf, n), dtype=torch.float64, device=positions.device)
        model._before()
        k.execute_batch_device(positions, True, True, forces, energies, q, boxes=boxes)
        model._after()
        ctx.set_materialize_grads(False)   # an output the loss does not use: a None (NULL) cotangent
        ctx.model, ctx.params, ctx.loaded = model, params, model._loads
        ctx.inputs = (charges, bonds, angles, waters)
        ctx.lj = None if sigmas is None else (sigmas, epsilons)
        ctx.boxes = None if boxes is None else boxes.copy()   # the caller may change its array before backward
        ctx.save_for_backward(positions)
        return energies, forces, q

    @staticmethod
    def backward(ctx, e_bar, f_bar, q_bar):
        model = ctx.model
        k = model.kernel
        (positions,) = ctx.saved_tensors
        if model._loads != ctx.loaded:   # another forward has changed the parameters since: put these back
            model._load(ctx.params)
            ctx.loaded = model._loads
        nconf, n = positions.shape[0], positions.shape[1]
        cot = [None if t is None else t.detach().to(torch.float64).contiguous() for t in (e_bar, q_bar, f_bar)]
        out = [None] * 4
        if any(ctx.needs_input_grad[1:5]):
            counts = k.param_counts()
            grad = torch.empty((nconf, sum(counts)), dtype=torch.float64, device=positions.device)
            model._before()
            k.execute_batch_vjp_device(positions, grad, *cot, boxes=ctx.boxes)
            model._after()
            g = k.split_gradient(grad.sum(dim=0, keepdim=True), counts)
            for slot, (t, name, need) in enumerate(zip(ctx.inputs, ("charges", "bonds", "angles", "waters"),
                                                       ctx.needs_input_grad[1:5])):
                out[slot] = g[name][0].reshape(t.shape).to(t.device) if need else None
        lj = [None, None]
        if ctx.lj is not None and any(ctx.needs_input_grad[5:7]):
            grad = torch.empty((nconf, 2 * n), dtype=torch.float64, device=positions.device)
            model._before()
            k.execute_batch_lj_vjp_device(positions, grad, cot[0], cot[2], boxes=ctx.boxes)
            model._after()
            g = grad.sum(dim=0)
            for slot, (t, need) in enumerate(zip(ctx.lj, ctx.needs_input_grad[5:7])):
                lj[slot] = g[slot * n:(slot + 1) * n].reshape(t.shape).to(t.device) if need else None
        return (None, *out, *lj, None, None)


class _DipoleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, charges, bonds, angles, waters, positions):
        params = tuple(t.detach().to("cpu", torch.float64).contiguous() for t in (charges, bonds, angles, waters))
        model._load(params)
        k = model.kernel
        nconf, n = positions.shape[0], positions.shape[1]
        dipoles = torch.empty((nconf, 3), dtype=torch.float64, device=positions.device)
        apts = torch.empty((nconf, n, 3, 3), dtype=torch.float64, device=positions.device)
        model._before()
        k.execute_batch_dipole_device(positions, dipoles, apts)
        model._after()
        ctx.set_materialize_grads(False)   # an output the loss does not use: a None (NULL) cotangent
        ctx.model, ctx.params, ctx.loaded = model, params, model._loads
        ctx.inputs = (charges, bonds, angles, waters)
        ctx.save_for_backward(positions)
        return dipoles, apts

    @staticmethod
    def backward(ctx, dipole_bar, apt_bar):
        model = ctx.model
        k = model.kernel
        (positions,) = ctx.saved_tensors
        if not any(ctx.needs_input_grad[1:5]):
            return (None,) * 6
        if model._loads != ctx.loaded:   # another forward has changed the parameters since: put these back
            model._load(ctx.params)
            ctx.loaded = model._loads
        cot = [None if t is None else t.detach().to(torch.float64).contiguous() for t in (dipole_bar, apt_bar)]
        counts = k.param_counts()
        grad = torch.empty((positions.shape[0], sum(counts)), dtype=torch.float64, device=positions.device)
        model._before()
        k.execute_batch_dipole_vjp_device(positions, grad, *cot)
        model._after()
        g = k.split_gradient(grad.sum(dim=0, keepdim=True), counts)
        out = [g[name][0].reshape(t.shape).to(t.device) if need else None
               for t, name, need in zip(ctx.inputs, ("charges", "bonds", "angles", "waters"), ctx.needs_input_grad[1:5])]
        return (None, *out, None)


class BatchedChargeFlux:
    """Energies, forces and charges of B conformations as a differentiable function of the
    parameters.  kernel: a HipCalcCoulForceKernel initialised with `force` (one rank);
    force: the CoulForce whose topology, sigma and epsilon are used -- its charges and flux
    parameters are overwritten by every call, its sigma and epsilon by a call with sigmas= and
    epsilons= (and stay as that call left them).

    __call__(charges (N,), bonds (nb,2), angles (na,2), waters (nw,5), positions (B,N,3), boxes=None,
    *, sigmas=None, epsilons=None):
    float64 tensors, the parameters on any device, positions contiguous on the kernel's device and
    not requiring grad.  boxes: for a periodic kernel, a float64 numpy array in host memory, (B,3,3)
    with one box per conformation or (3,3) for all of them (execute_batch_host's); a copy is kept for
    backward, and there are no gradients with respect to it.  Returns (energies (B,), forces (B,N,3),
    charges (B,N)) on that device.
    The parameter rows are the cf_params rows: bonds (k, b), angles (k, theta0), waters
    (k1, k2, kub, b0, ub0).  sigmas, epsilons: float64 (N,) tensors (nm, kJ/mol), both or neither
    (ValueError otherwise); given, they replace the force's LJ parameters and receive gradients (an
    atom with epsilon = 0: exactly 0 for both, the convention of cf_compute_batch_lj_vjp).  A kernel
    on a stream of its own is synchronised with torch's current stream around each call."""

    def __init__(self, kernel: HipCalcCoulForceKernel, force: CoulForce):
        self.kernel, self.force = kernel, force
        self._loads = 0

    def parameters(self, device=None):
        """The force's current parameters as four leaf tensors (requires_grad) on `device`."""
        a = self.force.arrays()
        return tuple(torch.tensor(a[key], dtype=torch.float64, device=device, requires_grad=True)
                     for key in ("charges", "fbond_par", "fangle_par", "fwater_par"))

    def lj_parameters(self, device=None):
        """The force's current LJ (sigmas, epsilons) as two leaf tensors (requires_grad) on `device`."""
        a = self.force.arrays()
        return tuple(torch.tensor(a[key], dtype=torch.float64, device=device, requires_grad=True)
                     for key in ("sigmas", "epsilons"))

    def _load(self, params):
        q, bonds, angles, waters = (p.numpy() for p in params[:4])
        f = self.force
        shapes = ((f.getNumParticles(),), (f.getNumFluxBonds(), 2), (f.getNumFluxAngles(), 2), (f.getNumFluxWaters(), 5))
        for p, name, shape in zip((q, bonds, angles, waters), ("charges", "bonds", "angles", "waters"), shapes):
            if tuple(p.shape) != shape:
                raise ValueError(f"{name} must have shape {shape}, got {tuple(p.shape)}")
        f._charges = [float(v) for v in q]
        f._fbond_par = [tuple(float(v) for v in row) for row in bonds]
        f._fangle_par = [tuple(float(v) for v in row) for row in angles]
        f._fwater_par = [tuple(float(v) for v in row) for row in waters]
        if len(params) > 4:
            for p, name in zip(params[4:], ("sigmas", "epsilons")):
                if tuple(p.shape) != shapes[0]:
                    raise ValueError(f"{name} must have shape {shapes[0]}, got {tuple(p.shape)}")
            f._sigma = [float(v) for v in params[4].numpy()]
            f._eps = [float(v) for v in params[5].numpy()]
        self.kernel.copyParametersToContext(f)
        self._loads += 1

    def _before(self):
        if self.kernel._stream:   # the kernel's own stream: the inputs torch has queued must exist
            torch.cuda.current_stream().synchronize()

    def _after(self):
        if self.kernel._stream:
            self.kernel.synchronize()

    def __call__(self, charges, bonds, angles, waters, positions, boxes=None, *, sigmas=None, epsilons=None):
        if (sigmas is None) != (epsilons is None):
            raise ValueError("sigmas and epsilons must be given together, or neither")
        lj = () if sigmas is None else ((sigmas, "sigmas"), (epsilons, "epsilons"))
        for t, name in ((charges, "charges"), (bonds, "bonds"), (angles, "angles"), (waters, "waters"),
                        (positions, "positions")) + lj:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                raise ValueError(f"{name} must be a float64 torch tensor")
        if positions.requires_grad:
            raise ValueError("positions must not require grad: gradients with respect to positions are not computed")
        if boxes is not None:   # before the parameters are loaded
            self.kernel._batch_boxes(boxes, positions.shape[0])
        return _BatchFn.apply(self, charges, bonds, angles, waters, sigmas, epsilons, positions, boxes)

    def dipoles(self, charges, bonds, angles, waters, positions):
        """Dipoles (B,3) and atomic polar tensors (B,N,3,3) of B conformations of a non-periodic
        system as a differentiable function of the four parameter tensors (arguments as __call__;
        cf_compute_batch_dipole forward, one cf_compute_batch_dipole_vjp summed over the
        conformations in backward; an output the loss does not use gives a NULL cotangent).  The
        dipole is taken about the coordinate origin: for a charged system it moves with a
        translation.  apts[c, b, i, j] = d dipole_i / d x_bj."""
        for t, name in ((charges, "charges"), (bonds, "bonds"), (angles, "angles"), (waters, "waters"),
                        (positions, "positions")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                raise ValueError(f"{name} must be a float64 torch tensor")
        if positions.requires_grad:
            raise ValueError("positions must not require grad: gradients with respect to positions are not computed")
        return _DipoleFn.apply(self, charges, bonds, angles, waters, positions)
