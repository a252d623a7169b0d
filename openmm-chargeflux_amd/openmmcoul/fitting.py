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

    energies, forces, charges, virials = model.virials(q, bonds, angles, waters, positions, boxes)
    loss = ((virials - target) ** 2).sum()            # stress / pressure matching, orthorhombic frames
    loss.backward()

virials() is cf_compute_batch_periodic_virial forward; backward adds one
cf_compute_batch_periodic_virial_vjp for the virials' cotangent to the calls above.

dipoles() is cf_compute_batch_dipole forward and one cf_compute_batch_dipole_vjp backward: the dipole
mu = sum_a q_a x_a about the coordinate origin (that of a charged system moves with a translation) and
the atomic polar tensors apts[c, b, i, j] = d mu_i / d x_bj, charge-flux part included.

    potentials = model.esp(q, bonds, angles, waters, positions, points)   # non-periodic: (B,M)
    loss = ((potentials - target) ** 2).sum()         # RESP-style fit to a QM potential
    loss.backward()

esp() is cf_compute_batch_esp forward and one cf_compute_batch_esp_vjp backward: the potential
V_p = ke sum_a q_a / |r_p - x_a| of the charges after flux at M probe points per conformation.

    products = model.hvp(q, bonds, angles, waters, positions, vectors)    # non-periodic: (B,K,N,3)
    loss = (((vectors * products).sum(dim=(2, 3)) - target) ** 2).sum()   # e . H e: squared frequencies
    loss.backward()

hvp() is cf_compute_batch_hvp forward and one cf_compute_batch_hvp_vjp backward: the Hessian-vector
products H(x_b) v_bk and their closed-form parameter gradients.  With boxes= (a periodic kernel) it
is cf_compute_batch_periodic_hvp and cf_compute_batch_periodic_hvp_vjp, H at fixed box.

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


class _VirialFn(torch.autograd.Function):
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
        virials = torch.empty((nconf, 3, 3), dtype=torch.float64, device=positions.device)
        model._before()
        k.execute_batch_virial_device(positions, True, True, forces, energies, q, virials, boxes=boxes)
        model._after()
        ctx.set_materialize_grads(False)   # an output the loss does not use: a None (NULL) cotangent
        ctx.model, ctx.params, ctx.loaded = model, params, model._loads
        ctx.inputs = (charges, bonds, angles, waters)
        ctx.lj = None if sigmas is None else (sigmas, epsilons)
        ctx.boxes = boxes.copy()   # the caller may change its array before backward
        ctx.save_for_backward(positions)
        return energies, forces, q, virials

    @staticmethod
    def backward(ctx, e_bar, f_bar, q_bar, v_bar):
        # the energy, force and charge cotangents: the periodic VJP and LJ VJP calls of __call__,
        # skipped when the loss uses none of the three
        out = [None] * 9 if e_bar is None and f_bar is None and q_bar is None \
            else list(_BatchFn.backward(ctx, e_bar, f_bar, q_bar))
        if v_bar is None:
            return tuple(out)
        model = ctx.model
        k = model.kernel
        (positions,) = ctx.saved_tensors
        if model._loads != ctx.loaded:   # another forward has changed the parameters since: put these back
            model._load(ctx.params)
            ctx.loaded = model._loads
        nconf, n = positions.shape[0], positions.shape[1]
        need, need_lj = ctx.needs_input_grad[1:5], ctx.lj is not None and any(ctx.needs_input_grad[5:7])
        counts = k.param_counts()
        grad = torch.empty((nconf, sum(counts)), dtype=torch.float64, device=positions.device) if any(need) else None
        lj_grad = torch.empty((nconf, 2 * n), dtype=torch.float64, device=positions.device) if need_lj else None
        if grad is None and lj_grad is None:
            return tuple(out)
        # queued on torch's stream before _before() orders it ahead of the kernel's; alive until _after()
        cot = v_bar.detach().to(torch.float64).contiguous()
        model._before()
        k.execute_batch_virial_vjp_device(positions, ctx.boxes, grad, cot, lj_grad)
        model._after()
        add = lambda old, g, t: g.reshape(t.shape).to(t.device) if old is None else old + g.reshape(t.shape).to(t.device)
        if grad is not None:
            g = k.split_gradient(grad.sum(dim=0, keepdim=True), counts)
            for slot, (t, name) in enumerate(zip(ctx.inputs, ("charges", "bonds", "angles", "waters"))):
                if need[slot]:
                    out[1 + slot] = add(out[1 + slot], g[name][0], t)
        if lj_grad is not None:
            g = lj_grad.sum(dim=0)
            for slot, t in enumerate(ctx.lj):
                if ctx.needs_input_grad[5 + slot]:
                    out[5 + slot] = add(out[5 + slot], g[slot * n:(slot + 1) * n], t)
        return tuple(out)


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


class _EspFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, charges, bonds, angles, waters, positions, points):
        params = tuple(t.detach().to("cpu", torch.float64).contiguous() for t in (charges, bonds, angles, waters))
        model._load(params)
        k = model.kernel
        potentials = torch.empty(points.shape[:2], dtype=torch.float64, device=positions.device)
        model._before()
        k.execute_batch_esp_device(positions, points, potentials)
        model._after()
        ctx.model, ctx.params, ctx.loaded = model, params, model._loads
        ctx.inputs = (charges, bonds, angles, waters)
        ctx.save_for_backward(positions, points)
        return potentials

    @staticmethod
    def backward(ctx, esp_bar):
        model = ctx.model
        k = model.kernel
        positions, points = ctx.saved_tensors
        if not any(ctx.needs_input_grad[1:5]):
            return (None,) * 7
        if model._loads != ctx.loaded:   # another forward has changed the parameters since: put these back
            model._load(ctx.params)
            ctx.loaded = model._loads
        cot = esp_bar.detach().to(torch.float64).contiguous()
        counts = k.param_counts()
        grad = torch.empty((positions.shape[0], sum(counts)), dtype=torch.float64, device=positions.device)
        model._before()
        k.execute_batch_esp_vjp_device(positions, points, grad, cot)
        model._after()
        g = k.split_gradient(grad.sum(dim=0, keepdim=True), counts)
        out = [g[name][0].reshape(t.shape).to(t.device) if need else None
               for t, name, need in zip(ctx.inputs, ("charges", "bonds", "angles", "waters"), ctx.needs_input_grad[1:5])]
        return (None, *out, None, None)


class _HvpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, charges, bonds, angles, waters, positions, vectors, boxes):
        params = tuple(t.detach().to("cpu", torch.float64).contiguous() for t in (charges, bonds, angles, waters))
        model._load(params)
        k = model.kernel
        model._before()
        out = k.execute_batch_hvp_device(positions, vectors, boxes=boxes)
        model._after()
        ctx.model, ctx.params, ctx.loaded = model, params, model._loads
        ctx.boxes = None if boxes is None else boxes.copy()   # the caller may change its array before backward
        ctx.inputs = (charges, bonds, angles, waters)
        ctx.save_for_backward(positions, vectors)
        return out

    @staticmethod
    def backward(ctx, out_bar):
        model = ctx.model
        k = model.kernel
        positions, vectors = ctx.saved_tensors
        if not any(ctx.needs_input_grad[1:5]):
            return (None,) * 8
        if model._loads != ctx.loaded:   # another forward has changed the parameters since: put these back
            model._load(ctx.params)
            ctx.loaded = model._loads
        cot = out_bar.detach().to(torch.float64).contiguous()
        counts = k.param_counts()
        grad = torch.empty((positions.shape[0], sum(counts)), dtype=torch.float64, device=positions.device)
        model._before()
        k.execute_batch_hvp_vjp_device(positions, vectors, grad, cot, boxes=ctx.boxes)
        model._after()
        g = k.split_gradient(grad.sum(dim=0, keepdim=True), counts)
        out = [g[name][0].reshape(t.shape).to(t.device) if need else None
               for t, name, need in zip(ctx.inputs, ("charges", "bonds", "angles", "waters"), ctx.needs_input_grad[1:5])]
        return (None, *out, None, None, None)


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

    def virials(self, charges, bonds, angles, waters, positions, boxes, *, sigmas=None, epsilons=None):
        """(energies (B,), forces (B,N,3), charges (B,N), virials (B,3,3)) of B periodic frames in
        orthorhombic boxes as a differentiable function of the parameters (arguments as __call__,
        boxes required).  The first three are bitwise what __call__ returns; virials[c] = -dE/d(strain)
        is what execute_batch_virial_device writes (cf_compute_batch_periodic_virial).  Backward makes
        the calls of __call__ for the energy, force and charge cotangents and adds one
        cf_compute_batch_periodic_virial_vjp for the virials' cotangent (flux parameters and, with
        sigmas= and epsilons=, the LJ parameters in the same call); a loss that does not use the
        virials skips that call, and one that uses the virials alone skips the others."""
        if (sigmas is None) != (epsilons is None):
            raise ValueError("sigmas and epsilons must be given together, or neither")
        lj = () if sigmas is None else ((sigmas, "sigmas"), (epsilons, "epsilons"))
        for t, name in ((charges, "charges"), (bonds, "bonds"), (angles, "angles"), (waters, "waters"),
                        (positions, "positions")) + lj:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                raise ValueError(f"{name} must be a float64 torch tensor")
        if positions.requires_grad:
            raise ValueError("positions must not require grad: gradients with respect to positions are not computed")
        boxes = self.kernel._batch_boxes(boxes, positions.shape[0])   # before the parameters are loaded
        return _VirialFn.apply(self, charges, bonds, angles, waters, sigmas, epsilons, positions, boxes)

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

    def esp(self, charges, bonds, angles, waters, positions, points):
        """Electrostatic potentials (B,M) in kJ/mol/e of B conformations of a non-periodic system at
        the probe points points (B,M,3) (nm, float64, contiguous on the kernel's device) as a
        differentiable function of the four parameter tensors (arguments as __call__;
        cf_compute_batch_esp forward, one cf_compute_batch_esp_vjp summed over the conformations in
        backward).  Every atom contributes to every point; a point on an atom gives a non-finite
        value.  Neither positions nor points may require grad."""
        for t, name in ((charges, "charges"), (bonds, "bonds"), (angles, "angles"), (waters, "waters"),
                        (positions, "positions"), (points, "points")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                raise ValueError(f"{name} must be a float64 torch tensor")
        if positions.requires_grad or points.requires_grad:
            raise ValueError("positions and points must not require grad: gradients with respect to them are not computed")
        if points.dim() != 3 or points.shape[0] != positions.shape[0] or points.shape[2] != 3:   # before the parameters are loaded
            raise ValueError(f"points must have shape (B, M, 3), got {tuple(points.shape)}")
        return _EspFn.apply(self, charges, bonds, angles, waters, positions, points)

    def hvp(self, charges, bonds, angles, waters, positions, vectors, boxes=None):
        """Hessian-vector products H(x_b) v_bk (B,K,N,3) of B conformations of a non-periodic system
        along the directions vectors (B,K,N,3) (float64, contiguous on the kernel's device) as a
        differentiable function of the four parameter tensors (arguments as __call__;
        cf_compute_batch_hvp forward, one cf_compute_batch_hvp_vjp with the incoming cotangent, summed
        over the conformations, in backward).  With v a normal mode e, d(e . H e)/d(parameters) is the
        first-order shift of its squared frequency.  Neither positions nor vectors may require grad.
        boxes: for a periodic kernel, as __call__'s (a copy is kept for backward): H at fixed box,
        cf_compute_batch_periodic_hvp forward and cf_compute_batch_periodic_hvp_vjp backward."""
        for t, name in ((charges, "charges"), (bonds, "bonds"), (angles, "angles"), (waters, "waters"),
                        (positions, "positions"), (vectors, "vectors")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                raise ValueError(f"{name} must be a float64 torch tensor")
        if positions.requires_grad or vectors.requires_grad:
            raise ValueError("positions and vectors must not require grad: gradients with respect to them are not computed")
        if vectors.dim() != 4 or vectors.shape[0] != positions.shape[0] or tuple(vectors.shape[2:]) != tuple(positions.shape[1:]):   # before the parameters are loaded
            raise ValueError(f"vectors must have shape (B, K, N, 3), got {tuple(vectors.shape)}")
        if boxes is not None:   # before the parameters are loaded
            boxes = self.kernel._batch_boxes(boxes, positions.shape[0])
        return _HvpFn.apply(self, charges, bonds, angles, waters, positions, vectors, boxes)
