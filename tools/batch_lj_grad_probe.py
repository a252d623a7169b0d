"""Cost of the LJ sigma / epsilon gradients of a batch against the batch itself, on two systems:

  C1    testsystems.cluster_c1 (256 atoms, non-periodic), and
  w64   64 waters (192 atoms) periodic, cutoff 0.45 nm, a box per conformation (the default box
        scaled per axis by seeded factors in [0.98, 1.02], positions scaled along).

B distinct conformations (seeded jitter of the base positions, generated here) go through

  (a) forward:  one cf_compute_batch / cf_compute_batch_periodic (forces + energies), and
  (b) gradient: one cf_compute_batch_lj_vjp with both cotangents (seeded normal values),

on the same handle and the same device buffers.  After a warm-up of both arms the two are timed
alternately, `--repeats` times each (at least 5), a host clock around the call and the stream
synchronise that ends it.  Prints one JSON line: per system and B the per-conformation time of both
arms (median, min and max over the repeats) and their ratio.

Without cf_compute_batch_lj_vjp the only route to the same gradient is finite differences of the
forward batch, and L is not polynomial in sigma: the extrapolated central difference takes four
forward calls per parameter, 4 * 2 N of them.  That cost is stated as the measured forward time x 8 N
-- arithmetic on the forward arm's median, not a separate run.

  python tools/batch_lj_grad_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_lj_grad_probe.json]
  python tools/batch_lj_grad_probe.py --only 1024 --repeats 5      # one size (for a kernel trace)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "openmm-chargeflux_amd")]
from openmmcoul import HipCalcCoulForceKernel, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nconf", type=int, default=1024)
ap.add_argument("--only", type=int, default=0, help="time this batch size alone")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=ts.SEED)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("batch_lj_grad_probe needs a HIP device")

sizes = [args.only] if args.only else sorted({1, 64, args.nconf})
bmax = sizes[-1]
lib = _cabi.load_library()
flags = _cabi.CF_INCLUDE_FORCES | _cabi.CF_INCLUDE_ENERGY
dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
ptr = lambda t: C.c_void_p(t.data_ptr())


def spread(ts_, nb):
    us = [1e6 * t / nb for t in ts_]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


def probe(name):
    rng = np.random.default_rng(args.seed)
    if name == "C1":
        system, force, pos, _ = ts.cluster_c1()
        boxes = None
    else:
        system, force, pos, box = ts.water_box(64, cutoff=0.45)
    n = len(pos)
    confs = pos[None] + rng.normal(0.0, 0.003, size=(bmax, n, 3))
    if name != "C1":
        s = rng.uniform(0.98, 1.02, size=(bmax, 3))
        confs = confs * s[:, None, :]
        boxes = np.ascontiguousarray(box[None] * s[:, None, :])
    k = HipCalcCoulForceKernel(stream=torch.cuda.current_stream().cuda_stream).initialize(system, force)
    pt = dev(confs)
    frc = torch.zeros_like(pt)
    ene = torch.zeros(bmax, dtype=torch.float64, device="cuda")
    e_bar, f_bar = dev(rng.normal(size=bmax)), dev(rng.normal(size=(bmax, n, 3)))
    grad = torch.zeros((bmax, 2 * n), dtype=torch.float64, device="cuda")
    a_pos, a_frc, a_ene, a_eb, a_fb, a_grad = (ptr(t) for t in (pt, frc, ene, e_bar, f_bar, grad))
    a_box = boxes.ctypes.data_as(_cabi.DP) if boxes is not None else None
    h, sync = k._h, lib.cf_synchronize

    def forward(nb):
        t0 = time.perf_counter()
        if boxes is None:
            _cabi.check(lib.cf_compute_batch(h, nb, a_pos, flags, a_frc, a_ene, None), lib)
        else:
            _cabi.check(lib.cf_compute_batch_periodic(h, nb, a_pos, a_box, flags, a_frc, a_ene, None), lib)
        _cabi.check(sync(h), lib)
        return time.perf_counter() - t0

    def gradient(nb):
        t0 = time.perf_counter()
        _cabi.check(lib.cf_compute_batch_lj_vjp(h, nb, a_pos, a_box, a_eb, a_fb, a_grad), lib)
        _cabi.check(sync(h), lib)
        return time.perf_counter() - t0

    out = {"atoms": n, "lj_parameters": 2 * n, "periodic": boxes is not None, "sizes": {}}
    for nb in sizes:
        forward(nb), gradient(nb)        # warm-up of both arms at this size (the workspace grows here)
        torch.cuda.synchronize()
        tf, tg = [], []
        for _ in range(args.repeats):    # alternating
            tf.append(forward(nb))
            tg.append(gradient(nb))
        sf, sg = spread(tf, nb), spread(tg, nb)
        assert torch.isfinite(grad[:nb]).all() and grad[:nb].abs().max() > 0
        out["sizes"][str(nb)] = {
            "forward_us_per_conf": sf, "gradient_us_per_conf": sg,
            "ratio_gradient_over_forward": sg["median"] / sf["median"],
            "finite_difference_route_us_per_conf_forward_median_x_8N": sf["median"] * 8 * n,
            "finite_difference_route_over_gradient": sf["median"] * 8 * n / sg["median"],
        }
    out["batch_stats"] = k.batch_stats()
    k.destroy()
    return out


result = {"probe": "batch_lj_grad_probe", "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "cotangents": "energy and forces",
          "unit": "microseconds per conformation, wall time including the closing synchronise",
          "systems": {name: probe(name) for name in ("C1", "w64")}}
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
