"""Cost of the dipoles and atomic polar tensors of a batch, on C1 (testsystems.cluster_c1, 256 atoms,
non-periodic, P = 608 parameters): B distinct conformations (seeded jitter of the C1 positions,
generated here) through

  (a) forward:  one cf_compute_batch_dipole (dipoles, polar tensors and charges),
  (b) gradient: one cf_compute_batch_dipole_vjp with both cotangents (seeded normal values), and
  (c) charges:  one cf_compute_batch with flags 0 and the charges output -- the flux and charge
                stages alone, which (a) runs before its own kernel,

on the same handle and the same device buffers.  After a warm-up of the three arms they are timed in
turn, `--repeats` times each (at least 5), a host clock around the call and the stream synchronise
that ends it.  Prints one JSON line: the per-conformation time of each arm (median, min and max over
the repeats).

  python tools/batch_dipole_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_dipole_probe.json]
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
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=ts.SEED)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("batch_dipole_probe needs a HIP device")

system, force, pos, _ = ts.cluster_c1()
n, nb = len(pos), args.nconf
rng = np.random.default_rng(args.seed)
confs = pos[None] + rng.normal(0.0, 0.003, size=(nb, n, 3))

stream = torch.cuda.current_stream().cuda_stream
k = HipCalcCoulForceKernel(stream=stream).initialize(system, force)
lib = _cabi.load_library()
nparam = sum(k.param_counts())
dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
pt = dev(confs)
mu, apt, chg, grad = zeros(nb, 3), zeros(nb, n, 3, 3), zeros(nb, n), zeros(nb, nparam)
mu_bar, apt_bar = dev(rng.normal(size=(nb, 3))), dev(rng.normal(size=(nb, n, 3, 3)))
ptr = lambda t: C.c_void_p(t.data_ptr())
a_pos, a_mu, a_apt, a_chg, a_grad, a_mb, a_pb = (ptr(t) for t in (pt, mu, apt, chg, grad, mu_bar, apt_bar))
h, sync = k._h, lib.cf_synchronize


def timed(call):
    t0 = time.perf_counter()
    _cabi.check(call(), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


arms = {
    "forward": lambda: lib.cf_compute_batch_dipole(h, nb, a_pos, a_mu, a_apt, a_chg),
    "gradient": lambda: lib.cf_compute_batch_dipole_vjp(h, nb, a_pos, a_mb, a_pb, a_grad),
    "charges": lambda: lib.cf_compute_batch(h, nb, a_pos, 0, None, None, a_chg),
}


def spread(ts_):
    us = [1e6 * t / nb for t in ts_]
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


for call in arms.values():       # warm-up of every arm (the workspace grows here)
    timed(call)
torch.cuda.synchronize()
times = {name: [] for name in arms}
for _ in range(args.repeats):    # in turn
    for name, call in arms.items():
        times[name].append(timed(call))
assert torch.isfinite(mu).all() and torch.isfinite(apt).all() and torch.isfinite(grad).all()
result = {"probe": "batch_dipole_probe", "system": "C1", "atoms": n, "parameters": nparam, "nconf": nb,
          "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "unit": "microseconds per conformation, wall time including the closing synchronise",
          "forward_us_per_conf": spread(times["forward"]), "gradient_us_per_conf": spread(times["gradient"]),
          "charges_us_per_conf": spread(times["charges"]), "batch_stats": k.batch_stats()}
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
k.destroy()
