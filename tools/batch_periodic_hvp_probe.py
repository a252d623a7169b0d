"""Cost of the Hessian-vector products of a periodic batch, on 64 waters (testsystems.water_box(64),
192 atoms, cutoff 0.55 nm): B boxes (seeded jitter and per-axis box scaling in [0.95, 1.05], generated
here) through

  (a) hvp_k1:   one cf_compute_batch_periodic_hvp with K = 1 direction per conformation,
  (b) hvp_k8:   one cf_compute_batch_periodic_hvp with K = 8 directions per conformation, and
  (c) forward:  one cf_compute_batch_periodic with both flags -- two of these per direction is what
                central differences of the forces would cost,

on the same handle and the same device buffers (seeded N(0, 1) directions), and then

  (d) hvp_k8_kd1: arm (b) in a child process on a build of the library with ONE direction per chunk
                (-DCF_BPH_KD=1; built beside the product on first use: `--kd1-lib`), so that the gain
                from carrying 4 directions per block is a measured number.

After a warm-up of its arms a process times them in turn, `--repeats` times each (at least 5), a
host clock around the call and the stream synchronise that ends it.  Prints one JSON line: the time
per (conformation, direction) of each arm (median, min and max over the repeats; the forward arm per
conformation), the ratio of each product arm's median to two forward batches and hvp_k8_kd1 over hvp_k8.

  python tools/batch_periodic_hvp_probe.py [--nconf 1024] [--repeats 7] [--out profiles/batch_periodic_hvp_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openmm-chargeflux_amd")
sys.path[:0] = [PKG]
from openmmcoul import HipCalcCoulForceKernel, _cabi  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nconf", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=ts.SEED)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
ap.add_argument("--kd1-lib", default=os.path.join(PKG, "libchargeflux_hip_kd1.so"),
                help="the library built with -DCF_BPH_KD=1 (built there if absent)")
ap.add_argument("--child", action="store_true", help="(internal) time hvp_k8 alone on --kd1-lib")
args = ap.parse_args()
if args.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("batch_periodic_hvp_probe needs a HIP device")
if args.child:
    _cabi._lib = _cabi.load_library(args.kd1_lib)
KS = (8,) if args.child else (1, 8)

system, force, pos, box = ts.water_box(64, cutoff=0.55)
n, nb = len(pos), args.nconf
rng = np.random.default_rng(args.seed)
scale = rng.uniform(0.95, 1.05, size=(nb, 3))
confs = (pos[None] + rng.normal(0.0, 0.003, size=(nb, n, 3))) * scale[:, None, :]
boxes = np.ascontiguousarray(box[None] * scale[:, None, :])

stream = torch.cuda.current_stream().cuda_stream
k = HipCalcCoulForceKernel(stream=stream).initialize(system, force)
lib = _cabi.load_library()
dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
ptr = lambda t: C.c_void_p(t.data_ptr())
bp = boxes.ctypes.data_as(C.POINTER(C.c_double))
pt = dev(confs)
vecs = {kk: dev(np.random.default_rng(args.seed + kk).normal(size=(nb, kk, n, 3))) for kk in KS}
outs = {kk: zeros(nb, kk, n, 3) for kk in KS}
frc, ene, chg = zeros(nb, n, 3), zeros(nb), zeros(nb, n)
h, sync = k._h, lib.cf_synchronize
flags = _cabi.CF_INCLUDE_FORCES | _cabi.CF_INCLUDE_ENERGY


def timed(call):
    t0 = time.perf_counter()
    _cabi.check(call(), lib)
    _cabi.check(sync(h), lib)
    return time.perf_counter() - t0


arms = {f"hvp_k{kk}": (lambda kk=kk: lib.cf_compute_batch_periodic_hvp(h, nb, ptr(pt), bp, kk, ptr(vecs[kk]),
                                                                         ptr(outs[kk]))) for kk in KS}
rows = {f"hvp_k{kk}": nb * kk for kk in KS}
if not args.child:
    arms["forward"] = lambda: lib.cf_compute_batch_periodic(h, nb, ptr(pt), bp, flags, ptr(frc), ptr(ene), ptr(chg))
    rows["forward"] = nb

for call in arms.values():       # warm-up of every arm (the workspaces grow here)
    timed(call)
torch.cuda.synchronize()
stats0 = k.batch_stats()
times = {name: [] for name in arms}
for _ in range(args.repeats):    # in turn
    for name, call in arms.items():
        times[name].append(timed(call))
stats1 = k.batch_stats()
assert all(torch.isfinite(o).all() for o in outs.values()) and torch.isfinite(frc).all()
result = {}
for name in arms:
    us = [1e6 * t / rows[name] for t in times[name]]
    result[name + "_us"] = {"median": statistics.median(us), "min": min(us), "max": max(us)}
result["passes_per_timed_round"] = (stats1[2] - stats0[2]) / args.repeats
kmax = list(k.ewald_params()[1])
k.destroy()
if args.child:
    print(json.dumps(result))
    sys.exit(0)

result = {"probe": "batch_periodic_hvp_probe", "system": "64 waters, cutoff 0.55 nm", "atoms": n, "nconf": nb,
          "kmax": kmax, "repeats": args.repeats,
          "device": torch.cuda.get_device_name(0),
          "unit": "microseconds per (conformation, direction) -- forward: per conformation -- wall time "
                  "including the closing synchronise", **result}
for kk in KS:
    result[f"hvp_k{kk}_over_two_forward"] = result[f"hvp_k{kk}_us"]["median"] / (2 * result["forward_us"]["median"])
# the same K = 8 arm with one direction per chunk: a fresh process on the variant library
if not os.path.exists(args.kd1_lib):
    subprocess.run(["make", "-s", "-j", "16", "-C", os.path.join(PKG, "csrc"), "OUT=" + os.path.abspath(args.kd1_lib),
                    "BUILD=" + os.path.join(PKG, "csrc", "build", "kd1"), "EXTRA_HIPFLAGS=-DCF_BPH_KD=1",
                    os.path.abspath(args.kd1_lib)], check=True)
child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--nconf", str(nb), "--repeats",
                        str(args.repeats), "--seed", str(args.seed), "--kd1-lib", args.kd1_lib],
                       check=True, capture_output=True, text=True, timeout=600)
kd1 = json.loads(child.stdout.strip().splitlines()[-1])
result["hvp_k8_kd1_us"] = kd1["hvp_k8_us"]
result["hvp_k8_kd1_over_hvp_k8"] = kd1["hvp_k8_us"]["median"] / result["hvp_k8_us"]["median"]
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
