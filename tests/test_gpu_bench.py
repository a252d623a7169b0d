"""bench.py's command line at the smallest configuration (C2, 3 000 atoms), run in-process:

  plain run        the result line holds the headline fields and none of --full's; --steps sets
                   the number of timed steps (counted as force evaluations by the library)
  --dump-outputs   forces / energy / positions / velocities of the last timed step as float64
                   .npy; the forces and the energy are the CoulForce evaluation at the dumped
                   positions (oracle: forces <= 2.5e-6 kJ/mol/nm, the grid path's bar; energy
                   <= 1e-9 |E| + 1e-8, as smoke()); a second run with the same arguments starts
                   from the same inputs: positions <= 1e-12 nm, velocities <= 1e-9 nm/ps, forces
                   <= 1e-8 kJ/mol/nm apart (fp64 summation order of the atomics over a few steps of
                   MD: dv = dt dF / m <= 1e-3 * 1e-8 per step, dx = dt dv)
  --full           the secondary measurements are in the line, next to the same headline fields
"""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bench  # noqa: E402
from openmmcoul import testsystems as ts  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "kernels_ms_per_step", "ms_per_force_eval", "ms_per_harness_step", "graph_replay_ms_per_step",
             "exact_kspace", "host_boundary", "openmm_gpu_buffers", "cpu_baseline")
STEPS, WARMUP = 3, 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _run(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--config", "C2", "--steps", str(STEPS),
                                      "--warmup", str(WARMUP), *extra])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1, "one JSON result line on stdout"
    return json.loads(lines[0])


def test_plain_run_and_dump(monkeypatch, capsys, tmp_path):
    from oracle import Oracle

    a, b = tmp_path / "a", tmp_path / "b"
    line = _run(monkeypatch, capsys, "--dump-outputs", str(a))
    for k in HEADLINE:
        assert k in line, k
    for k in FULL_ONLY:
        assert k not in line, k
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["unit"] == "ns/day" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(86.4 / line["ms_per_step"], rel=1e-3)
    # the timed region is exactly --steps force evaluations
    assert int(line["config"]["nlist_builds_in_timed_steps"].split("/")[1]) == STEPS

    system, force, pos0, box = ts.make("C2")
    n = len(pos0)
    out = {k: np.load(a / f"{k}.npy") for k in ("forces", "energy", "positions", "velocities")}
    assert all(v.dtype == np.float64 for v in out.values())
    assert out["forces"].shape == out["positions"].shape == out["velocities"].shape == (n, 3)
    assert out["energy"].shape == (1,) and out["energy"][0] == line["energy_kj_mol"]
    assert sum(v.nbytes for v in out.values()) <= 64e6
    assert np.abs(out["positions"] - pos0).max() > 0, "the dumped state is after the timed steps"

    ref = Oracle(force, box).execute(out["positions"], box)
    assert np.abs(out["forces"] - ref["forces"]).max() <= 2.5e-6
    assert abs(out["energy"][0] - ref["energy"]) <= 1e-9 * abs(ref["energy"]) + 1e-8

    _run(monkeypatch, capsys, "--dump-outputs", str(b))
    assert np.abs(np.load(b / "positions.npy") - out["positions"]).max() <= 1e-12
    assert np.abs(np.load(b / "velocities.npy") - out["velocities"]).max() <= 1e-9
    assert np.abs(np.load(b / "forces.npy") - out["forces"]).max() <= 1e-8


def test_full_run(monkeypatch, capsys):
    line = _run(monkeypatch, capsys, "--full")
    for k in HEADLINE + FULL_ONLY:
        assert k in line, k
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    assert line["roofline"] is not None and line["cpu_baseline"]["ms_per_force_eval"] > 0
    assert line["exact_kspace"]["max_abs_dforce_grid_vs_exact"] <= 2.5e-6
