"""The exposure / attainment call of the C++ host facade (include/pharmsol_hip.hpp, Resident::exposure_attainment): a
compiled program (tests/cpp/exposure_facade_test.cpp) prints one PTA and one mean per profile, and the same design run
through the Python path - predict, exposure, target_attainment on the device - gives the same bits."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "exposure_facade_test")


def test_cpp_exposure_facade_compiles():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/cpp/exposure_facade_test"], check=True)
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_exposure_facade_gives_the_python_path_s_bits():
    import torch

    from pharmsol_amd import Data, Subject, runtime
    from tests import models

    subprocess.run(["make", "-C", ROOT, "-s", "tests/cpp/exposure_facade_test"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True)
    assert r.returncode == 0 and "exposure facade: ok" in r.stdout, r.stdout + r.stderr
    got = [(float.fromhex(line.split()[3]), float.fromhex(line.split()[5])) for line in r.stdout.splitlines() if line.startswith("profile")]
    m = models.handwritten_analytical("two_compartments", 0, 4).with_ndrugs(1)
    subs = []
    for s in range(5):
        b = Subject.builder(str(s)).infusion(0.0, 500.0 + 25.0 * s, 0, 0.5)
        for t in (0.5, 1.0, 2.0, 4.0, 8.0, 12.0, 24.0):
            b = b.observation(t, 0.0, 0)
        subs.append(b.build())
    P = 8
    p = np.arange(P, dtype=np.float64)
    theta = np.stack([0.05 + 0.03125 * p, 0.125 + 0.015625 * p, 0.0625 + 0.0078125 * p, 20.0 + 2.0 * p], axis=1)
    pop = runtime.DevicePopulation(m.flatten(Data(subs)), 0)
    pred, _ = runtime.predict(m, pop, theta)
    auc = runtime.exposure(pop, pred, metrics=("auc",))["auc"]
    pta, mean = runtime.target_attainment(pop, auc, np.full(P, 0.125), np.full(5, 60.0), mean=True)
    torch.cuda.synchronize()
    assert len(got) == 5
    assert [g[0] for g in got] == pta.cpu().tolist() and [g[1] for g in got] == mean.cpu().tolist()
    assert 0.0 < min(g[0] for g in got) and max(g[0] for g in got) < 1.0 or len({g[0] for g in got}) > 1
