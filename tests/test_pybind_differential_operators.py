"""The compiled pybind11 module `differential_operators` of meshfem_amd/pybind (the reference's extension-module name, function names,
argument names and defaults), checked in an interpreter of its own (tests/pybind_differential_operators_checks.py) like the other compiled
modules: host part = import, signatures, no `bilaplacian`; device part = laplacian / mass / mass_elasticity with forceP1 and upperTriOnly in
both settings, lumped, gradient and divergence against the oracle."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _run(what):
    r = subprocess.run([sys.executable, os.path.join(HERE, "pybind_differential_operators_checks.py"), what], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_module_imports_with_the_reference_signatures():
    _run("cpu")


@pytest.mark.gpu
def test_operators_match_oracle_on_the_device():
    _run("gpu")
