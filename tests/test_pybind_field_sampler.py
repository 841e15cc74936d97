"""The compiled pybind11 module `field_sampler` of meshfem_amd/pybind (the reference's extension-module name, class name, method names,
argument names and defaults), checked in an interpreter of its own (tests/pybind_field_sampler_checks.py) like the other compiled modules:
host part = import, signatures, defaults; device part = both constructors and every method against the numpy restatement
(tests/field_sampler_util.py)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _run(what):
    r = subprocess.run([sys.executable, os.path.join(HERE, "pybind_field_sampler_checks.py"), what], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_module_imports_with_the_reference_signatures():
    _run("cpu")


@pytest.mark.gpu
def test_sampler_matches_the_restatement_on_the_device():
    _run("gpu")
