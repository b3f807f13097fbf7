"""CPU: the cases of tests/test_gpu_shoot_adjoint.py (tests/shoot_adjoint_case.py) against the
float64 oracle, with the kernels replaced by the oracle-backed float64 spec (tests/fake_hip.py).

- ShootFn's host logic: every case, every cotangent pattern, gradients in q0, p0, x0 and again in
  p0 alone, at 1e-12 (the float64 anchor; measured 2e-15).  The support and the carried points are
  cut to HOST_M / HOST_N rows here (the fake kernels are dense float64 autograd); the graph and
  cutoff routes need a device, so on the CPU their cases run ShootFn's fused route.
- The two conditions that keep the device test from being hollow, at the device test's own shapes
  and from the oracle alone (shoot_adjoint_case.conditions): every slot bites, and the float32
  oracle's error is far from being the tolerance.
"""
import pytest
import torch

import fake_hip
import shoot_adjoint_case as S

HOST_M, HOST_N = 160, 200
CASES = S.gpu_cases()
HOST_CASES = list(dict.fromkeys(c._replace(M=min(c.M, HOST_M), N=min(c.N, HOST_N)) for c in CASES))


def _id(c):
    return f"{c.scheme}-{c.version}-{c.cloud}-M{c.M}-D{c.D}-N{c.N}-nt{c.nt}-s{c.seed}-{len(c.patterns)}p"


@pytest.fixture
def fake(monkeypatch):
    fake_hip.install(monkeypatch)


@pytest.mark.parametrize("c", HOST_CASES, ids=_id)
def test_host_adjoint_matches_float64(fake, c):
    ref = S.reference(c)
    for pattern in c.patterns:
        for p0_only in (False, True):
            out = S.run_library(ref, pattern, "cpu", dtype=torch.float64, p0_only=p0_only)
            S.check(out, ref, pattern, p0_only, grad_tol=1e-12, traj_tol=1e-12, label="host")


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_device_case_conditions(c):
    """At the device test's shape: a dropped slot moves a compared gradient by >= 100 x its
    tolerance, the slots that reach no input are exactly the model's dead ones, and 4 x the
    float32 oracle's error is <= 1e-3."""
    m = S.conditions(S.reference(c))
    print(_id(c), m)
    assert m["bite"] >= S.BITE and m["oracle32"] <= S.ORACLE32_MAX
