"""The mixture-prior kernels (csrc/kernels/gmm.hip) against the float64 oracle (models/gmm.py, on the CPU): one EM
iteration per shape, every output per element, within the rule of tests/gmm_cases.py; the status word; a dead
component."""
import pytest
import torch

from tests import gmm_cases as gc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# Factors above 8 that an output needed, with their cause (docs/KERNELS.md "Mixture prior"): none.


def _C():
    from multidisttorch_amd.ops import native

    return native.require()


def _em_step(z, pi, mu, cov, reg=None):
    (n, Z), K = z.shape, pi.numel()
    C = _C()
    new = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)  # nothing unwritten may be read
    ws = new(C.gmm_ws_numel(n, Z, K))
    out = dict(r=new(n, K), ll=new(n), pi=new(K), mu=new(K, Z), cov=new(K, Z, Z))
    C.gmm_em_step(z.to(DEV), pi.to(DEV), mu.to(DEV), cov.to(DEV), ws, *out.values(), **({} if reg is None else dict(reg=reg)))
    out.update(W=C.gmm_ws_view(ws, n, Z, K, "W"), c=C.gmm_ws_view(ws, n, Z, K, "c"))
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.IDS)
def test_em_step_matches_the_oracle_per_element(shape, native_ext):
    z, p32, ref64, ref32 = gc.step_case(shape)
    got = _em_step(z, *p32)
    bad = []
    for k, ref in ref64.items():
        err, tol = float((got[k].double() - ref).abs().max()), gc.tolerance(ref, ref32[k])
        print(f"{shape} {k}: max error {err:.3e}, tolerance {tol:.3e}, error / float32 oracle's deviation "
              f"{err / max(float((ref32[k].double() - ref).abs().max()), 1e-300):.2f}")
        if got[k].shape != ref.shape or not err <= tol:
            bad.append(k)
    assert not bad


def test_indefinite_covariance_raises_from_the_status_word(native_ext):
    z, (pi, mu, cov), _, _ = gc.step_case((37, 5, 3))
    cov = cov.clone()
    cov[1] -= 2.0 * float(torch.linalg.eigvalsh(cov[1].double())[-2]) * torch.eye(5)  # two negative eigenvalues
    with pytest.raises(ValueError, match="component 1 is not positive definite"):
        _em_step(z, pi, mu, cov, reg=0.0)
    _em_step(z, pi, mu, gc.step_case((37, 5, 3))[1][2], reg=0.0)  # the parameters it was derived from are good


def test_dead_component_keeps_its_parameters(native_ext):
    z, (pi, mu, cov), _, _ = gc.step_case((130, 20, 10))
    mu = mu.clone()
    mu[4] += 1e3
    got, ref = _em_step(z, pi, mu, cov), gc.em_step(z.double(), pi.double(), mu.double(), cov.double())
    assert float(got["pi"][4]) == 0.0 and torch.equal(got["mu"][4], mu[4]) and torch.equal(got["cov"][4], cov[4])
    assert torch.allclose(got["pi"].double(), ref["pi"], rtol=0, atol=1e-6) and float(ref["pi"][4]) == 0.0
