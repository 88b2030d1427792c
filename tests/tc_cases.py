"""Shared inputs, oracle and bounds of the total-correlation penalty tests
(tests/unit/test_tc_penalty.py, tests/gpu/test_tc_penalty_gpu.py).

The value is defined by models/latent.py (``tc_batch = M * latent_report(...)
["tc"]`` on the batch rows with ``n = M``) and the gradient by autograd through
``latent_report(..., return_rows=True)``, both in float64 on the float32 rows
and noise.

The bound follows tests/latent_cases.py: per quantity, ``MARGIN`` = 16 times the
error of the same oracle run in float32 against the float64 one on the same
input, floored by one float32 rounding of the largest value that enters the
quantity. It never comes from the code under test.

* gradient: the largest gradient element.
* ``tc_batch``: the largest per-row log-density (``row_scale``, as
  tests/latent_cases.py floors the report's row means) or the value itself.
"""
import torch

from multidisttorch_amd.models import tc
from tests import latent_cases as lc

MARGIN = lc.MARGIN
U32 = lc.U32

# (name, rows) of the kernel-level inputs
KERNEL_CASES = (
    ("overlap_40_4", lambda: lc.overlap(40, 4)),
    ("mixed_37_12", lambda: lc.mixed(37, 12)),
    ("mixed_65_20", lambda: lc.mixed(65, 20)),
    ("mixed_128_32", lambda: lc.mixed(128, 32)),
    ("mixed_200_64", lambda: lc.mixed(200, 64)),
    ("mixed_37_10", lambda: lc.mixed(37, 10)),   # Z no multiple of 4: the kernels' padded dimensions
    ("sharp_37_12", lambda: lc.sharp(37, 12)),
    ("sharp_64_64", lambda: lc.sharp(64, 64)),
    ("mixed_65_20_mu100", lambda: _shift_mu(lc.mixed(65, 20), 100.0)),
    ("one_row", lambda: lc.mixed(1, 12)),
)


def _shift_mu(mulv, by):
    Z = mulv.shape[1] // 2
    out = mulv.clone()
    out[:, :Z] += by
    return out


def noise(M, Z, seed=11):
    return torch.randn(M, Z, generator=torch.Generator().manual_seed(seed))


def oracle(mulv, eps, dtype=torch.float64):
    """(tc_batch, d tc_batch / d[mu | lv] as [M, 2Z]) by autograd through
    models/latent.py in ``dtype``, from float32 rows and noise."""
    Z = mulv.shape[1] // 2
    m = mulv.detach().cpu().to(dtype)
    mu, lv = m[:, :Z].clone().requires_grad_(), m[:, Z:].clone().requires_grad_()
    v = tc.tc_batch(mu, lv, eps.detach().cpu().to(dtype))
    v.backward()
    return float(v), torch.cat([mu.grad, lv.grad], 1).double()


def bounds(mulv, eps):
    """(value64, grad64, value bound, gradient bound)."""
    v64, g64 = oracle(mulv, eps)
    v32, g32 = oracle(mulv, eps, torch.float32)
    rows = lc.oracle(mulv, eps)
    row_scale = max(float(rows[k].abs().max()) for k in ("lq_joint", "lq_marg"))
    bv = MARGIN * max(abs(v32 - v64), U32 * max(row_scale, abs(v64)))
    bg = MARGIN * max(float((g32 - g64).abs().max()), U32 * float(g64.abs().max()))
    return v64, g64, bv, bg
