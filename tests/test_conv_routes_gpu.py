"""Every route of the conv host ops (vaehip/ops.py: conv_fwd, conv_dgrad, conv_wgrad, the upsampler helpers, _wgrad_wino,
_reduce_splits) against a float64 CPU convolution of the operands as the serving kernel reads them.

The kernels have their own tests; this module holds what the host layer composes from them: which kernel family runs, whether
GroupNorm(+SiLU) is fused or materialised first (once), how each operand, the residual and the result are stored, whether a
launch is redone on fp32 copies, whether the upsampler's gradient is pooled, how splits are reduced, and which attributes the
result carries.  tests/conv_routes.py has the table (one case per arm, with the route it must take) and the reference;
tests/test_conv_routes_host.py holds every case's route without a GPU.

Bars are the project's own (conv_routes.BAR_*): fp32 direct / flat and bf16 arithmetic on exactly rounded operands 2e-5
(weight gradient 3e-5, 5e-5 behind a fused GroupNorm), F(2x2) Winograd 1e-5, F(4x4) 4e-5, all relative to the reference's
max; a bf16-stored result per element, |got - ref| <= 2^-7 |ref| + 1e-6 with no element over; epilogue sums against a
separate pass over the returned tensor at 1e-5.

The last test asserts that every statement of those functions ran inside a case whose value was compared (sys.settrace on
their code objects; a refused call does not count): run the module whole.  VAEHIP_ROUTES_MEASURED=<file> writes every case's figures next to their bars
(profiles/conv_routes_measured.json)."""
import json
import os

import pytest

import conv_routes as cr

pytestmark = pytest.mark.gpu

SEEN = set()     # (function, line) pairs executed inside the cases whose value was compared (test_every_statement_ran_in_a_case)
MEASURED = {}    # case id -> {figure: [measured, bar]}


def _codes():
    from vaehip import ops
    return cr.traced_codes(ops)


@pytest.mark.parametrize("case", cr.CASES, ids=[c.id for c in cr.CASES])
def test_route_and_value(cuda, case):
    from vaehip.lib import VaeHipError
    codes = _codes()
    if case.raises:  # refused by the library's launch check: nothing runs, no value to compare, and its lines do not count
        with pytest.raises(VaeHipError):
            cr.run(case)
        return
    lines = set()
    with cr.LineTracer(codes, lines):
        r = cr.run(case)
    cr.check_route(case, r)
    fig = cr.check_value(case, r)
    SEEN.update(lines)  # (only now: the statements ran inside a call whose value was compared)
    MEASURED[case.id] = {"kernels": r["route"].names, **{k: [m, b] for k, (m, b) in fig.items()}}
    print(case.id, r["route"].names, {k: f"{m:.3g} (bar {b:g})" for k, (m, b) in fig.items()})
    over = {k: v for k, v in fig.items() if not v[0] <= v[1]}
    assert not over, (case.id, case.why, over)


def test_every_statement_ran_in_a_case(cuda):
    """every statement of the conv host ops (docstrings and `raise` lines aside) executed inside a case above, except the at
    most 5 of conv_routes.ALLOWED"""
    from vaehip import ops
    out = os.environ.get("VAEHIP_ROUTES_MEASURED")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)
    assert len(MEASURED) == sum(not c.raises for c in cr.CASES), "run the whole module: the cases above collect the executed lines"
    assert len(cr.ALLOWED) <= 5
    never = cr.missed([getattr(ops, n) for n in cr.TRACED], SEEN)
    assert set(never) <= set(cr.ALLOWED), never
