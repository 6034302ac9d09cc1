"""Every route's window tap layout on the device, with a rough, asymmetric window (tests/window_cases.py).

The designed window is smooth and symmetric up to a shift of one sample: an index slip in a tap layout -- a neighbour's taps, a
reversed tap order, the whole window reversed -- stays under the parity bounds with it.  With independent standard-normal taps
every such slip moves the result by at least ten ceilings (tests/test_window_taps_host.py shows that in the float64 oracle, for
every case and mutation), while a correct float32 pipeline stays a factor of 35 under them.  A caller-supplied ``window=`` is a
documented feature of ``FxPlan``: this is a product path.

Each case names a route, asserts it from ``plan.path`` / ``plan.info``, and compares with the float64 oracle under the same float64
window: every chunk's SPECTRUM row of baseline (0, 1), all baselines of chunk 0 with 3 and more antennas, ``fx_accumulate`` +
``finalize`` against the float64 mean of the rows; every spectrum for ``channelize``."""
import numpy as np
import pytest

import window_cases as wc
from tolerances import TOL_SPEC, TOL_SPEC_ANY, TOL_VIS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan_mod(torch):
    from effex_amd import plan
    return plan


def assert_route(case, p):
    seen = dict(p.info, path=p.path)
    assert {k: seen[k] for k in case.expect} == case.expect, (case.id, seen)


@pytest.mark.parametrize("case", wc.CASES, ids=[c.id for c in wc.CASES])
def test_window_taps(plan_mod, torch, monkeypatch, case):
    for name, value in case.env.items():      # (read when the plan is made; all but FXC_RTC exist in the developer library only)
        monkeypatch.setenv(name, value)
    window = wc.rough_window(case.ntaps, case.nchan)
    x, u8 = wc.make_input(case)
    ref = wc.oracle(case, x, window)
    xd = torch.from_numpy(x if u8 is None else u8).cuda()
    with plan_mod.FxPlan(case.n_ant, case.nchan, case.ntaps, wc.num_samp(case), window=window, path=case.path, dev=case.dev) as p:
        if case.entry == "channelize":
            spec = p.channelize(xd.reshape(-1, xd.shape[-1])).cpu().numpy()
            assert_route(case, p)
            assert spec.shape == ref.shape
            bound = TOL_SPEC_ANY if case.nchan & (case.nchan - 1) else TOL_SPEC
            for label, err in wc.checks(case, spec, ref):
                print("%s: %s: %.3g" % (case.id, label, err))
                assert err < bound, (case.id, label)
            return
        rows = (p.fx_rows_u8(xd, "SPECTRUM") if u8 is not None else p.fx_rows(xd, "SPECTRUM")).cpu().numpy()
        assert_route(case, p)
        assert rows.shape == ref.shape
        for label, err in wc.checks(case, rows, ref):
            print("%s: %s: %.3g" % (case.id, label, err))
            assert err < TOL_VIS, (case.id, label)
        if u8 is not None:
            p.fx_accumulate_u8(xd)
        else:
            p.fx_accumulate(xd)
        integ = p.finalize("SPECTRUM")
        err = wc.rel_err(integ, rows.astype(np.complex128).mean(axis=0))
        print("%s: integration against the mean of the rows: %.3g" % (case.id, err))
        assert err < 2e-6, case.id
