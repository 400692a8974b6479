"""The plans and resident loops the library makes for the cases of tests/golden/plan_shapes.json
(plan_shape_cases.py: the workloads at 8 .. 2048 walkers per half-step, the S and T models of
test_gpu_shapes.py) against the record: nh_half_step_info / _split / _syn_form of every plan the
device loop creates and the whole of resident_info -- the launch's grid and the
two-walkers-in-flight instance included, which follow from the runtime's occupancy answer and are
out of test_plan_shape_host.py's reach -- or the recorded refusal.  The sizes the descriptor
carried are compared too: were they to drift, the host test would be replaying another model."""
import pytest

import plan_shape_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def na():
    import naima_amd
    from naima_amd import _lib
    _lib.get_context()
    return naima_amd


@pytest.mark.parametrize("cid", PC.case_ids())
def test_shapes_are_the_recorded_ones(na, monkeypatch, cid):
    from naima_amd import _lib
    want = PC.load_golden()[cid]
    ncu = _lib.get_context().info()["compute_units"]
    if ncu != want["ncu"]:
        pytest.skip("the shapes were recorded on a device of %d CUs; this one has %d"
                    % (want["ncu"], ncu))
    got = PC.run_case(na, monkeypatch, cid)
    assert [p["out"] for p in got["plans"]] == [p["out"] for p in want["plans"]]
    assert got["resident"] == want["resident"]
    assert got.get("resident_reason") == want.get("resident_reason")
    assert [p["in"] for p in got["plans"]] == [p["in"] for p in want["plans"]]
