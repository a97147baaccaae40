"""Who frees the device buffers of distributed_plonk_amd/kzg.py: every function is call-scoped (DeviceScope), so a clean run leaves no live
buffer, and with the i-th allocation, the j-th upload or any `*_dev` call failed the injected exception comes out and nothing stays
allocated.  The tracker, the injection loop and the fixture are those of tests/test_gpu_buffer_ownership.py, imported as they are."""
import numpy as np
import pytest

from distributed_plonk_amd import kzg
from distributed_plonk_amd import verifier as VF
from tests import kzg_ref as R
from tests.kzg_ref import CURVES
from tests.test_gpu_buffer_ownership import exercise, trackers  # noqa: F401 - `trackers` is the fixture

pytestmark = pytest.mark.gpu

N = 9                                                     # coefficients; the key has N points
_STATE = {}


def _prepare(w, curve, oracle, scratch):
    """The trapdoor key resident on the tracked worker (its buffer is the caller's, unobserved), a polynomial, three points, and — made once,
    by the reference — a commitment with three honest openings."""
    cid = dict(CURVES)[curve]
    d_srs = scratch(np.zeros((N, 2 * w.q64), np.uint64))
    w.synth_srs(R.to_limbs(curve, R.TAU), N, d_srs)
    w.init_dev(d_srs, N, 0, 0)
    if curve not in _STATE:
        coeffs = list(range(3, 3 + N))
        zs = [0, 5, R.FR[curve] - 1]
        comm = R.commitment(curve, cid, coeffs)
        ops = [kzg.Opening(R.to_limbs(curve, z), R.to_limbs(curve, R.horner(curve, coeffs, z)), R.xy_of(R.proof(curve, cid, coeffs, z))) for z in zs]
        _STATE[curve] = dict(coeffs=coeffs, limbs=R.vec_to_limbs(curve, coeffs), zs=zs, pts=R.vec_to_limbs(curve, zs), comm=comm, ops=ops,
                             key=VF.OpenKey.from_trapdoor(curve, R.TAU))
    return dict(_STATE[curve], curve=curve)


def _evaluate(w, st, own):
    got = kzg.evaluate(w, st["limbs"], st["pts"])
    assert np.array_equal(got, R.vec_to_limbs(st["curve"], [R.horner(st["curve"], st["coeffs"], z) for z in st["zs"]]))


def _open_many_two_chunks(w, st, own):
    calls = []
    real = w.poly_open_many_dev
    w.poly_open_many_dev = lambda *a: calls.append(a) or real(*a)
    try:
        ops = kzg.open_many(w, st["limbs"], st["pts"], max_scratch_bytes=2 * (N - 1) * 32)
    finally:
        w.poly_open_many_dev = real
    assert len(calls) == 2 and [c[3] for c in calls] == [2, 1]
    assert all(np.array_equal(a.value, b.value) and np.array_equal(a.proof_xy, b.proof_xy) for a, b in zip(ops, st["ops"]))


def _batch_verify(w, st, own):
    assert kzg.batch_verify(w, st["key"], [st["comm"]] * 3, st["ops"], seed=1) == [True] * 3


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("name,run", [("evaluate", _evaluate), ("open_many", _open_many_two_chunks), ("batch_verify", _batch_verify)])
def test_kzg_functions_leave_no_buffer_behind(trackers, oracle, curve, cid, name, run):  # noqa: F811
    exercise(trackers(curve), _prepare, run, oracle, curve)
