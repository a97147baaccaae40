"""bench.py --dump-outputs (benchlib/dump.py): exact float64 encoding of the limbs, the fixed seeded sample of long vectors, the 64 MB budget
at the flagship size.  CPU only: device buffers are stood in for by host arrays."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import dump  # noqa: E402


class _Buf:
    """a device buffer of `count` field elements, or of zeros when no contents are given (sizes only)"""

    def __init__(self, count, data=None):
        self.count, self.data = count, data

    def download(self, shape, dtype=np.uint64, byte_offset=0):
        assert byte_offset % 32 == 0 and byte_offset // 32 + shape[0] <= self.count, (shape, byte_offset, self.count)
        if self.data is None:
            return np.zeros(shape, dtype=dtype)
        return self.data[byte_offset // 32:byte_offset // 32 + shape[0]].copy()


def _halves_to_u64(f):
    h = f.astype(np.uint64)
    return h[..., 0::2] | (h[..., 1::2] << np.uint64(32))


def test_limbs_are_written_exactly():
    a = np.random.default_rng(1).integers(0, 2 ** 64, size=(5, 4), dtype=np.uint64)
    a[0] = [0, 1, 2 ** 64 - 1, 2 ** 63]
    f = dump.limbs_as_float(a)
    assert f.dtype == np.float64 and f.shape == (5, 8)
    assert np.array_equal(_halves_to_u64(f), a)
    assert np.array_equal(dump.limbs_as_float(np.array([True, False])), [1.0, 0.0])


def test_proof_arrays_split_points_and_evaluations():
    rng = np.random.default_rng(2)
    pt = lambda: (rng.integers(0, 2 ** 64, size=8, dtype=np.uint64), False)
    ev = lambda: rng.integers(0, 2 ** 64, size=4, dtype=np.uint64)
    proof = {"wires_poly_comms": [pt() for _ in range(5)], "prod_perm_poly_comm": pt(), "wires_evals": [ev() for _ in range(5)],
             "perm_next_eval": ev(), "_debug": {"anything": 1}}
    out = dump.proof_arrays(proof)
    assert sorted(out) == ["perm_next_eval", "prod_perm_poly_comm_inf", "prod_perm_poly_comm_xy", "wires_evals", "wires_poly_comms_inf", "wires_poly_comms_xy"]
    assert out["wires_poly_comms_xy"].shape == (5, 16) and out["wires_poly_comms_inf"].shape == (5,)
    assert np.array_equal(_halves_to_u64(out["wires_poly_comms_xy"][3]), proof["wires_poly_comms"][3][0])
    assert out["perm_next_eval"].shape == (1, 8) and np.array_equal(_halves_to_u64(out["wires_evals"]), np.stack(proof["wires_evals"]))


def test_long_vectors_are_a_fixed_seeded_sample():
    small = dump.sample_index(1000)
    assert np.array_equal(small, np.arange(1000))
    n = 1 << 20
    idx = dump.sample_index(n)
    assert np.array_equal(idx, dump.sample_index(n))                       # the same sample in every run
    assert len(idx) == dump.SAMPLE_BLOCK * dump.SAMPLE_BLOCKS and np.all(np.diff(idx) > 0) and idx[-1] < n
    data = np.random.default_rng(3).integers(0, 2 ** 64, size=(n, 4), dtype=np.uint64)
    got = dump.device_vector(_Buf(n, data), n)
    assert np.array_equal(got["_index"], idx) and np.array_equal(_halves_to_u64(got[""]), data[idx])
    whole = dump.device_vector(_Buf(100, data[:100]), 100)
    assert set(whole) == {""} and np.array_equal(_halves_to_u64(whole[""]), data[:100])


@pytest.mark.parametrize("scheme,n_lanes", [("single", 1), ("reference2d", 2), ("classes", 2)])
def test_op_mix_dump_of_the_flagship_size_fits_the_budget(scheme, n_lanes):
    n = 1 << 24
    w = types.SimpleNamespace(g1_to_affine=lambda jac: (np.zeros(8, dtype=np.uint64), False))
    b = types.SimpleNamespace(w=w, scheme=scheme, n=n, m=8 * n, n_loc=n, m_loc=8 * n, nbig=26, n_lanes=n_lanes,
                              buf_n=[[_Buf(n), _Buf(n)] for _ in range(7)], buf_m=[[_Buf(8 * n), _Buf(8 * n)] for _ in range(n_lanes)],
                              cls={"bn": [[_Buf(n), _Buf(n)] for _ in range(7)], "quot": _Buf(8 * n)})
    arrays = dump.op_mix_arrays(b, np.zeros(12, dtype=np.uint64))
    assert {"commitment_xy", "commitment_inf", "intt_n_6", "intt_n_6_index", "coset_ifft_8n"} <= set(arrays)
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= dump.MAX_BYTES


def test_write_refuses_a_dump_over_budget(tmp_path, monkeypatch):
    arrays = {"a": np.zeros((4, 8)), "b": np.ones(3)}
    res = dump.write(str(tmp_path / "d"), arrays, "test")
    assert res["files"] == ["a.npy", "b.npy"] and res["bytes"] == 4 * 8 * 8 + 3 * 8
    assert np.array_equal(np.load(tmp_path / "d" / "b.npy"), np.ones(3))
    monkeypatch.setattr(dump, "MAX_BYTES", 100)
    with pytest.raises(ValueError):
        dump.write(str(tmp_path / "e"), arrays, "test")
    assert not (tmp_path / "e").exists()


def test_the_option_is_on_the_command_line(monkeypatch):
    from benchlib.cli import parse
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4", "--dump-outputs", "out_dir"])
    a = parse()
    assert a.dump_outputs == "out_dir" and a.steps == 4
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert parse().dump_outputs is None
