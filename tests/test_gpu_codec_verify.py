"""Verifying what a prover sends: four proofs of a 2^10-gate instance serialized with transcript.serialize_proof, their public inputs as 32-byte
scalars, and the open key as bytes, through verifier.batch_verify_bytes — decoded on the device (plonk_proofs_from_bytes_dev) and handed to
plonk_verify_batch_dev as device records, the output pairs folded into the device's sum tree masked by status and decode words.  All four
accepted with one pairing check; a flipped sign bit is the verifier's rejection (decode status 0), an x without a point the codec's (decode
status 1); neither disturbs the other proofs, and the pairing checks are those verifier.bisect_tree counts for the same leaves, in a batch of
four and in one of three with a padded leaf; the verdicts are those of batch_verify on the dicts proof_from_bytes returns."""
import pytest

from distributed_plonk_amd import codec as CD
from distributed_plonk_amd import transcript as TR
from distributed_plonk_amd import verifier as VF
from tests import codec_ref as R
from tests.circuit_cases import _proved
from tests.test_gpu_codec import no_point_x, point_at

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3


@pytest.mark.parametrize("curve,cid", CURVES)
def test_batch_verify_bytes(gpu_workers, oracle, curve, cid):
    w, vk, pub, proofs = _proved(gpu_workers, oracle, curve, cid, nproofs=4)
    K = 4
    ref_key = VF.OpenKey.from_trapdoor(curve, TAU)
    key = VF.OpenKey.from_bytes(curve, TR.serialize_g1(curve, ref_key.g, False), CD.g2_to_bytes(curve, ref_key.h),
                                CD.g2_to_bytes(curve, ref_key.beta_h, "uncompressed"))
    blobs = [TR.serialize_proof(curve, p) for p in proofs]
    pub_bytes = b"".join(TR.serialize_fr(curve, x) for x in pub)
    st = {}
    assert VF.batch_verify_bytes(w, vk, key, [pub_bytes] * K, blobs, seed=1, stats=st) == [True] * K
    assert st["pairing_checks"] == 1 and st["decode_status"] == [0] * K and st["status"] == [0] * K

    nb = R.NBYTES[curve]
    sign = point_at(curve, 1) + nb - 1
    flip = lambda blob: blob[:sign] + bytes([blob[sign] ^ 0x80]) + blob[sign + 1:]       # -[w_1]: a point of the curve, not the prover's
    at = point_at(curve, 8)
    no_point = blobs[1][:at] + no_point_x(curve) + blobs[1][at + nb:]
    bad = [blobs[0], no_point, flip(blobs[2]), blobs[3]]
    got = VF.batch_verify_bytes(w, vk, key, [pub_bytes] * K, bad, seed=2, stats=st)
    assert got == [True, False, False, True]
    assert st["decode_status"] == [0, 1, 0, 0] and st["status"][2] == 0
    # the pairing checks are those of the bisection over a tree of four leaves [live, masked, bad, live]: the sums that contain leaf 2 fail
    want, checks = VF.bisect_tree(4, [True, False, True, True], lambda node: node not in (0, 2, 3 + 2))
    assert want == got and st["pairing_checks"] == checks == 4

    # three proofs, the wrong one in the middle: a padded fourth leaf, nothing masked by the decoder, and a bisection
    got = VF.batch_verify_bytes(w, vk, key, [pub_bytes] * 3, [blobs[0], flip(blobs[1]), blobs[2]], seed=4, stats=st)
    want, checks = VF.bisect_tree(4, [True] * 3, lambda node: node not in (0, 1, 3 + 1))
    assert got == want == [True, False, True] and st["pairing_checks"] == checks == 4
    assert st["decode_status"] == [0] * 3 and st["status"] == [0] * 3

    # the same verdicts from batch_verify on the decoded dicts (the proof that does not decode has none)
    dicts = [CD.proof_from_bytes(w, b) for i, b in enumerate(bad) if i != 1]
    with pytest.raises(ValueError, match="status 1"):
        CD.proof_from_bytes(w, bad[1])
    assert VF.batch_verify(w, vk, ref_key, [pub] * 3, dicts, seed=2) == [True, False, True]

    # a public input that is no canonical scalar rejects its proof alone
    r_bytes = R.fr_modulus(curve).to_bytes(32, "little")
    pubs = [pub_bytes, pub_bytes, r_bytes + pub_bytes[32:], pub_bytes]
    assert VF.batch_verify_bytes(w, vk, key, pubs, blobs, seed=3, stats=st) == [True, True, False, True]
    assert st["decode_status"] == [0, 0, 8, 0]
    assert VF.batch_verify_bytes(w, vk, key, [], []) == []
    with pytest.raises(ValueError):
        VF.batch_verify_bytes(w, vk, key, [pub_bytes], blobs)
