"""A pure-Python reference of the Rescue sponge, the Rescue counter-mode stream and the ElGamal / Rescue hybrid over the embedded Edwards
curves (a helper of the ElGamal tests, not a test; imports no project code — the permutation is tests/rescue_ref.py's, the group
tests/edwards_ref.py's).  Written from the definitions with Python integers:

    sponge(x_0 .. x_{L-1}; n_out)   s = (0, 0, 0, L);  per block b < ceil(L / 3):  s[j] += x[3b + j] (j < 3, 3b + j < L), s = permute(s);  -> s[0 : n_out]
    keystream(k, L)                 element i is permute((k, i div 3, 0, -1))[i mod 3]
    encrypt(ek, m, r)               E = [r] G,  S = [r] ek,  k = permute((S.x, S.y, 0, 0))[0],  ct_i = m_i + keystream(k, L)[i]   -> (E, ct)
    decrypt(dk, (E, ct))            S = [dk] E (E off the curve: the identity),  the same k,  m_i = ct_i - keystream(k, L)[i]
                                    -> (m, ok),  ok: E is on the curve and [l] E = (0, 1)"""
from tests import edwards_ref as E
from tests import rescue_ref as R

MODULI = R.MODULI
CURVES = R.CURVES


def sponge(curve, xs, n_out=1, rescue=None):
    r = MODULI[curve]
    xs = list(xs)
    L = len(xs)
    assert 1 <= L < 1 << 32 and n_out in (1, 2, 3)
    s = [0, 0, 0, L % r]
    for b in range((L + 2) // 3):
        for j in range(3):
            if 3 * b + j < L:
                s[j] = (s[j] + xs[3 * b + j]) % r
        s = R.permute(curve, s, rescue)
    return s[:n_out]


def stream_block(curve, k, j, rescue=None):
    """ks_j under key k: three residues"""
    r = MODULI[curve]
    return R.permute(curve, [k % r, j % r, 0, r - 1], rescue)[:3]


def keystream(curve, k, L, rescue=None):
    """the L first elements of the keystream under key k"""
    out = []
    for j in range((L + 2) // 3):
        out += stream_block(curve, k, j, rescue)
    return out[:L]


def stream(curve, k, text, decrypt=False, rescue=None):
    r = MODULI[curve]
    ks = keystream(curve, k, len(text), rescue)
    return [(x - z) % r if decrypt else (x + z) % r for x, z in zip(text, ks)]


def dh_key(curve, scalar, P, prm=None, rescue=None):
    """hash3(S.x, S.y, 0) for S = [scalar] P; a P off the curve counts as the identity"""
    if not E.on_curve(curve, P, prm):
        P = E.IDENTITY
    S = E.mul(curve, scalar, P, prm)
    return R.permute(curve, [S[0], S[1], 0, 0], rescue)[0]


def keygen(curve, dk, prm=None):
    return E.mul(curve, dk, E.params(curve, prm)["G"], prm)


def encrypt(curve, ek, msg, r, prm=None, rescue=None):
    """-> (E, ct)"""
    c = E.params(curve, prm)
    assert 0 <= r < c["l"]
    return E.mul(curve, r, c["G"], prm), stream(curve, dh_key(curve, r, ek, prm, rescue), msg, False, rescue)


def decrypt(curve, dk, ciphertext, prm=None, rescue=None):
    """-> (msg, ok)"""
    Ep, ct = ciphertext
    return stream(curve, dh_key(curve, dk, Ep, prm, rescue), ct, True, rescue), E.in_subgroup(curve, Ep, prm)
